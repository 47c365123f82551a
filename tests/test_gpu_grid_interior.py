"""GPU: the request-order loop of the one-lane grid kernel (csrc/hs_kernels.hpp hs_station_run<1, false, true, true>) takes a lean
body while every active lane of a wavefront is INTERIOR -- its request arrives, starts and departs inside the window, nobody
waits from an earlier launch, no two of its events share a nanosecond (csrc/hs_station.hpp req_interior / req_step_interior) --
and today's req_step otherwise.  Everything here is an exact comparison with the C oracle: the summary and the per-kind
histogram, every per-LP statistic (`total_service_s` bit for bit), every Sink record in order and `final_time_ns` (the elected
event beyond the end).  Debug flag 1 << 22 keeps small grids on the one-lane kernel; every test first checks that this is the
kernel that ran."""
import numpy as np
import pytest

import helpers as H
from oracle import hs_oracle as O

pytestmark = pytest.mark.gpu

ONE_LANE = 1 << 22


def _spec(n, rate=8.0, mean=0.1, end_s=5.0, mode="single", seed=77, name="interior"):
    return dict(name=name, n_chains=n, arr="poisson", rate=rate, svc="exp", mean=mean, concurrency=1, queue_cap=None,
                stop_after_s=None, downstream=True, end_s=end_s, rng="philox", seed=seed, mode=mode, trace=False)


def _on_uni_kernel(eng):
    from happy_simulator_amd import _native as N
    assert eng.run_path() & N.RUN_ONE_LANE_UNI, hex(eng.run_path())


def _check(spec, runs=None, ends=None):
    """Run the spec on the one-lane uniform kernel (to every end of `ends` in turn, then to the spec's end) against the oracle."""
    from test_gpu_parity import _compare_engine_to_oracle

    runs = runs if runs is not None else H.run_oracle_for_spec(spec)
    eng, p = H.engine_for_spec(spec, flags=ONE_LANE)
    with eng:
        for e in ends or ():
            eng.run_until(e)
            _on_uni_kernel(eng)
        eng.run_until(p["end_ns"])
        _on_uni_kernel(eng)
        _compare_engine_to_oracle(spec, eng, p, runs)
    return runs


def _outputs(eng):
    s = eng.summary()
    out = {"events": s.events_processed, "final": s.final_time_ns, "completed": s.requests_completed,
           "sink_records": s.sink_records, "by_kind": s.events_by_kind.copy()}
    out.update(eng.lp_stats())
    c, t, cr = eng.read_sinks()
    out.update(sink_counts=c, sink_t=t, sink_created=cr)
    return out


def _windowed_oracle(spec, windows):
    """_execute_until per window on the same heap (tests/test_gpu_parity.py test_reentrant_windows_match_oracle)."""
    n = spec["n_chains"]
    p = H.spec_chain_params(spec)
    g, nodes = H.oracle_graph_for(spec, list(range(n)), list(range(n)))
    return [(list(range(n)), nodes, O.run(g, p["end_ns"], seed=spec["seed"], windows=windows))]


# ---- 1. sizes: a partial wavefront, a partial workgroup, two workgroups
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_sizes(n):
    _check(_spec(n))


# ---- 2. no interior iteration at all / almost only interior ones
def test_a_window_without_interior_iterations():
    spec = _spec(128, end_s=0.05)
    runs = H.run_oracle_for_spec(spec)
    assert int(runs[0][2].completed.sum()) < 128               # fewer than one request per LP completes
    _check(spec, runs)


def test_a_window_of_almost_only_interior_iterations():
    spec = _spec(128, end_s=20.0)
    runs = H.run_oracle_for_spec(spec)
    want, _ = H.oracle_per_chain(spec, runs)
    assert (want["completed"] > 100).all()
    _check(spec, runs)


# ---- 3. lanes that finish far apart: a handful of iterations next to hundreds in one wavefront
def test_lanes_that_finish_far_apart():
    n = 256
    rates = [float(r) for r in np.geomspace(0.5, 50.0, n)]
    spec = _spec(n, rate=rates, mean=[0.8 / r for r in rates], end_s=3.0)
    runs = H.run_oracle_for_spec(spec)
    want, _ = H.oracle_per_chain(spec, runs)
    assert want["completed"].min() < 8 and want["completed"].max() > 100
    _check(spec, runs)


# ---- 4. ties inside the lean region: whole nanoseconds with mean gaps of 50 ns
def test_ties_inside_the_lean_region():
    n = 128
    spec = _spec(n, rate=2e7, mean=4e-8, end_s=15e-6)
    runs = H.run_oracle_for_spec(spec)
    _, sinks = H.oracle_per_chain(spec, runs)
    hit = 0
    for c in range(n):
        t, cr = (np.asarray(a, np.int64) for a in sinks[c])
        prev_done = np.concatenate(([np.iinfo(np.int64).min], t[:-1]))
        start = np.maximum(cr, prev_done)                        # one worker, FIFO: request k starts at max(a_k, D_{k-1})
        on_earlier_completion = any(cr[k] in set(t[:k].tolist()) for k in range(len(t)))
        hit += bool(on_earlier_completion or (t == start).any())
    assert hit >= n // 4, hit
    _check(spec, runs)


# ---- 5. windows: entering with requests waiting, one in service, a departure pending beyond the previous end
def _uneven_ends(rng, end_ns, k=40):
    ends = sorted(int(x) for x in rng.integers(1, end_ns, k - 8))
    for j in (3, 11, 19, 27):                                    # some only microseconds apart
        ends += [ends[j] + 1_000, ends[j] + 4_500]
    return sorted(ends)


def test_windows_equal_one_run_and_the_oracle():
    spec = _spec(256, end_s=10.0, seed=5)
    ends = _uneven_ends(np.random.default_rng(11), 10_000_000_000)
    assert len(ends) == 40
    _check(spec, _windowed_oracle(spec, ends), ends=ends)
    _check(spec)                                                 # one run to 10 s against the plain oracle run ...
    outs = []
    for ee in (ends, ()):                                        # ... and the two engine runs against each other
        eng, p = H.engine_for_spec(spec, flags=ONE_LANE)
        with eng:
            for e in ee:
                eng.run_until(e)
            eng.run_until(p["end_ns"])
            outs.append(_outputs(eng))
    for k in outs[0]:
        np.testing.assert_array_equal(np.asarray(outs[0][k]), np.asarray(outs[1][k]), err_msg=k)


# ---- 6. REPLICAS mode: the same kernel with a per-LP overshoot
@pytest.mark.parametrize("n", [65, 300])
def test_sizes_in_replicas_mode(n):
    _check(_spec(n, mode="replicas"))


# ---- 7. a log that fills inside the lean body: the capacity guards
def test_a_log_that_fills_is_reported_and_stores_nothing_out_of_bounds():
    from happy_simulator_amd import _native as N

    spec = _spec(64, end_s=5.0)
    eng, p = H.engine_for_spec(spec, log_capacity=16, flags=ONE_LANE)
    with eng:
        with pytest.raises(N.EngineError) as ei:
            eng.run_until(p["end_ns"])
        assert ei.value.code == N.HS_E_OVERFLOW
        _on_uni_kernel(eng)
    eng, p = H.engine_for_spec(spec, log_capacity=16, flags=ONE_LANE)
    with eng:
        with pytest.raises(N.EngineError) as ei:
            eng.bench_runs(p["end_ns"], 2)
        assert ei.value.code == N.HS_E_OVERFLOW
    _check(spec)                                                 # a following engine on the same device runs clean


# ---- 8. the divisor gate: the uniform kernel divides with multiply + FMA untested, so such grids must not reach it
@pytest.mark.parametrize("which", ["rate", "lambda"])
def test_divisors_the_fast_quotient_is_not_exact_for_run_on_the_generic_kernel(which):
    """A rate whose significand is all ones (Markstein's theorem excludes it), and -- the reciprocal of a binary64 never has
    such a significand (tests/test_uni_gate_host.py) -- a lambda = 1 / mean beyond the exponents the sequence stays normal for."""
    from happy_simulator_amd import _native as N
    from test_gpu_parity import _compare_engine_to_oracle

    ones = float(np.nextafter(2.0, 0.0))
    spec = _spec(64, rate=ones, mean=0.4) if which == "rate" else _spec(64, rate=8.0, mean=2.0 ** -201)
    runs = H.run_oracle_for_spec(spec)
    eng, p = H.engine_for_spec(spec, flags=ONE_LANE)
    with eng:
        eng.run_until(p["end_ns"])
        assert eng.run_path() & N.RUN_ONE_LANE and not eng.run_path() & N.RUN_ONE_LANE_UNI, hex(eng.run_path())
        _compare_engine_to_oracle(spec, eng, p, runs)


# ---- 9. windows that begin at both parities of the two stream positions (the producer starts inside a Philox block)
def test_windows_begin_at_odd_and_even_stream_positions():
    from test_gpu_parity import _compare_engine_to_oracle

    spec = _spec(256, end_s=10.0, seed=9)
    ends = [int(x) for x in np.linspace(0.13e9, 9.7e9, 24)]
    runs = _windowed_oracle(spec, ends)
    seen = np.zeros((2, 2, 256), bool)                           # [stream][parity][LP]
    eng, p = H.engine_for_spec(spec, flags=ONE_LANE)
    with eng:
        for e in ends:
            eng.run_until(e)
            _on_uni_kernel(eng)
            st = eng.lp_stats()
            arr_k = st["generated"]                              # arrival draws consumed: one per tick
            svc_k = st["completed"] + st["active"]               # service draws consumed: one per start
            for s, k in enumerate((arr_k, svc_k)):
                seen[s, 0] |= (k % 2 == 0)
                seen[s, 1] |= (k % 2 == 1)
        assert seen.any(axis=2).all(), "windows began at one parity only"
        eng.run_until(p["end_ns"])
        _compare_engine_to_oracle(spec, eng, p, runs)
