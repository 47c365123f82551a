"""GPU: RateLimitedEntity on the single-heap loop (csrc/hs_graph.hip kEvLimRequest / kEvLimPoll) against the recorded live
reference (tests/golden/live_rate_limiter/, written by tests/golden/make_golden_rate_limiter.py).  Every comparison is exact
equality: Sink records, per-entity statistics, the limiters' counters, queue depth, time series and final policy state, probe
samples, event totals, the first event beyond the end.

The 1-ns guards (`wait == Duration.ZERO -> Duration(1)`): the recorded search found a run that meets the guard for every one of the
four policies (test_guard_cases; the recording holds the try it was found at), so none had to be left out."""
import numpy as np
import pytest

import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import rate_limiter_specs as RS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine
from recorded import RATE_LIMITER as RR

pytestmark = pytest.mark.gpu

# what the engine has no counterpart for (the reference heap's length, the wrapper's guard count) or what is compared in a form of
# its own (by_kind: the engine reports the public fifteen kinds; the limiters' two per node; trace: test_record_order_follows_the_trace)
_NOT_COMPARED = {"trace", "by_kind", "pending_events", "lim_guard_hits", "entity_summaries"}
_BY_KIND_SLICES = [("by_kind", N.EV_KINDS), (lambda got: got["lim_events"].sum(axis=0), N.EV_KINDS + 2)]      # (the limiters' two kinds: per limiter)


def _equals_the_recording(spec, sim, pools, ref):
    got = GF.results(spec, sim, pools, "rate_limiter")
    FC.compare(spec["name"], got, ref, _NOT_COMPARED, _BY_KIND_SLICES)
    es = sim.summary.entities
    assert {x.name: [es[x.name].entity_type, es[x.name].events_handled, es[x.name].queue_stats is None]
            for x in pools["limiter"]} == ref["entity_summaries"]
    return got


def _run(spec, **kw):
    sim, pools = GF.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph)
    return sim, pools


@pytest.mark.parametrize("name", sorted(RS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = RS.FIXTURES[name]
    sim, pools = _run(spec)
    got = _equals_the_recording(spec, sim, pools, RR.get("case", spec))
    if name.endswith("_constant"):
        kind = name[:-len("_constant")]
        assert tuple(got["lim_stats"][0, :4]) + (got["total_events"],) == RS.ISSUE_VALUES[kind]
    if name == "nodes_beyond_lds":
        # 70 chains are 70 parts of four nodes; on ONE heap the 280 nodes' parameters and state stay in HBM
        import happy_simulator_amd.simulation as S

        assert sim._graph.arrays.n > 192 and sim._graph_parts > 1
        old, S.MAX_PARTS = S.MAX_PARTS, 1
        try:
            one_sim, one_pools = _run(spec)
        finally:
            S.MAX_PARTS = old
        assert one_sim._graph_parts == 1
        _equals_the_recording(spec, one_sim, one_pools, RR.get("case", spec))
        # ... and on the side-by-side kernel, around ITS 48 LDS node rows (hs_graph_run_batch; test_graph_host.py pins the constant):
        # 6 heaps of 48 / 44 nodes (the last sizes whose rows stay in LDS), 5 heaps of 56 and 2 heaps of 140 (rows in HBM).  Every
        # heap holds all four policies; a fall-back to one heap would leave _graph_parts == 1
        from happy_simulator_amd.graph_engine import split_parts

        for max_parts, sizes in ((6, {44, 48}), (5, {56}), (2, {140})):
            heaps = [b for _ids, _pos, b in split_parts(sim._graph.arrays, max_parts)]
            assert {b.n for b in heaps} == sizes
            assert all(len(set(b.lim_policy[b.kind == N.NODE_RATE_LIMITER].tolist())) == 4 for b in heaps)
            old, S.MAX_PARTS = S.MAX_PARTS, max_parts
            try:
                few_sim, few_pools = _run(spec)
            finally:
                S.MAX_PARTS = old
            assert few_sim._graph_parts == max_parts
            _equals_the_recording(spec, few_sim, few_pools, RR.get("case", spec))


@pytest.mark.parametrize("k", range(RS.N_RANDOM))
def test_random_graph_with_limiters_equals_the_reference(k):
    spec = RS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, RR.get("case", spec))


@pytest.mark.parametrize("kind", RS.POLICIES)
def test_guard_cases(kind):
    """The first seeded run in which `time_until_available` of this policy answered Duration(1) in the reference."""
    rec = RR.get("guard", kind)
    assert rec["tries"] >= 0, f"the search of {RS.GUARD_TRIES} tries found no run that meets the {kind} guard"
    spec = RS.guard_spec(kind, rec["tries"])
    assert int(rec["result"]["lim_guard_hits"].sum()) > 0
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, rec["result"])


_TRACED = [n for n in sorted(RS.FIXTURES) if len(RS.FIXTURES[n]["servers"]) <= 16]      # (the generator's own rule)


@pytest.mark.parametrize("name", _TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event; kinds 15 / 16 = a
    Request at a limiter / its poll): every Request at a limiter and every Sink event, in the one processing order of the whole graph
    -- so a limiter's forward lands where the reference's does among the other events of its nanosecond -- and every drained Request
    at a poll of its limiter, in order."""
    spec = RS.FIXTURES[name]
    trace = RR.get("case", spec)["trace"]
    _sim, _pools, g, eng, end_ns, _start, _c = FC.engine(spec)
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        polls = {int(i): eng.limiter(int(i))["polls_handled"] for i in np.nonzero(g.arrays.kind == N.NODE_RATE_LIMITER)[0]}
    kind = g.arrays.kind[node]
    lim = kind == N.NODE_RATE_LIMITER
    arrivals = (lim & (v != N.LIMITER_DRAINED)) | (kind == N.NODE_SINK)
    want = FC.live_rows(trace, (N.EV_KINDS, N.EV_NAMES.index("sink")))
    assert len(want) > 0 and np.array_equal(np.stack([t[arrivals], node[arrivals]], axis=1), want[:, [0, 2]])
    poll_rows = trace[trace[:, 1] == N.EV_KINDS + 1]
    assert {int(i): int((poll_rows[:, 2] == i).sum()) for i in polls} == polls
    it = iter(map(tuple, poll_rows[:, [0, 2]].tolist()))
    drained = lim & (v == N.LIMITER_DRAINED)
    assert all(row in it for row in zip(t[drained].tolist(), node[drained].tolist()))      # a subsequence, in order


def test_the_kernels_window_start_is_pythons():
    """FixedWindowPolicy._get_window_start on the device (hs_debug_window_start: the loop's own py_floordiv_pos / exact_fmod_pos)
    against CPython's float `//`: the recorded window sizes at clocks of 0, 10^5 s and 4 x 10^6 s (one ulp of to_seconds is about a
    nanosecond there) around the window edges, windows down to a nanosecond and beyond the clock, random pairs."""
    rng = np.random.default_rng(3)
    ws = (0.1, 0.3, 1.0 / 3.0, 0.5, 0.75, 1.0, 1e-9, 2.5e-7, 7.0, 1e7, 2.0 ** -20, 3.0 * 2.0 ** 40)
    base = [0, 1, 99_999_999, 100_000_000, 100_000_001, 299_999_999, 300_000_000, 333_333_333, 333_333_334]
    nows = [b + off for off in (0, 10 ** 14, 4 * 10 ** 15) for b in base] + rng.integers(0, 5 * 10 ** 15, 600).tolist()
    now = np.array([x for x in nows for _ in ws] + rng.integers(0, 2 ** 62, 4000).tolist(), np.int64)
    w = np.array([x for _ in nows for x in ws] + np.exp(rng.uniform(np.log(1e-9), np.log(1e9), 4000)).tolist(), np.float64)
    div, start = np.zeros(len(now), np.float64), np.zeros(len(now), np.int64)
    rc = N.lib().hs_debug_window_start(0, len(now), now.ctypes.data, w.ctypes.data, div.ctypes.data, start.ctypes.data)
    assert rc == N.HS_OK, N.lib().hs_last_global_error()
    want_div = [(int(a) / 1e9) // float(b) for a, b in zip(now, w)]
    bad = [i for i, (a, b) in enumerate(zip(div.tolist(), want_div)) if a != b]
    assert not bad, (len(bad), int(now[bad[0]]), float(w[bad[0]]), float(div[bad[0]]), want_div[bad[0]])
    assert start.tolist() == [int(d * float(b) * 1e9) for d, b in zip(want_div, w)]       # Instant.from_seconds(div * window)


def test_windows_equal_one_run_and_the_reference():
    spec = RS.FIXTURES["windows"]
    ref = RR.get("case", spec)
    sim, pools, _ = FC.engine_run(spec, list(spec["windows"]) + [spec["end_s"]])
    got = _equals_the_recording(spec, sim, pools, ref)
    one_sim, one_pools = _run({k: v for k, v in spec.items() if k != "windows"})
    one = GF.results(spec, one_sim, one_pools, "rate_limiter")
    for key in got:
        assert np.array_equal(np.asarray(got[key]), np.asarray(one[key])), key


def _overload_spec():
    # 2 000 Requests / s against one per second: ~3 000 Requests wait in the limiter's list, more than the Request pool starts with
    return RS._chain("growth", ["leaky", 1.0], source="poisson", rate=2000.0, cap=5000, end_s=1.5, seed=3)


def test_growth_from_capacities_of_one_equals_the_plain_run():
    spec = _overload_spec()
    grown_sim, grown_pools, _ = FC.engine_run(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1)
    plain_sim, plain_pools = _run(spec)
    grown, plain = GF.results(spec, grown_sim, grown_pools, "rate_limiter"), GF.results(spec, plain_sim, plain_pools, "rate_limiter")
    assert plain["lim_stats"][0, 4] > 2000                        # the queue outgrew the initial pool (1 024 + 4 n Requests)
    for key in plain:
        assert np.array_equal(np.asarray(grown[key]), np.asarray(plain[key])), key


def test_replicas_equal_single_runs():
    spec = RS.FIXTURES["two_in_a_row"]
    built = []

    def build_fn():
        sim, pools = GF.build(spec)
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=500)
    assert len(results) == 64
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph)
        got = GF.results(spec, sim, pools, "rate_limiter")
        one_sim, one_pools = _run(spec, seed=500 + i)
        one = GF.results(spec, one_sim, one_pools, "rate_limiter")
        for key in one:
            assert np.array_equal(np.asarray(got[key]), np.asarray(one[key])), (i, key)
    assert len({GF.results(spec, s, p, "rate_limiter")["total_events"] for s, p in built}) > 8       # (the seeds matter)


def _chains_spec(n, source, name):
    return dict(name=name, topology="graph", n_sinks=n, links=[], routers=[], lbs=[], end_s=2.0, seed=11,
                servers=[dict(mean=0.03, c=1, cap=None, out=["sink", j], svc="exp") for j in range(n)],
                limiters=[dict(policy=list(RS.FOUR[RS.POLICIES[j % 4]]), cap=3, out=["server", j]) for j in range(n)],
                sources=[dict(kind=source, rate=6.0 + (j % 3 if source == "poisson" else 0), to=["limiter", j]) for j in range(n)])


@pytest.mark.parametrize("source", ["poisson", "constant"])
def test_600_chains_as_parts_equal_one_heap(source):
    """Disconnected Source -> limiter -> Server -> Sink chains in ONE Simulation.  Poisson Sources: the parts run side by side.
    Lock-step constant Sources: every part meets a timestamp group only the whole Simulation orders (a pre-run tick next to run-time
    events), the run is repeated on one heap -- either way the result is the one heap's."""
    import happy_simulator_amd.simulation as S

    spec = _chains_spec(600, source, f"chains_{source}")
    sim, pools = _run(spec)
    assert sim._graph_parts > 1 if source == "poisson" else sim._graph_parts == 1
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    got, one = GF.results(spec, sim, pools, "rate_limiter"), GF.results(spec, one_sim, one_pools, "rate_limiter")
    for key in one:
        assert np.array_equal(np.asarray(got[key]), np.asarray(one[key])), key
    assert got["lim_stats"][:, 2].sum() > 100 and got["total_events"] == int(got["by_kind"].sum()) + int(got["lim_events"].sum())


def test_auto_terminating_run_ends_where_the_reference_ends():
    """end_time = Infinity: the polls are daemon events, the run ends when they are all that is pending -- after 4 events, with two
    Requests still queued.  With an end, the same graph processes its polls like any event."""
    spec = RS.FIXTURES["auto_terminate"]
    sim, pools = _run(spec)
    lim = pools["limiter"][0]
    assert sim.summary.total_events_processed == 4 and lim.stats == hs.RateLimitedEntityStats(3, 1, 2, 0)
    assert lim.queue_depth == 2 and lim._poll_scheduled and pools["sink"][0].events_received == 1
    ended = dict(spec, auto=False, end_s=5.0)
    sim, pools = _run(ended)
    assert pools["limiter"][0].stats == hs.RateLimitedEntityStats(3, 3, 2, 0) and pools["sink"][0].events_received == 3


def test_a_limiter_without_a_policy_is_a_state_error():
    sim, _pools = GF.build(RS.FIXTURES["token_constant"])
    a = sim.lowered().arrays
    a.lim_policy = None                                            # (the handle is created, no policy follows)
    with GraphEngine(a, seed=1) as eng:
        with pytest.raises(N.EngineError) as e:
            eng.run_until(10 ** 9)
        assert e.value.code == N.HS_E_STATE and "without a policy" in str(e.value)


def test_the_max_events_refusal_names_a_fixed_window_as_the_likely_cause():
    """The run-time refusal at max_events says what a user can act on: with a FixedWindowPolicy in the graph it names the window
    that is no binary fraction (the reference's own livelock); without one the text is what it was."""
    for fixture, named in (("fixed_constant", True), ("token_constant", False)):
        sim, _pools = GF.build(RS.FIXTURES[fixture])
        with GraphEngine(sim.lowered().arrays, seed=1, max_events=50) as eng:
            with pytest.raises(N.EngineError, match="max_events") as e:
                eng.run_until(5 * 10 ** 9)
            assert e.value.code == N.HS_E_UNSUPPORTED and ("FixedWindowPolicy" in str(e.value)) == named
