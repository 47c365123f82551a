"""MI355X: the engines at the ABSOLUTE time magnitudes where their exact arithmetic switches paths.

Every gate below is decided on the host from absolute times, and every fast path rests on an error bound that is tightest at the
top of its range.  Each placement here is a short run (2 s, or a few thousand events) put just below and just above one gate,
compared bit for bit with the C oracle run at the same offset, and the path the engine reports (hs_engine_run_path /
hs_lb_run_path) is asserted, so that a gate that moves leaves these tests failing instead of covering nothing.

| gate | where | what switches |
|---|---|---|
| horizon < 2^39 ns | `hs_engine.hip` wide_lanes, `hs_kernels_wave.hpp` | one wavefront per LP, speculated whole-ns arrival steps (margin 2^-10) <-> `hs_station_wide<K>`: K = 8 up to 4 096 LPs, K = 4 up to 16 384 |
| horizon < 2^40 | `hs_lb.hip` run_async, `lb_step_encode` | LB Sources' speculated steps <-> the reference's ten-op step |
| run span < 2^44 - 3 | `hs_engine.hip` (`kPkNever`, 44-bit packed link bounds) | `hs_net_async` <-> the windowed fallback |
| horizon < 2^50, rates > 1e-3, horizon + longest service < 2^52 | `hs_lb.hip` hs_lb_create | `hs_lbk_scan<true>` (times as binary64 whole ns) <-> `<false>` |
| horizon < 2^51, rate > 1e-3, mean < 1e4 | `hs_engine.hip` set_stations / set_network | the `UNI` station and network kernels (binary64 time algebra, `i64_from_whole_d` mask) <-> int64 |
| tb + sb <= 64 | `hs_lb.hip` slot_bits | shared-Sink merge packs `created_at << slot_bits` <-> gathers `created_at` |
| tb + bb <= 64, tb <= 56 | `hs_lb.hip` hs_lb_create | named refusal of the sort key |
| horizon + one longest step < ~2^63 | every engine, at construction | named refusal (the reference's ints never overflow) |
| start_time < 0 | every engine, `Simulation.run` | named refusal |

All offsets are integer nanoseconds; every absolute time of a configuration (the end, `stop_after`, window ends) moves with them.
"""
import numpy as np
import pytest

import happy_simulator_amd as hs
from happy_simulator_amd import Instant
from happy_simulator_amd import _native as N
from happy_simulator_amd.engine import StationArrays, StationEngine, debug_time_ops
from happy_simulator_amd.lb_engine import LbBackendArrays, LbSourceArrays, LoadBalancerEngine
from oracle import hs_oracle as O

import helpers as H
from test_gpu_ring import _check_against_oracle as check_ring
# hs_engine.hip wide_lanes for a fresh uniform grid: shared with tests/test_gpu_wide.py and tests/test_gpu_uniform_kernels_oracle.py
from uniform_cases import device_lanes as _device_lanes, expected_uniform_kernel as _expected_uniform_kernel

pytestmark = pytest.mark.gpu

SPAN = 2_000_000_000
WAVE, WIDE, UNI, ONE = N.RUN_WAVE, N.RUN_WIDE, N.RUN_ONE_LANE_UNI, N.RUN_ONE_LANE
KERNELS = N.RUN_ONE_LANE | N.RUN_ONE_LANE_UNI | N.RUN_WIDE | N.RUN_WAVE | N.RUN_TANDEM | N.RUN_SINGLE_HEAP


def _lanes(path):
    return (path >> N.RUN_LANES_SHIFT) & 0xFF


# ---- the device time algebra against Python's exact ints -----------------------------------------------------------------------
def _time_inputs():
    rng = np.random.default_rng(39)
    mags = np.exp2(rng.uniform(0.0, 62.0, 4000)).astype(np.int64)
    ns = [int(v) for v in mags] + [-int(v) for v in mags[:2000]]
    for k in (39, 40, 44, 50, 51, 52, 53, 62):
        ns += [(1 << k) - 1, 1 << k, (1 << k) + 1, -((1 << k) + 1)]
    ns += [0, 1, -1]
    return ns


def test_time_ops_equal_python_semantics():
    """seconds_from_ns / ns_from_seconds and their binary64 forms (csrc/hs_device.hpp) against `float(ns) / 1_000_000_000` and
    `int(x * 1_000_000_000)` (Instant.to_seconds / from_seconds) at magnitudes 2^0 .. 2^62, both signs, and around every gate.  The
    binary64 forms equal the int64 forms on whole ns in [0, 2^52) -- the range the gates keep them in -- and differ above it."""
    ns = _time_inputs()
    secs = [float(t) / 1_000_000_000 for t in ns]
    out = debug_time_ops(np.array(ns, np.int64), np.array(secs, np.float64))
    for i, (t, x) in enumerate(zip(ns, secs)):
        assert out["seconds_from_ns"][i] == x, t
        assert out["seconds_from_ns_d"][i] == x, t            # (the same sequence from the same binary64 value)
        want = int(x * 1_000_000_000)
        assert out["ns_from_seconds"][i] == want, (t, x)
        assert out["ns_from_seconds_d"][i] == float(want), (t, x)
    whole = np.array([0 <= t < (1 << 52) for t in ns])
    got = out["i64_from_whole_d"]
    for i, t in enumerate(ns):
        if whole[i]:
            assert got[i] == t and float(t) == t, t
        else:       # (true by construction -- the mask lands in [0, 2^52) -- kept as the statement of the range the gates keep)
            assert got[i] != t, t
    odd = [t for t in ns if t > (1 << 53) and t % 2 == 1]
    assert odd and all(int(float(t)) != t for t in odd)        # float(ns) itself rounds above 2^53


# ---- uniform grids (StationArrays.uniform) -------------------------------------------------------------------------------------
def _chains(n, start, end, seed=9, rate=2.0, mean=0.1, windows=(), tweak=None):
    """A uniform grid at [start, end] against the oracle: everything _compare_engine_to_oracle compares.  Returns the path bits of
    every run_until."""
    g = O.mm1_chains(n, rate=rate, mean=mean)
    st = StationArrays.uniform(n, rate=rate, mean=mean)
    if tweak:
        tweak(g, st)
    r = O.run(g, end, start_ns=start, seed=seed)
    paths = []
    with StationEngine(st, mode=N.MODE_SINGLE, horizon_ns=end, start_ns=start, seed=seed) as eng:
        for w in (*windows, end):
            eng.run_until(w)
            paths.append(eng.run_path())
        s = eng.summary()
        stats = eng.lp_stats()
        counts, t, cr = eng.read_sinks()
    assert (s.events_processed, s.final_time_ns) == (r.events_processed, r.final_time_ns)
    np.testing.assert_array_equal(s.events_by_kind, r.events_by_kind)
    srv = np.arange(n) * 2 + n
    np.testing.assert_array_equal(stats["generated"], r.generated[:n])
    for k, arr in (("accepted", r.accepted), ("completed", r.completed), ("queue_depth", r.depth), ("active", r.active),
                   ("total_service_s", r.total_service_s)):
        np.testing.assert_array_equal(stats[k], arr[srv], err_msg=k)
    sinks = sorted(r.sinks)
    np.testing.assert_array_equal(counts, [len(r.sinks[i][0]) for i in sinks])
    np.testing.assert_array_equal(t, np.concatenate([r.sinks[i][0] for i in sinks]))
    np.testing.assert_array_equal(cr, np.concatenate([r.sinks[i][1] for i in sinks]))
    assert len(t) == 0 or t.min() > start
    return paths


E39, E51 = (1 << 39) - 1, (1 << 51) - 1


@pytest.mark.parametrize("n,start,end,kernel,lanes,f64", [
    (64, E39 - SPAN, E39, WAVE, 8, True), (4096, E39 - SPAN, E39, WAVE, 8, True), (4097, E39 - SPAN, E39, WAVE, 16, True),
    (64, 1 << 39, (1 << 39) + SPAN, WIDE, 8, True), (4096, 1 << 39, (1 << 39) + SPAN, WIDE, 8, True),
    (4097, 1 << 39, (1 << 39) + SPAN, WIDE, 4, True), (16384, 1 << 39, (1 << 39) + SPAN, WIDE, 4, True),
    (16385, 1 << 39, (1 << 39) + SPAN, UNI, 0, True),
    (64, E51 - SPAN, E51, WIDE, 8, True), (16385, E51 - SPAN, E51, UNI, 0, True),
    (64, 1 << 51, (1 << 51) + SPAN, ONE, 0, False), (16385, 1 << 51, (1 << 51) + SPAN, ONE, 0, False),
    (64, (1 << 53) + 1, (1 << 53) + 1 + SPAN, ONE, 0, False),
], ids=lambda v: str(v))
def test_uniform_grid_at_offset(n, start, end, kernel, lanes, f64):
    """The table's K and workgroup shapes are those of a whole MI355X (256 CUs); on a partitioned device the same rule
    (hs_engine.hip wide_lanes) is evaluated with its CU count."""
    (path,) = _chains(n, start, end)
    if _device_lanes() != 256 * 4 * 64:
        kernel, lanes = _expected_uniform_kernel(n, end, _device_lanes(), f64)
    assert path & KERNELS == kernel, hex(path)
    assert _lanes(path) == lanes, hex(path)
    assert bool(path & N.RUN_F64_TIMES) == f64, hex(path)


def test_uniform_grid_windows_across_2_39_and_2_51():
    """Windows whose ends straddle a gate: the horizon decides the kernel (the first window on K lanes, the next continues on one
    lane), and the state the first window leaves must continue identically."""
    paths = _chains(64, (1 << 39) - SPAN // 2, (1 << 39) + SPAN // 2, windows=((1 << 39) - 1, 1 << 39))
    assert paths[0] & KERNELS == WIDE and _lanes(paths[0]) == 8, [hex(p) for p in paths]     # (64 LPs: K = 8 on any device)
    assert all(p & KERNELS == UNI for p in paths[1:]), [hex(p) for p in paths]
    paths = _chains(64, (1 << 51) - SPAN // 2, (1 << 51) + SPAN // 2, windows=((1 << 51) - 1, 1 << 51))
    assert all(p & KERNELS == ONE and not p & N.RUN_F64_TIMES for p in paths), [hex(p) for p in paths]


@pytest.mark.parametrize("rate0,mean0,f64", [(1.000001e-3, 0.1, True), (1e-3, 0.1, False), (2.0, 9999.999, True), (2.0, 1e4, False)])
def test_uniform_grid_rate_and_mean_gates(rate0, mean0, f64):
    """One LP at the rate / mean bound of the binary64 time algebra: just inside it the grid stays on the uniform kernels."""
    n = 64

    def tweak(g, st):
        g.rate[0] = rate0
        g.lat_mean[n] = mean0
        st.src_rate[0] = rate0
        st.svc_mean_s[0] = mean0

    (path,) = _chains(n, 1 << 40, (1 << 40) + SPAN, tweak=tweak)
    assert bool(path & N.RUN_F64_TIMES) == f64, hex(path)
    assert path & KERNELS == (WIDE if f64 else ONE), hex(path)


# ---- station families (tests/random_specs.py shapes) at offsets ------------------------------------------------------------
def _family_specs():
    base = dict(rng="philox", mode="single", n_chains=12, arr="poisson", rate=6.0, svc="exp", mean=0.1, end_s=2.0, seed=5)
    return {
        "station": dict(base),
        "tie": dict(base, arr="constant", rate=10.0, svc="const", mean=0.1),
        "multi_source": dict(base, more_sources=[[["poisson", 3.0]]] * 12),
        "workers_stop": dict(base, n_chains=8, concurrency=2, stop_after_s=1.5),
        "probes": dict(base, probes=[["depth", 0.25]] * 12),
    }


@pytest.mark.parametrize("family", sorted(_family_specs()))
@pytest.mark.parametrize("start", [1 << 39, (1 << 51) - SPAN - 1, (1 << 53) + 1], ids=["2^39", "2^51-span-1", "2^53+1"])
def test_station_family_at_offset(family, start):
    """General station configurations (several Sources per Server, ties of constant arrivals, workers with stop_after, Probes) with
    every absolute time shifted by `start` (spec["start_ns"]): the oracle and the engine agree bit for bit.  The end of the middle
    placement is 2^51 - 1, the top of the binary64 range."""
    from test_gpu_parity import _compare_engine_to_oracle

    spec = dict(_family_specs()[family], start_ns=start)
    runs = H.run_oracle_for_spec(spec)
    eng, p = H.engine_for_spec(spec)
    with eng:
        eng.run_until(p["end_ns"])
        path = eng.run_path()
        _compare_engine_to_oracle(spec, eng, p, runs)
    f64 = p["end_ns"] < (1 << 51)
    assert bool(path & N.RUN_F64_TIMES) == f64, hex(path)
    if family == "station":             # every LP Poisson -> Exp, c = 1: the uniform kernels while the times are binary64
        assert path & KERNELS == (WIDE if f64 else ONE) and _lanes(path) == (8 if f64 else 0), hex(path)
    else:                               # the general one-lane kernel (behind a prologue where one exists)
        assert path & ONE and not path & (WIDE | WAVE | UNI), hex(path)


# ---- networks ---------------------------------------------------------------------------------------------------------------
def _ring(spec, start, end, flags):
    gr, nodes = H.oracle_ring_graph(spec)
    r = O.run(gr, end, start_ns=start, seed=spec["seed"])
    st, net, cap, _ = H.ring_arrays(spec)
    with StationEngine(st, mode=N.MODE_SINGLE, horizon_ns=end, start_ns=start, seed=spec["seed"], log_capacity=cap, network=net) as eng:
        if flags:
            eng.set_debug_flags(flags)
        eng.run_until(end)
        path = eng.run_path()
        check_ring(spec, eng, r, nodes)
    return path


RINGS = {
    "ring": dict(n=48, ext_rate=4.0, mean=0.1, lat_min=0.001, jitter_mean=0.01, seed=10),
    "jitter_ring": dict(n=32, ext_rate=3.0, mean=0.05, lat_min=0.002, jitter_mean=0.2, seed=12),
    "multi_source_ring": dict(n=24, ext_rate=2.0, mean=0.1, lat_min=0.001, jitter_mean=0.01, seed=13,
                              more_sources=[[["poisson", 1.5]]] * 24),
}


@pytest.mark.parametrize("flags", [0, 16], ids=["async", "windowed"])
@pytest.mark.parametrize("name", sorted(RINGS))
@pytest.mark.parametrize("start,uni", [((1 << 51) - SPAN - 1, True), (1 << 51, False), ((1 << 53) + 1, False)],
                         ids=["2^51-span", "2^51", "2^53+1"])
def test_ring_at_offset(name, flags, start, uni):
    spec = dict(RINGS[name], topology="ring", end_s=SPAN / 1e9)
    path = _ring(spec, start, start + SPAN, flags)
    if flags == 16:
        assert path & N.RUN_NET_WINDOWED and not path & N.RUN_NET_ASYNC, hex(path)
    else:
        assert path & N.RUN_NET_ASYNC, hex(path)
        if "more_sources" not in spec:      # (several Sources per Server: the PF instantiation, never the uniform one)
            assert bool(path & N.RUN_NET_ASYNC_UNI) == uni, hex(path)
    assert bool(path & N.RUN_F64_TIMES) == (uni and "more_sources" not in spec) or "more_sources" in spec


@pytest.mark.parametrize("span,asynchronous", [((1 << 44) - 4, True), ((1 << 44) - 3, False)], ids=["under", "at"])
def test_slow_ring_at_the_packed_bound_span(span, asynchronous):
    """A ring with slow Sources whose run spans just under / exactly at the 44-bit packed link bound (4.9 h of simulated time, a
    few thousand events): the asynchronous engine below it, the windowed one at it."""
    spec = dict(n=8, ext_rate=0.02, mean=0.1, lat_min=1.0, jitter_mean=0.5, seed=14, topology="ring", end_s=span / 1e9)
    start = 1 << 30
    path = _ring(spec, start, start + span, 0)
    assert bool(path & N.RUN_NET_ASYNC) == asynchronous, hex(path)
    assert bool(path & N.RUN_NET_WINDOWED) == (not asynchronous), hex(path)


# ---- the load balancer ------------------------------------------------------------------------------------------------------
def _lb(start, end, S=8, B=16, rate=20.0, mean=0.1, strategy="chash", conc=1, svc="exp", shared=True, stop_after=None, seed=11,
        expect_sink_order=True):
    spec = dict(n_sources=S, n_backends=B, rate=rate, mean=mean, vnodes=100, n_clients=5000, end_s=(end - start) / 1e9, seed=seed,
                concurrency=conc, shared_sink=shared, strategy=strategy, svc=svc)
    g, p = H.oracle_lb_graph_ext(spec)
    stop = -1 if stop_after is None else start + stop_after
    for i in range(S):
        g.stop_after_ns[i] = stop
    r = O.run(g, end, start_ns=start, seed=seed)
    src = LbSourceArrays(n=S, src_rate=np.full(S, float(rate)), n_clients=np.full(S, 5000, np.int64),
                         src_stop_after_ns=np.full(S, stop, np.int64))
    be = LbBackendArrays(n=B, names=[f"srv{j}" for j in range(B)], concurrency=np.full(B, conc, np.int32),
                         svc_kind=np.full(B, N.LAT_EXPONENTIAL if svc == "exp" else N.LAT_CONSTANT, np.uint8),
                         svc_mean_s=np.full(B, float(mean)))
    strat = {"chash": N.LB_CONSISTENT_HASH, "round_robin": N.LB_ROUND_ROBIN, "random": N.LB_RANDOM}[strategy]
    with LoadBalancerEngine(src, be, virtual_nodes=100, horizon_ns=end, start_ns=start, seed=seed, shared_sink=shared,
                            strategy=strat) as eng:
        eng.run(end)
        path = eng.run_path()
        H.compare_lb_engine_with_oracle(eng, p, r, check_sink_order=expect_sink_order)
    return path, r


E40, E50 = (1 << 40) - 1, (1 << 50) - 1
LB_PLACES = [(E40 - SPAN, E40, True, True), (1 << 40, (1 << 40) + SPAN, False, True),
             (E50 - SPAN, E50, False, True), (1 << 50, (1 << 50) + SPAN, False, False)]


@pytest.mark.parametrize("strategy", ["chash", "round_robin", "random"])
@pytest.mark.parametrize("start,end,margin,f64", LB_PLACES, ids=["2^40-1", "2^40", "2^50-1", "2^50"])
def test_lb_at_offset(strategy, start, end, margin, f64):
    """Three strategies just below / at 2^40 (speculated Source steps at their largest A, then off) and 2^50 (binary64 times)."""
    path, _ = _lb(start, end, strategy=strategy)
    assert bool(path & N.LB_RUN_MARGIN) == margin, hex(path)
    assert bool(path & N.LB_RUN_LEAN) == margin, hex(path)
    assert bool(path & N.LB_RUN_F64_TIMES) == f64, hex(path)
    assert path & N.LB_RUN_SCAN, hex(path)


@pytest.mark.parametrize("start,end,f64", [(E40 - SPAN, E40, True), (1 << 50, (1 << 50) + SPAN, False)], ids=["2^40-1", "2^50"])
def test_lb_workers_and_stop_after_at_offset(start, end, f64):
    """Backends with two workers (the [k][backend] kernels, not the scan) and Sources with stop_after, at offsets."""
    path, _ = _lb(start, end, conc=2, stop_after=SPAN // 2)
    assert not path & N.LB_RUN_SCAN and not path & N.LB_RUN_LEAN, hex(path)
    assert bool(path & N.LB_RUN_F64_TIMES) == f64, hex(path)


def test_lb_shared_sink_without_slot_bits():
    """tb + sb > 64: the shared Sink's merge gathers created_at by slot instead of packing it beside the slot (never reached by the
    rest of the suite)."""
    path, _ = _lb(1 << 50, (1 << 50) + SPAN, S=64, B=16, rate=100.0)
    assert path & N.LB_RUN_SINK_GATHER and not path & N.LB_RUN_SINK_PACKED, hex(path)
    path, _ = _lb(1 << 40, (1 << 40) + SPAN, S=64, B=16, rate=100.0)
    assert path & N.LB_RUN_SINK_PACKED, hex(path)


def test_lb_sort_key_width_at_its_limit():
    """tb + bb = 64 runs; 65 is refused by name at construction."""
    start = 1 << 50
    path, _ = _lb(start, start + SPAN, S=4, B=8192, rate=10.0)     # tb 51 + bb 13
    assert path & N.LB_RUN_SCAN, hex(path)
    src = LbSourceArrays(n=1, src_rate=np.array([10.0]), n_clients=np.array([5000], np.int64))
    be = LbBackendArrays(n=8193, names=[f"srv{j}" for j in range(8193)])
    with pytest.raises(N.EngineError, match="64-bit sort key"):
        LoadBalancerEngine(src, be, virtual_nodes=1, horizon_ns=start + SPAN, start_ns=start)


@pytest.mark.parametrize("svc,mean", [("const", (1 << 52) / 1e9), ("const", 5e6), ("exp", 1.3e5)],
                         ids=["constant-2^52ns", "constant-5e6s", "exp-mean-1.3e5s"])
def test_lb_long_service_pending_departure(svc, mean):
    """One backend whose service reaches past 2^52 ns.  Its first request's departure D = S + service is pending at the end and is
    the backend's candidate for the event beyond end_time; hs_lbk_scan<true> converted it with i64_from_whole_d, exact below 2^52
    only, which turned D = S + 2^52 into about S / 2 -- an event BEFORE the end that won the election (a wrong final_time, no
    error).  The binary64 gate must include the longest service (36.8 exponential means, or the constant)."""
    path, r = _lb(0, SPAN, S=1, B=1, rate=2.0, mean=mean, svc=svc)
    assert path & N.LB_RUN_SCAN, hex(path)
    assert not path & N.LB_RUN_F64_TIMES, hex(path)
    assert r.final_time_ns > SPAN


# ---- single-heap graphs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [1 << 51, (1 << 53) + 1], ids=["2^51", "2^53+1"])
def test_general_graphs_through_simulation_at_offset(start):
    """Random general graphs (shared links, routers, LoadBalancers: the single-heap engine) through `Simulation(start_time=Instant(ns))`:
    lowering carries the start, and everything the graph checker compares equals the oracle run at the same offset."""
    import graph_specs as GS
    from happy_simulator_amd.graph_engine import GeneralGraph
    from random_specs import graph_spec
    from test_gpu_graph import _compare_with_oracle

    ran = 0
    for k in range(40):
        spec = graph_spec(k)
        if spec.get("end_s") is None:
            continue
        sim, ents = GS.build(spec, start_ns=start)
        if not isinstance(sim.lowered(), GeneralGraph):
            continue
        g_o, nodes = H.oracle_graph(spec)
        r = O.run(g_o, start + H.ns_from_seconds(spec["end_s"]), start_ns=start, seed=spec["seed"],
                  schedule=[(nd, start + t) for nd, t in H.oracle_graph_schedule(spec, nodes)])
        sim.run()
        _compare_with_oracle(spec, sim, ents, r, nodes)
        ran += 1
        if ran == 4:
            break
    assert ran >= 2


def test_chain_through_simulation_at_2_39():
    """`Simulation(start_time=Instant(2^39))` on the station engine: lowering carries the start."""
    start = 1 << 39
    sink = hs.Sink()
    server = hs.Server("srv", service_time=hs.ExponentialLatency(0.1), downstream=sink)
    source = hs.Source.poisson(rate=8, target=server)
    hs.Simulation(start_time=Instant(start), end_time=Instant(start + SPAN), sources=[source], entities=[server, sink], seed=42).run()
    r = O.run(O.mm1_chains(1, rate=8.0, mean=0.1), start + SPAN, start_ns=start, seed=42)
    assert [t.nanoseconds for t in sink.completion_times] == list(r.sinks[sorted(r.sinks)[0]][0])
    assert source.generated_count == r.generated[0]


# ---- refusals: never a launch on times that left int64, never a negative start -----------------------------------------------
def test_int64_reach_is_refused_at_construction():
    with pytest.raises(N.EngineError, match="leaves int64"):
        StationEngine(StationArrays.uniform(4, rate=1e-12), mode=N.MODE_SINGLE, horizon_ns=SPAN)
    with pytest.raises(N.EngineError, match="leaves int64"):
        StationEngine(StationArrays.uniform(4, mean=1e9), mode=N.MODE_SINGLE, horizon_ns=(1 << 62) + SPAN, start_ns=1 << 62)
    src = LbSourceArrays(n=1, src_rate=np.array([1e-12]), n_clients=np.array([5000], np.int64))
    be = LbBackendArrays(n=2, names=["a", "b"])
    with pytest.raises(N.EngineError, match="leaves int64"):
        LoadBalancerEngine(src, be, virtual_nodes=10, horizon_ns=SPAN)
    src = LbSourceArrays(n=1, src_rate=np.array([2.0]), n_clients=np.array([5000], np.int64))
    be = LbBackendArrays(n=2, names=["a", "b"], svc_kind=np.full(2, N.LAT_CONSTANT, np.uint8), svc_mean_s=np.array([0.1, 5e9]))
    with pytest.raises(N.EngineError, match="leaves int64"):
        LoadBalancerEngine(src, be, virtual_nodes=10, horizon_ns=(1 << 62) + SPAN, start_ns=1 << 62)
    spec = dict(RINGS["ring"], topology="ring", end_s=2.0)
    st, net, cap, _ = H.ring_arrays(spec)
    net.link_lat_min_s[:] = 1e10
    with pytest.raises(N.EngineError, match="leaves int64"):
        StationEngine(st, mode=N.MODE_SINGLE, horizon_ns=SPAN, log_capacity=cap, network=net)
    sink = hs.Sink()
    server = hs.Server("srv", service_time=hs.ExponentialLatency(0.1), downstream=sink)
    link = hs.NetworkLink("far", latency=hs.ConstantLatency(1e10), egress=server)
    source = hs.Source.poisson(rate=2, target=link)
    sim = hs.Simulation(duration=2.0, sources=[source], entities=[server, link, sink])
    assert type(sim.lowered()).__name__ == "GeneralGraph"       # (the single-heap engine: refused before its first launch)
    with pytest.raises(N.EngineError, match="leaves int64"):
        sim.run()


def test_negative_start_is_refused_by_name():
    with pytest.raises(N.EngineError, match="start_time"):
        StationEngine(StationArrays.uniform(4), mode=N.MODE_SINGLE, horizon_ns=SPAN, start_ns=-SPAN)
    src = LbSourceArrays(n=1, src_rate=np.array([2.0]), n_clients=np.array([5000], np.int64))
    with pytest.raises(N.EngineError, match="start_time"):
        LoadBalancerEngine(src, LbBackendArrays(n=2, names=["a", "b"]), virtual_nodes=10, horizon_ns=SPAN, start_ns=-SPAN)
    from happy_simulator_amd.graph_engine import GraphArrays, GraphEngine

    ga = GraphArrays(2)
    ga.kind[:] = (N.NODE_SOURCE, N.NODE_SINK)
    ga.target[0] = 1
    with pytest.raises(N.EngineError, match="start_time"):
        GraphEngine(ga, start_ns=-SPAN)
