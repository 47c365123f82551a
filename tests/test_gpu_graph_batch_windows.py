"""GPU: the side-by-side instantiation of the single-heap loop (csrc/hs_graph.hip hs_graph_run_batch = graph_loop<1024, 48>, behind
hs_graph_run_many and hs_graph_run_parts) at and beyond ITS LDS windows: heaps that stay below 1 024 entries, cross that edge while
running and lie far beyond it; graphs of 48 / 49 nodes (node rows in LDS / in HBM) with Probes, RoundRobin state and the wavefront's
least-loaded selection.  The lone kernel's windows (4 096 / 192) are test_gpu_graph.py's and test_gpu_rate_limiter.py's; the limiter
policies around 48 nodes are test_gpu_rate_limiter.py::test_named_fixture_equals_the_reference[nodes_beyond_lds].

Every comparison is exact equality.  Every test asserts FIRST that its case crosses the window it is named for -- the oracle's
heap_peak, the nodes per heap, `_graph_parts`, `coop_selects` -- with 1 024 and 48 as literals (test_graph_host.py pins them on
the source)."""
import numpy as np
import pytest

import family_checks as FC
import graph_specs as GS
import happy_simulator_amd as hs
import helpers as H
import strategy_specs as SS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine, split_parts
from oracle import hs_oracle as O
from test_gpu_graph import _compare_with_oracle

pytestmark = pytest.mark.gpu

W_HEAP, W_NODES = 1024, 48                     # kLdsHeapBatch, kLdsNodesBatch


# ---- the shapes: N Sources -> one Server -> one Sink -------------------------------------------------------------------------
def _fan_in(name, sources, c, mean, end_s):
    return dict(name=name, topology="graph", n_sinks=1, links=[], routers=[], servers=[dict(mean=mean, c=c, cap=None, out=["sink", 0])],
                sources=[dict(s, to=0) for s in sources], end_s=end_s, seed=0)


def _far_sources(poisson_only=False, base=2.0, mod=7):
    return [dict(kind="poisson" if (poisson_only or k % 3) else "constant", rate=base + (k % mod)) for k in range(2500)]


SHAPES = {
    # name: (spec, the band of the oracle's heap_peak, the first of eight seeds)
    "below": (_fan_in("below", [dict(kind="poisson", rate=5.0)] * 900, 400, 0.02, 1.0), (900, W_HEAP - 1), 98),
    "hover": (_fan_in("hover", [dict(kind="poisson", rate=5.0)] * 960, 400, 0.02, 1.0), (W_HEAP + 1, 1200), 1),
    "far": (_fan_in("far", _far_sources(), 2000, 0.4, 0.5), (2 * W_HEAP + 1, 1 << 40), 99),
    # 16 Sources of 2 500 Requests / s on 6 000 workers: the heap outgrows the capacity its handle starts with (4 n + 1 024 = 1 096)
    # more than four times over, each time but the first with its tail already in HBM
    "burst": (_fan_in("burst", [dict(kind="poisson", rate=2500.0)] * 16, 6000, 2.0, 0.15), (4 * (4 * 18 + 1024) + 1, 1 << 40), 5),
}
_cache = {}


def _case(name):
    """(spec, lowered arrays, oracle graph, oracle nodes, the product's node ids in the oracle's terms), built once per shape."""
    if name not in _cache:
        spec = SHAPES[name][0]
        sim, _ents = GS.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph)
        g_o, nodes = H.oracle_graph(spec)
        _cache[name] = (spec, g.arrays, g_o, nodes, _product_nodes(spec))
    return _cache[name]


def _oracle(name, seed, end_s=None):
    key = (name, seed, end_s)
    if key not in _cache:
        spec, _a, g_o, nodes, _p = _case(name)
        _cache[key] = O.run(g_o, H.ns_from_seconds(spec["end_s"] if end_s is None else end_s), seed=seed,
                            schedule=H.oracle_graph_schedule(spec, nodes))
    return _cache[key]


def _in_band(name, r):
    lo, hi = SHAPES[name][1]
    return lo <= r.heap_peak <= hi


def _product_nodes(spec):
    """graph_specs.build's node numbering (Sources, then `servers + lbs + routers + links + sinks`) under helpers.oracle_graph's keys."""
    out, at = {}, 0
    for key, cnt in (("source", len(spec["sources"])), ("server", len(spec["servers"])), ("lb", len(spec.get("lbs") or [])),
                     ("router", len(spec["routers"])), ("link", len(spec["links"])), ("sink", spec["n_sinks"])):
        out[key] = list(range(at, at + cnt))
        at += cnt
    out["n"] = at
    return out


def _want_stats(spec, r, nodes, P):
    """What GraphEngine.stats() must hold, array for array, from the oracle's Result (Sources, Servers, RoundRobin LoadBalancers, Sinks)."""
    n = P["n"]
    want = {k: np.zeros((n, 6) if k == "lb" else n, np.float64 if k == "total_service_s" else np.int64) for k in N.GRAPH_STATS if k != "rt_taken"}
    want["generated"][P["source"]] = want["payloads"][P["source"]] = r.generated[nodes["source"]]      # (no stop_after: one payload per tick)
    for k, arr in (("accepted", r.accepted), ("dropped", r.dropped), ("completed", r.completed), ("rejected", r.rejected),
                   ("total_service_s", r.total_service_s), ("queue_depth", r.depth), ("active", r.active)):
        want[k][P["server"]] = arr[nodes["server"]]
    want["received"][P["sink"]] = [len(r.sinks[nd][0]) for nd in nodes["sink"]]
    taken = []
    for j, nd in enumerate(nodes["lb"]):
        st = r.lbs[nd]["stats"]                                    # received, forwarded, failed, no_backend_available, in flight
        want["lb"][P["lb"][j]] = [st[0], st[1], st[2], st[3], st[4], r.lbs[nd]["strategy_index"]]
        taken.extend(r.lbs[nd]["total_requests"])
    want["rt_taken"] = np.asarray(taken, np.int64)
    return want


def _assert_engine_equals_oracle(eng, spec, r, nodes, P, what):
    s = eng.summary()
    assert (s.events_processed, s.final_time_ns) == (r.events_processed, r.final_time_ns), what
    np.testing.assert_array_equal(list(s.events_by_kind), r.events_by_kind, err_msg=what)
    got, want = eng.stats(), _want_stats(spec, r, nodes, P)
    assert set(got) == set(want) | {"limiters"} and not got["limiters"]
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    node, t, cr = eng.records()                                     # in processing order; per Sink that is the oracle's order
    assert np.isin(node, P["sink"]).all() and len(node) == sum(len(r.sinks[nd][0]) for nd in nodes["sink"])
    for j, nd in enumerate(nodes["sink"]):
        mine = node == P["sink"][j]
        np.testing.assert_array_equal(t[mine], r.sinks[nd][0], err_msg=f"{what}: sink {j}")
        np.testing.assert_array_equal(cr[mine], r.sinks[nd][1], err_msg=f"{what}: sink {j} created_at")


def _assert_engines_equal(a, b, what):
    sa, sb = a.summary(), b.summary()
    assert (sa.events_processed, sa.final_time_ns, list(sa.events_by_kind)) == (sb.events_processed, sb.final_time_ns, list(sb.events_by_kind)), what
    sta, stb = a.stats(), b.stats()
    for k in sta:
        np.testing.assert_array_equal(sta[k], stb[k], err_msg=f"{what}: {k}")
    for x, y in zip(a.records(), b.records()):
        np.testing.assert_array_equal(x, y, err_msg=what)


def _close(engines):
    for e in engines:
        e.close()


# ---- 1. heaps around 1 024 entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["below", "hover", "far"])
def test_eight_replicas_around_the_heap_window_equal_the_oracle(name):
    """hs_graph_run_many on eight handles, seeds base + i: `below` never leaves the 1 024 LDS entries, `hover` starts at 960 and
    crosses the edge while running (sifts split at i < 1024), `far` keeps most of its heap in HBM."""
    spec, arrays, _g_o, nodes, P = _case(name)
    base = SHAPES[name][2]
    runs = [_oracle(name, base + i) for i in range(8)]
    assert all(_in_band(name, r) for r in runs), [r.heap_peak for r in runs]
    engines = [GraphEngine(arrays, seed=base + i) for i in range(8)]
    try:
        GraphEngine.run_many(engines, H.ns_from_seconds(spec["end_s"]))
        for i, (e, r) in enumerate(zip(engines, runs)):
            _assert_engine_equals_oracle(e, spec, r, nodes, P, f"{name} replica {i}")
    finally:
        _close(engines)
    assert len({r.events_processed for r in runs}) > 4                       # (the seeds differ)


def test_replicas_that_cross_the_heap_window_through_the_runner():
    """The `hover` shape through ParallelRunner.run_replicas: replica i == the oracle with seed base + i, every statistic and record."""
    spec, _arrays, g_o, nodes, _P = _case("hover")
    base = SHAPES["hover"][2]
    runs = [_oracle("hover", base + i) for i in range(8)]
    assert all(_in_band("hover", r) for r in runs), [r.heap_peak for r in runs]
    built = []

    def build_fn():
        sim, ents = GS.build(spec)
        built.append((sim, ents))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 8, base_seed=base)
    assert len(results) == len(built) == 8 and isinstance(built[0][0].lowered(), GeneralGraph)
    for i, ((sim, ents), res, r) in enumerate(zip(built, results, runs)):
        assert res.name == f"replica_{i}" and res.summary.total_events_processed == r.events_processed
        _compare_with_oracle(spec, sim, ents, r, nodes)


def test_one_batch_of_heaps_on_every_side_of_the_window():
    """ONE hs_graph_run_many call over two `below`, two `hover` and two `far` handles (one end for all: 0.5 s), with record logs that
    start at 16 entries: each heap is relaunched whenever its log is full, so they finish in different launches, the longer ones
    copied into and out of the window many times -- each == its own oracle run."""
    end_s = 0.5
    members = [(name, SHAPES[name][2] + i) for name in ("below", "hover", "far") for i in range(2)]
    runs = [_oracle(name, seed, end_s) for name, seed in members]
    assert all(_in_band(name, r) for (name, _seed), r in zip(members, runs)), [r.heap_peak for r in runs]
    engines = [GraphEngine(_case(name)[1], seed=seed, record_capacity=16) for name, seed in members]
    try:
        GraphEngine.run_many(engines, H.ns_from_seconds(end_s))
        assert len({e.summary().launches for e in engines}) > 1              # (they did not all finish together)
        for (name, seed), e, r in zip(members, engines, runs):
            spec, _a, _g, nodes, P = _case(name)
            _assert_engine_equals_oracle(e, spec, r, nodes, P, f"{name} seed {seed}")
    finally:
        _close(engines)


@pytest.mark.parametrize("name, first_s", [("hover", 0.3), ("far", 0.2), ("burst", 0.05)])
def test_batch_heaps_grow_and_continue_with_their_tail_in_hbm(name, first_s):
    """Handles created with the smallest capacities, run side by side to two ends.  Every launch that fills the record log ends with a
    heap longer than the 1 024-entry window and the next one begins with it: the head is copied back and in again, the tail stays.
    `burst` also outgrows its heap buffer (hs_graph_create gives at least 4 n + 1 024 entries) three times, so grow() moves a heap
    whose tail is in HBM.  Each handle == the same graph run alone (the lone kernel) on a default handle to the same two ends, and
    == the oracle at the final end."""
    spec, arrays, _g_o, nodes, P = _case(name)
    base = SHAPES[name][2]
    ends = [H.ns_from_seconds(first_s), H.ns_from_seconds(spec["end_s"])]
    seeds = [base, base + 1]
    for seed in seeds:
        assert _in_band(name, _oracle(name, seed)), _oracle(name, seed).heap_peak
        assert _oracle(name, seed, first_s).pending > W_HEAP                 # the heap is beyond the window where the first run stops
    alone = [GraphEngine(arrays, seed=seed) for seed in seeds]
    small = [GraphEngine(arrays, seed=seed, heap_capacity=1, request_capacity=1, record_capacity=16) for seed in seeds]
    try:
        for w, end in enumerate(ends):
            for e in alone:
                e.run_until(end)
            GraphEngine.run_many(small, end)
            assert all(e.summary().launches > 1 for e in small)                # (relaunched: the heap came back into the window)
            for seed, a, b in zip(seeds, alone, small):
                _assert_engines_equal(b, a, f"{name} seed {seed} end {w}")
        for seed, e in zip(seeds, small):
            _assert_engine_equals_oracle(e, spec, _oracle(name, seed), nodes, P, f"{name} seed {seed}")
    finally:
        _close(alone + small)


# ---- 2. heaps around 48 nodes ------------------------------------------------------------------------------------------------------
def _chains_spec(n_chains, probes=()):
    """n chains of five Poisson Sources -> Server(c = 40, Exp 0.3) -> Sink (7 nodes each; outside the station shape)."""
    return dict(name=f"chains_{n_chains}", topology="graph", n_sinks=n_chains, links=[], routers=[], end_s=2.0, seed=11,
                servers=[dict(mean=0.3, c=40, cap=None, out=["sink", i]) for i in range(n_chains)],
                sources=[dict(kind="poisson", rate=1.0 + (k % 5), to=k // 5) for k in range(5 * n_chains)],
                probes=[[["server", i], "depth", 0.25] for i in probes])


@pytest.mark.parametrize("n_chains, probes, per_heap", [(12, (), 42), (14, (), 49), (14, (0, 7), 50)], ids=["42", "49", "50_probed"])
def test_parts_of_42_49_and_50_nodes_equal_the_oracles_one_heap(n_chains, probes, per_heap):
    """One Simulation of 12 / 14 chains on TWO heaps: 42 nodes per heap keep their rows in LDS, 49 leave them in HBM; with one Probe
    per heap (50 nodes) the samples read HBM rows too.  == the oracle's one heap: totals, the one event beyond the end, every
    Source's, Server's and Sink's arrays, every sample."""
    import happy_simulator_amd.simulation as S

    spec = _chains_spec(n_chains, probes)
    g_o, nodes = H.oracle_graph(spec)
    r = O.run(g_o, H.ns_from_seconds(spec["end_s"]), seed=spec["seed"])
    sim, ents = GS.build(spec)
    assert isinstance(sim.lowered(), GeneralGraph)
    heaps = split_parts(sim.lowered().arrays, 2)
    assert [b.n for _ids, _pos, b in heaps] == [per_heap, per_heap] and (per_heap > W_NODES) == (n_chains == 14)
    assert [int((b.kind == N.NODE_PROBE).sum()) for _ids, _pos, b in heaps] == [len(probes) // 2] * 2
    old, S.MAX_PARTS = S.MAX_PARTS, 2
    try:
        sim.run()
    finally:
        S.MAX_PARTS = old
    assert sim._graph_parts == 2
    _compare_with_oracle(spec, sim, ents, r, nodes)
    for (pr, data), nd in zip(ents["probes"], nodes["probe"]):
        t, v = r.sinks[nd]
        assert len(t) >= 7
        np.testing.assert_array_equal(data._t_ns, t, err_msg=pr.name)
        np.testing.assert_array_equal(data._v, v, err_msg=pr.name)


def _lb_spec(strategy, n_sources, seed=3):
    """S Poisson Sources -> LoadBalancer -> 40 Servers (c from {1, 2, 3}, Exp 0.5) -> one Sink: S + 42 nodes, ~600 Requests in 2 s."""
    rng = np.random.default_rng(40)
    return SS._lb_case(f"{strategy}_{n_sources}_sources", strategy, 40, SS._poisson(n_sources, 300.0 / n_sources), mean=0.5, end_s=2.0,
                       seed=seed, c=[int(c) for c in rng.choice([1, 2, 3], size=40)])


@pytest.mark.parametrize("n_sources", [6, 7])
def test_least_connections_replicas_of_48_and_49_nodes_equal_single_runs(n_sources):
    """64 replicas side by side; 40 backends >= the cooperative threshold, so all 64 lanes read the backends' `active` -- from LDS rows
    at 48 nodes, from HBM rows at 49.  Replica i == the same Simulation run alone with seed base + i (the lone kernel keeps all these
    nodes in LDS: an independent instantiation)."""
    spec = _lb_spec("least_conn", n_sources)
    assert N.GRAPH_COOP_MIN_BACKENDS <= 40
    built = []

    def build_fn():
        sim, ents = SS.build(spec)
        built.append((sim, ents))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=700)
    g = built[0][0].lowered()
    assert len(results) == len(built) == 64 and isinstance(g, GeneralGraph)
    assert g.arrays.n == n_sources + 42 and (g.arrays.n > W_NODES) == (n_sources == 7)
    totals = set()
    for i, ((sim, ents), res) in enumerate(zip(built, results)):
        alone, ents1 = SS.build(spec, seed=700 + i)
        alone.run()
        assert res.summary.total_events_processed == alone.summary.total_events_processed
        sim._summary = res.summary
        FC.same(SS.results(spec, sim, ents), SS.results(spec, alone, ents1), f"replica {i}")
        totals.add(res.summary.total_events_processed)
        assert ents["lbs"][0].stats.requests_forwarded > 300
    assert len(totals) > 16


@pytest.mark.parametrize("n_sources", [6, 7])
def test_forced_cooperative_selection_in_a_batch_of_48_and_49_nodes(n_sources):
    """The same at the C ABI with GRAPH_DEBUG_COOPERATIVE on every handle of the batch: coop_selects() > 0 on each, and each == the
    same graph run alone on a default handle."""
    spec = _lb_spec("least_conn", n_sources)
    sim, _ents = SS.build(spec)
    g = SS.lower_single_heap(sim, spec)
    assert g.arrays.n == n_sources + 42 and (g.arrays.n > W_NODES) == (n_sources == 7)
    end_ns = H.ns_from_seconds(spec["end_s"])
    engines = [GraphEngine(g.arrays, seed=900 + i) for i in range(64)]
    try:
        for e in engines:
            e.set_debug_flags(N.GRAPH_DEBUG_COOPERATIVE)
        GraphEngine.run_many(engines, end_ns)
        for i, e in enumerate(engines):
            forwarded = int(e.stats()["lb"][:, 1].sum())
            assert e.coop_selects() == forwarded > 300, i
            with GraphEngine(g.arrays, seed=900 + i) as alone:
                alone.run_until(end_ns)
                _assert_engines_equal(e, alone, f"replica {i}")
    finally:
        _close(engines)


@pytest.mark.parametrize("n_sources", [6, 7])
def test_round_robin_replicas_of_48_and_49_nodes_equal_the_oracle(n_sources):
    """RoundRobin._index and the per-backend counts live in the LoadBalancer's row and in rt_taken: 64 replicas of 48 / 49 nodes side
    by side (hs_graph_run_many; through `hs.Simulation` this shape is the pipeline's), replica i == the oracle with seed base + i."""
    spec = _lb_spec("round_robin", n_sources)
    g_o, nodes = H.oracle_graph(spec)
    P = _product_nodes(spec)
    sim, _ents = SS.build(spec)
    g = SS.lower_single_heap(sim, spec)
    assert g.arrays.n == P["n"] == n_sources + 42 and (g.arrays.n > W_NODES) == (n_sources == 7)
    end_ns = H.ns_from_seconds(spec["end_s"])
    engines = [GraphEngine(g.arrays, seed=300 + i) for i in range(64)]
    try:
        GraphEngine.run_many(engines, end_ns)
        totals = set()
        for i, e in enumerate(engines):
            r = O.run(g_o, end_ns, seed=300 + i)
            assert r.lbs[nodes["lb"][0]]["stats"][1] > 300                  # (Requests forwarded)
            _assert_engine_equals_oracle(e, spec, r, nodes, P, f"replica {i}")
            totals.add(r.events_processed)
        assert len(totals) > 16
    finally:
        _close(engines)


# ---- 3. both windows at once, as parts -----------------------------------------------------------------------------------------
def test_two_parts_beyond_both_windows_equal_the_oracles_one_heap():
    """ONE Simulation of two disconnected `far`-shaped components (Poisson Sources only: no pre-run tick can share a nanosecond with a
    run-time event) on two heaps of 2 502 nodes and more than 2 048 pending events each == the oracle's one heap, including the one
    event beyond the end, elected from each part's heap[0] after the head is copied back."""
    halves = [_far_sources(poisson_only=True), _far_sources(poisson_only=True, base=3.0, mod=5)]
    for h, (srcs, mean) in enumerate(zip(halves, (0.4, 0.5))):                # each component alone: its heap is beyond the window
        one = _fan_in(f"far_part_{h}", srcs, 2000, mean, 0.5)
        g_1, _n = H.oracle_graph(one)
        assert O.run(g_1, H.ns_from_seconds(0.5), seed=17).heap_peak > 2 * W_HEAP
    spec = dict(name="two_far_parts", topology="graph", n_sinks=2, links=[], routers=[], end_s=0.5, seed=17,
                servers=[dict(mean=0.4, c=2000, cap=None, out=["sink", 0]), dict(mean=0.5, c=2000, cap=None, out=["sink", 1])],
                sources=[dict(s, to=h) for h, srcs in enumerate(halves) for s in srcs])
    g_o, nodes = H.oracle_graph(spec)
    r = O.run(g_o, H.ns_from_seconds(spec["end_s"]), seed=spec["seed"])
    sim, ents = GS.build(spec)
    heaps = split_parts(sim.lowered().arrays)
    assert [b.n for _ids, _pos, b in heaps] == [2502, 2502]
    sim.run()
    assert sim._graph_parts == 2
    assert r.final_time_ns > H.ns_from_seconds(spec["end_s"])                 # (the event beyond the end was elected and processed)
    _compare_with_oracle(spec, sim, ents, r, nodes)
