"""GPU: PooledCycleResource and InventoryBuffer on the single-heap loop (csrc/hs_graph.hip, level kLvStock of graph_loop) against the
recorded live reference (tests/golden/live_stock/, written by tests/golden/make_golden_stock.py).  Every comparison is exact equality:
Sink records with their times, every per-entity statistic of every family's result reader, all by_kind slices (rows 60 .. 63: the four
Events of the two entities) and the event identity, every counter, `_available` / `_active` / `len(_queue)`, `_stock` and
`_order_pending`, the frozen stats with utilization and fill_rate.  No case is skipped or excluded
(test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import stock_specs as ST
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
SR = ST.STOCK
N_CASES = len(ST.FIXTURES) + ST.N_RANDOM + 2        # + the groups and the growth case


def _equals_the_recording(spec, sim, pools, ref):
    got = ST.results(spec, sim, pools)
    ST.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == ST.N_KINDS == 64 and "pc_state" in ref and "ib_state" in ref
    return got


def _run(spec, **kw):
    sim, pools = ST.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "PooledCycleResource or InventoryBuffer" in sim._station_refusal
    return sim, pools


def _one_heap(spec):
    import happy_simulator_amd.simulation as S

    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        return _run(spec)
    finally:
        S.MAX_PARTS = old


def _same(got, one, where):
    assert set(got) == set(one)
    for key in one:
        assert (got[key] == one[key]) if isinstance(one[key], list) else np.array_equal(np.asarray(got[key]), np.asarray(one[key])), (where, key)


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random chain of stock_specs, the two tests further down the groups
    and the growth case: every one of the N_CASES recorded cases has a recording and a test that compares it."""
    names = [s["name"] for s in ST.recorded_specs()]
    assert len(names) == len(set(names)) == N_CASES == 160 and ST.N_RANDOM == 100 and len(ST.FIXTURES) == 58
    with_events = []
    for spec in ST.recorded_specs():
        ref = SR.get("case", spec)
        assert ref["total_events"] <= 60_000
        if ref["by_kind"][ST.EV_ST_FIRST:].any():
            with_events.append(spec["name"])
    # (in one random chain no Request ever reaches the buffers: they wait in a BatchProcessor that never fills)
    assert sorted(set(names) - set(with_events)) == ["stock_graph_11"]
    for name in ST.TRACED:
        assert len(SR.get("case", ST.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(ST.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = ST.FIXTURES[name]
    if spec.get("windows"):
        sim, pools = ST.engine_run(spec, list(spec["windows"]) + [None])      # the reference ran it in these windows
    else:
        sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, SR.get("case", spec))


@pytest.mark.parametrize("k", range(ST.N_RANDOM))
def test_random_chain_equals_the_reference(k):
    spec = ST.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, SR.get("case", spec))


@pytest.mark.parametrize("name", ST.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink and Probe
    record in the one processing order of the whole graph, the engine's count of every kind equals the trace's, and the trace's rows
    of the four kinds name the nodes the product lowered the pools and buffers to."""
    spec = ST.FIXTURES[name]
    trace = SR.get("case", spec)["trace"]
    sim, pools, g, eng, end_ns, _start, _c = ST.engine(spec)
    a = g.arrays
    with eng:
        eng.run_until(end_ns)
        node, t, _v = eng.records()
        s = eng.summary()
        by_kind = list(s.events_by_kind)
        _crashed, internal, _k = eng.faults()
        events, flows = eng.stock_events(), eng.flow_events()
    count = lambda first, n: [int((trace[:, 1] == first + k).sum()) for k in range(n)]  # noqa: E731
    assert by_kind == count(0, N.EV_KINDS) and internal.tolist() == count(N.EV_KINDS, 4)
    assert flows[:N.FLOW_KINDS].tolist() == count(31, N.FLOW_KINDS)
    assert events.tolist() == count(ST.EV_ST_FIRST, N.STOCK_KINDS) and events.sum() > 0
    assert s.events_processed == sum(by_kind) + int(internal.sum()) + int(flows[:N.FLOW_KINDS].sum()) + int(events.sum()) == len(trace)
    assert set(trace[trace[:, 1] >= ST.EV_ST_FIRST][:, 2].tolist()) <= {g.node_of[id(x)] for x in pools["pool"] + pools["buffer"]}
    want = FC.live_rows(trace, kinds=(N.EV_NAMES.index("sink"), N.EV_NAMES.index("probe")))
    kept = (a.kind[node] == N.NODE_SINK) | (a.kind[node] == N.NODE_PROBE)
    assert np.array_equal(np.stack([t[kept], node[kept]], axis=1), want[:, [0, 2]])


# five uneven window ends each, some of them ON a cycle end / a replenish nanosecond of constant Sources' Requests
_WINDOWS = {"pool_accepts_queues_and_rejects_within_three_arrivals": [0.1, 0.6, 0.6, 1.1, 2.35],
            "resent_request_meets_arrivals_with_two_units": [0.2, 0.4, 0.4000001, 1.0, 1.6],
            "pool_with_a_cycle_time_of_zero": [0.1, 0.1, 0.75, 1.0, 1.9],
            "paused_pool_across_a_cycle_end": [0.4, 0.55, 0.7, 0.95, 2.0],
            "lead_time_zero_constant_sources": [0.1, 0.2, 0.95, 1.5, 2.5],
            "lead_time_a_third_from_1e5_s": [0.3, 0.333333334, 1.0, 1.7, 2.9],
            "pool_feeds_a_buffer_whose_stock_outs_return_to_a_second_pool": [0.33, 0.9, 1.4, 2.2, 2.95],
            "probes_on_all_four_metrics": [0.5, 1.0, 1.5, 1.9, 2.4]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    """Five uneven window ends, then the spec's own end: what one run leaves.  Behind every window the objects hold a consistent
    state of their own: a pool's units are free or active, the counters only grow, a buffer's stock is what came minus what went."""
    spec = ST.FIXTURES[name]
    assert len(_WINDOWS[name]) == 5
    seen = []

    def read(sim, pools, g, eng):
        st = ST.stock_state(pools)
        for p, row in zip(pools["pool"], st["pc_state"]):
            assert row[0] + row[1] == p.pool_size and row[0] >= 0 and row[1] >= 0 and (row[2] == 0 or p._queue_capacity == 0 or row[2] <= p._queue_capacity)
        for b, row, b0 in zip(pools["buffer"], st["ib_state"], spec["buffers"]):
            assert row[0] == b0["init"] + row[4] - row[3] >= 0 and row[4] % b0["q"] == 0 and row[2] - row[4] // b0["q"] in (0, 1)
        seen.append(st)

    sim, pools = ST.engine_run(spec, _WINDOWS[name] + [None], read=read)
    assert len(seen) == 6
    for key, cols in (("pc_state", (3, 4)), ("ib_state", (1, 2, 3, 4))):
        for col in cols:
            assert all((a[key][:, col] <= b[key][:, col]).all() for a, b in zip(seen, seen[1:]))
    assert any(seen[0][k].tobytes() != seen[-1][k].tobytes() for k in ("pc_state", "ib_state"))
    _equals_the_recording(spec, sim, pools, SR.get("case", spec))


_WINDOWED = sorted(n for n, s in ST.FIXTURES.items() if s.get("windows"))


@pytest.mark.parametrize("name", _WINDOWED)
def test_object_state_after_every_window(name):
    """The results are bound behind EVERY window of a windowed run: each pool's and buffer's state equals what the reference's objects
    held behind the same window."""
    spec = ST.FIXTURES[name]
    ref = SR.get("case", spec)
    ends = list(spec["windows"]) + [None]
    assert len(_WINDOWED) == 4 and ST.WINDOW_KEYS <= set(ref) and len(ref["window_pc_state"]) == len(ends) == 6
    seen = []
    sim, pools = ST.engine_run(spec, ends, read=lambda sim, pools, g, eng: seen.append(ST.stock_state(pools)))
    assert len(seen) == len(ends)
    for k, got in enumerate(seen):
        for key, have in got.items():
            assert np.array_equal(have, ref["window_" + key][k]), (name, k, key, have.tolist(), ref["window_" + key][k].tolist())
    _equals_the_recording(spec, sim, pools, ref)


@pytest.mark.parametrize("make", [ST.growth_spec, lambda: ST.FIXTURES["crashed_pool_restarts_with_a_line"],
                                  lambda: ST.FIXTURES["in_front_of_a_link_a_router_a_limiter_and_flows"]], ids=["line_of_400", "crashed_pool", "flows"])
def test_growth_from_capacity_one(make):
    """Heap, Request and record capacity 1: every buffer grows across relaunches; a line of some 400 Requests is longer than any
    Request pool the run began with, and every waiting Request keeps its place in the line."""
    spec = make()
    ref = SR.get("case", spec)
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = ST.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            launches = eng.summary().launches
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        assert launches > 3, launches
        got = _equals_the_recording(spec, sim, pools, ref)
        if spec["name"].startswith("line_of_400"):
            assert got["pc_state"][0, 2] > 300 and pools["pool"][0].queued == got["pc_state"][0, 2]


def test_64_replicas_equal_64_single_runs():
    names = ["resent_request_loses_the_unit_to_an_arrival_of_its_nanosecond", "crashed_pool_restarts_with_a_line", "buffer_pool_server_sink",
             "lead_time_a_third_from_1e5_s"]
    specs = [dict(ST.FIXTURES[names[i % 4]], end_s=2.0) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = ST.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=2900)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph) and "PooledCycleResource or InventoryBuffer" in sim._station_refusal
        got = ST.results(specs[i], sim, pools)
        one_sim, one_pools = _run(specs[i], seed=2900 + i)
        _same(got, ST.results(specs[i], one_sim, one_pools), i)
        seen.add((got["total_events"], tuple(got["sink_t_ns"][:50].tolist())))
    assert len(seen) > 32                                     # (the two constant-Source specs draw no random number: one result each)


def test_6_groups_as_parts_equal_one_heap_and_the_recording():
    """6 disconnected groups in ONE Simulation, one of 48 and one of 49 nodes: the parts run side by side (hs_graph_run_parts), a
    buffer's stockout_target in the part of its buffer, and leave what one heap over all of them leaves, which is what the reference's
    one heap left."""
    spec = ST.groups_spec()
    ref = SR.get("case", spec)
    sizes = sorted(ST.group_sizes(spec))
    assert len(sizes) == 6 and 48 in sizes and 49 in sizes               # csrc/hs_graph.hip kLdsNodesBatch = 48
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1 and sim._graph_parts == 6
    got = _equals_the_recording(spec, sim, pools, ref)
    _equals_the_recording(spec, one_sim, one_pools, ref)
    assert (got["pc_state"][:, 3] > 5).all() and (got["ib_state"][:, 2] > 1).all()


def test_a_batch_that_mixes_stock_and_other_graphs():
    """hs_graph_run_many over two graphs with the new entities, one of an older family and a plain one: the whole batch runs at the
    new level (hs_graph_level), and every handle leaves what it leaves alone."""
    import mixed_specs as MX

    mine = [ST.FIXTURES["buffer_pool_server_sink"], ST.FIXTURES["crash_over_a_replenish_leaves_the_order_pending"]]
    others = [MX.FIXTURES["client_server_batch_processor"]]

    def plain_run():
        # Source -> Server -> Sink on the single-heap loop (Simulation.run() would hand this one to the station engines)
        sink = hs.Sink("sink")
        srv = hs.Server("srv", service_time=hs.ExponentialLatency(0.03), downstream=sink)
        sim = hs.Simulation(sources=[hs.Source.poisson(rate=20.0, target=srv, name="src")], entities=[srv, sink], end_time=hs.Instant.from_seconds(3.0), seed=5)
        g = sim._lower_general()
        end_ns, start_ns, sched, cancelled = sim._general_prepare(g, False)
        return sim, None, g, sim._general_engine(g, start_ns, sched), end_ns, start_ns, cancelled

    runs = [ST.engine(s) for s in mine] + [MX.engine(s) for s in others] + [plain_run()]
    level = lambda r, which: r[3]._lib.hs_graph_level(r[3]._h, which)  # noqa: E731
    try:
        assert [level(r, 0) for r in runs] == [N.GRAPH_LEVEL_STOCK, N.GRAPH_LEVEL_STOCK, N.GRAPH_LEVEL_FLOW, N.GRAPH_LEVEL_PLAIN]
        assert N.GRAPH_LEVEL_STOCK == 11 and all(level(r, 1) == -1 for r in runs)
        GraphEngine.run_many([r[3] for r in runs], max(r[4] for r in runs))
        assert [level(r, 1) for r in runs] == [N.GRAPH_LEVEL_STOCK] * 4 and level(runs[3], 0) == N.GRAPH_LEVEL_PLAIN
        plain_got = (runs[3][3].summary().events_processed, [x.tolist() for x in runs[3][3].records()])
        for (sim, pools, g, eng, end_ns, _start, cancelled), spec in zip(runs[:3], mine + others):
            sim._general_finish(g, eng, max(r[4] for r in runs), cancelled, 0.0)
    finally:
        for r in runs:
            r[3].close()
    for (sim, pools, *_), spec in zip(runs[:2], mine):
        _equals_the_recording(spec, sim, pools, SR.get("case", spec))
    MX.compare(others[0]["name"], MX.results(others[0], runs[2][0], runs[2][1]), MX.MIXED.get("case", others[0]))
    alone = plain_run()
    with alone[3] as eng:
        eng.run_until(alone[4])
        assert eng._lib.hs_graph_level(eng._h, 1) == N.GRAPH_LEVEL_PLAIN
        assert plain_got == (eng.summary().events_processed, [x.tolist() for x in eng.records()]) and plain_got[0] > 100 and len(plain_got[1][0]) > 20


def test_object_state_after_a_run():
    """The public interface after Simulation.run(): frozen stats, the properties, the reference's private names."""
    spec = ST.FIXTURES["crashed_pool_restarts_with_a_line"]
    sim, pools = _run(spec)
    p = pools["pool"][0]
    assert isinstance(p.stats, hs.PooledCycleStats) and p.stats.pool_size == 1 and p.available + p.active == 1 and p.queued == len(p._queue) > 0
    assert p.completed == p._completed > 2 and p.utilization == p.active / 1 and p.stats.utilization == p.utilization
    with pytest.raises(Exception):
        p.stats.completed = 0
    spec = ST.FIXTURES["crash_over_a_replenish_leaves_the_order_pending"]
    sim, pools = _run(spec)
    b = pools["buffer"][0]
    assert isinstance(b.stats, hs.InventoryStats) and b._order_pending is True and b.stock == b._stock == 0 and b.stats.reorders == 1
    assert b.stats.fill_rate == b.stats.items_consumed / (b.stats.items_consumed + b.stats.stockouts) < 1.0
    assert sim._stock_by_kind.shape == (N.STOCK_KINDS,) and sim._stock_by_kind[2:].all() and not sim._stock_by_kind[:2].any()
    with pytest.raises(Exception):
        b.stats.stockouts = 0


def test_setters_and_getters_of_the_c_abi():
    """hs_graph_set_pool / hs_graph_set_inventory come before the first run and once per node; node = -1 returns the counts alone."""
    spec = ST.FIXTURES["buffer_pool_server_sink"]
    sim, pools, g, eng, end_ns, _start, _c = ST.engine(spec)
    pn, bn = g.node_of[id(pools["pool"][0])], g.node_of[id(pools["buffer"][0])]
    lib = eng._lib
    with eng:
        assert eng.stock(pn) == dict(available=2, active=0, queued=0, completed=0, rejected=0) and eng.stock_events().tolist() == [0] * 4
        assert eng.stock(bn) == dict(stock=5, stockouts=0, reorders=0, items_consumed=0, items_replenished=0, order_pending=0)
        assert lib.hs_graph_set_pool(eng._h, pn, 1, 1000, 0) == N.HS_E_STATE                  # configured already
        assert lib.hs_graph_set_pool(eng._h, bn, 1, 1000, 0) == N.HS_E_INVALID                # not a pool
        assert lib.hs_graph_set_inventory(eng._h, pn, 1, 1, 1, 0.5, -1) == N.HS_E_INVALID
        eng.run_until(end_ns)
        assert lib.hs_graph_set_inventory(eng._h, bn, 1, 1, 1, 0.5, -1) == N.HS_E_STATE
        events = eng.stock_events()
        s = eng.summary()
        assert events.all() and s.events_processed == sum(s.events_by_kind) + int(eng.faults()[1].sum()) + int(events.sum())
        w = eng.stock(pn)
        assert w["available"] + w["active"] == 2 and events[1] == w["completed"] and events[0] >= w["completed"] + w["active"] + w["queued"] + w["rejected"]
    import copy

    bare = copy.copy(g.arrays)
    bare.st_params = None                                                                     # a handle whose nodes are never configured
    with GraphEngine(bare, seed=1) as raw:
        with pytest.raises(N.EngineError, match="without its parameters"):
            raw.run_until(10 ** 9)
        assert lib.hs_graph_set_pool(raw._h, pn, N.POOL_MAX_UNITS + 1, 1000, 0) == N.HS_E_UNSUPPORTED
        assert lib.hs_graph_set_pool(raw._h, pn, 0, 1000, 0) == N.HS_E_INVALID and b"pool_size must be > 0, got 0" in lib.hs_graph_last_error(raw._h)
        assert lib.hs_graph_set_inventory(raw._h, bn, 1, 1, 0, 0.5, -1) == N.HS_E_INVALID and b"order_quantity must be > 0, got 0" in lib.hs_graph_last_error(raw._h)
        assert lib.hs_graph_set_inventory(raw._h, bn, 1, 1, 1, float("nan"), -1) == N.HS_E_UNSUPPORTED
        assert lib.hs_graph_set_inventory(raw._h, bn, N.INVENTORY_MAX + 1, 1, 1, 0.5, -1) == N.HS_E_UNSUPPORTED
        assert lib.hs_graph_set_inventory(raw._h, bn, 0, N.INVENTORY_MAX, N.INVENTORY_MAX, 0.5, -1) == N.HS_E_UNSUPPORTED
        assert b"reorder_point + order_quantity = 9223372036854775808 is beyond 2^63 - 2^48" in lib.hs_graph_last_error(raw._h)
        assert lib.hs_graph_set_inventory(raw._h, bn, N.INVENTORY_MAX, N.INVENTORY_MAX_LEVEL - N.INVENTORY_MAX, N.INVENTORY_MAX, 0.5, -1) == N.HS_OK
