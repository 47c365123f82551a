"""GPU: Hedge and Fallback on the single-heap loop (csrc/hs_graph.hip, the hedge instantiation of graph_loop) against the recorded
live reference (tests/golden/live_hedge/, written by tests/golden/make_golden_hedge.py).  Every comparison is exact equality: Sink
records with their times, every per-entity statistic of every family's result reader, all by_kind slices (rows 53 .. 59: the
wrappers' seven Events) and the event identity, every HedgeStats / FallbackStats field, `_next_request_id` and every `_in_flight`
entry -- id, start_time, completed / hedges_sent / responses_received or the state -- in the reference's dict order.  No case is
skipped or excluded (test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import hedge_specs as HG
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
HR = HG.HEDGE


def _equals_the_recording(spec, sim, pools, ref):
    got = HG.results(spec, sim, pools)
    HG.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == HG.N_KINDS and "hg_stats" in ref and "hg_in_flight" in ref and "fb_stats" in ref and "fb_in_flight" in ref
    return got


def _run(spec, **kw):
    sim, pools = HG.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "Hedge or Fallback" in sim._station_refusal
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
    """The parametrised tests below run every fixture and every random chain of hedge_specs, and every one has a recording."""
    names = [s["name"] for s in HG.all_specs()]
    assert len(names) == len(set(names)) == len(HG.FIXTURES) + HG.N_RANDOM and HG.N_RANDOM >= 150 and len(HG.FIXTURES) >= 50
    for spec in HG.recorded_specs():
        ref = HR.get("case", spec)
        assert ref["total_events"] <= 60_000 and ref["by_kind"][HG.EV_HG_FIRST:].any()
    for name in HG.TRACED:
        assert len(HR.get("case", HG.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(HG.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = HG.FIXTURES[name]
    if spec.get("windows"):
        sim, pools = HG.engine_run(spec, list(spec["windows"]) + [None])      # the reference ran it in these windows
    else:
        sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, HR.get("case", spec))


@pytest.mark.parametrize("k", range(HG.N_RANDOM))
def test_random_chain_equals_the_reference(k):
    spec = HG.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, HR.get("case", spec))


@pytest.mark.parametrize("name", HG.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink, Probe and
    limiter record in the one processing order of the whole graph, and the engine's count of every kind equals the trace's."""
    spec = HG.FIXTURES[name]
    trace = HR.get("case", spec)["trace"]
    sim, pools, g, eng, end_ns, _start, _c = HG.engine(spec)
    a = g.arrays
    with eng:
        eng.run_until(end_ns)
        node, t, _v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        events, flows = eng.hedge_events(), eng.flow_events()
    count = lambda first, n: [int((trace[:, 1] == first + k).sum()) for k in range(n)]  # noqa: E731
    assert by_kind == count(0, N.EV_KINDS) and internal.tolist() == count(N.EV_KINDS, 4)
    assert flows[:N.FLOW_KINDS].tolist() == count(31, N.FLOW_KINDS)
    assert events.tolist() == count(HG.EV_HG_FIRST, N.HEDGE_KINDS) and events.sum() > 0
    # the wrappers' rows of the trace name the nodes the product lowered them to
    assert set(trace[trace[:, 1] >= HG.EV_HG_FIRST][:, 2].tolist()) <= {g.node_of[id(x)] for x in pools["hedge"] + pools["fallback"]}
    want = FC.live_rows(trace, kinds=(N.EV_NAMES.index("sink"), N.EV_NAMES.index("probe")))
    kept = (a.kind[node] == N.NODE_SINK) | (a.kind[node] == N.NODE_PROBE)
    assert np.array_equal(np.stack([t[kept], node[kept]], axis=1), want[:, [0, 2]])


# five uneven window ends each, some of them ON a send-hedge / timeout nanosecond of a constant Source's Requests
_WINDOWS = {"hedge_constant_source_delay_at_the_link_latency": [0.3, 0.425, 1.0, 1.0, 2.175],
            "hedge_delay_half_the_link_latency_three_hedges": [0.15, 0.275, 0.9, 1.6000001, 2.9],
            "crashed_hedge_restarts": [0.5, 1.0, 1.07, 1.8, 2.5],
            "hedge_behind_a_batch_processor": [0.21, 0.8, 1.3, 1.35, 2.7],
            "fallback_constant_source_timeout_at_the_primary_latency": [0.175, 0.3, 1.0, 1.8, 2.55],
            "fallback_entity_is_a_link_in_front_of_a_server": [0.4, 0.41, 1.2, 2.0, 2.9],
            "inject_latency_on_the_primary_link": [0.6, 1.0, 1.5, 2.0, 2.4],
            "hedge_behind_a_fallback_server": [0.33, 0.9, 1.4, 2.2, 2.95]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    """Five uneven window ends, then the spec's own end: what one run leaves.  Behind every window the objects hold a consistent
    state of their own: every request either left or is in flight, ids ascend, no entry is younger than the clock."""
    spec = HG.FIXTURES[name]
    assert len(_WINDOWS[name]) == 5
    seen = []

    def read(sim, pools, g, eng):
        st = HG.hedge_state(pools)
        for rows, ent, off in (("hg_stats", "hg_in_flight", "hg_in_flight_off"), ("fb_stats", "fb_in_flight", "fb_in_flight_off")):
            for i, row in enumerate(st[rows]):
                mine = st[ent][st[off][i]:st[off][i + 1]]
                total, next_id, live = int(row[0]), int(row[5 if rows == "hg_stats" else 6]), int(row[6 if rows == "hg_stats" else 7])
                assert total == next_id and live == len(mine) and (np.diff(mine[:, 0]) > 0).all() and (mine[:, 0] <= next_id).all()
                assert (mine[:, 1] <= sim._current_time.nanoseconds).all()
                if rows == "fb_stats":
                    assert int(row[1]) + int(row[4]) + live == total                    # left by the primary, left by the fallback entity, in flight
                else:
                    assert int(row[1]) + int(row[2]) + int((mine[:, 2] == 0).sum()) == total      # every request won once, or waits
        seen.append(st)

    sim, pools = HG.engine_run(spec, _WINDOWS[name] + [None], read=read)
    assert len(seen) == 6 and [int(s["hg_stats"][:, 0].sum() + s["fb_stats"][:, 0].sum()) for s in seen] == sorted(
        int(s["hg_stats"][:, 0].sum() + s["fb_stats"][:, 0].sum()) for s in seen) and any(seen[0][k].tobytes() != seen[-1][k].tobytes() for k in ("hg_stats", "fb_stats"))
    _equals_the_recording(spec, sim, pools, HR.get("case", spec))


_WINDOWED = sorted(n for n, s in HG.FIXTURES.items() if s.get("windows"))


@pytest.mark.parametrize("name", _WINDOWED)
def test_object_state_after_every_window(name):
    """The results are bound behind EVERY window of a windowed run: each wrapper's counters and `_in_flight` entries equal what the
    reference's objects held behind the same window."""
    spec = HG.FIXTURES[name]
    ref = HR.get("case", spec)
    ends = list(spec["windows"]) + [None]
    assert len(_WINDOWED) >= 4 and HG.WINDOW_KEYS <= set(ref) and len(ref["window_hg_stats"]) == len(ends) == 6
    seen = []
    sim, pools = HG.engine_run(spec, ends, read=lambda sim, pools, g, eng: seen.append(HG.hedge_state(pools)))
    assert len(seen) == len(ends)
    for k, got in enumerate(seen):
        for key, have in got.items():
            assert np.array_equal(have, ref["window_" + key][k]), (name, k, key, have.tolist(), ref["window_" + key][k].tolist())
    _equals_the_recording(spec, sim, pools, ref)


@pytest.mark.parametrize("name", ["hedge_3_delay_below_the_link_latency", "crashed_hedge_target_restarts", "hedge_behind_a_batch_processor",
                                  "late_primary_response_after_the_timeout", "crashed_fallback_entity", "two_hedges_in_one_graph"])
def test_growth_from_capacity_one(name):
    """In-flight tables of one place, heap, Request and record capacity 1: every buffer grows across relaunches -- a Request at a wrapper
    waits in front of the pop until its table has room, a send-hedge or a timeout until the pool has a Request for the duplicate."""
    spec = HG.FIXTURES[name]
    ref = HR.get("case", spec)
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = HG.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1, table_capacity=1)
        with eng:
            first = [eng.hedge(g.node_of[id(x)])["table_capacity"] for x in pools["hedge"] + pools["fallback"]]
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            last = [eng.hedge(g.node_of[id(x)])["table_capacity"] for x in pools["hedge"] + pools["fallback"]]
            launches = eng.summary().launches
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        assert set(first) == {1} and max(last) >= 4 and launches > 3, (first, last, launches)
        _equals_the_recording(spec, sim, pools, ref)


def test_a_table_of_leaked_entries_grows_and_is_read_back():
    """400 entries leak behind a crashed target, from a table of one place: nine doublings, every entry read back by id."""
    spec = HG.leak_spec()
    ref = HR.get("case", spec)
    sim, pools, g, eng, end_ns, _start, cancelled = HG.engine(spec, table_capacity=1)
    with eng:
        eng.run_until(end_ns)
        w = eng.hedge(g.node_of[id(pools["hedge"][0])])
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    assert w["in_flight_count"] == 400 and w["table_capacity"] == 1024 and w["entries"][:, 0].tolist() == list(range(1, 401))
    assert (w["entries"][:, 3] == 2).sum() >= 390 and not w["entries"][:, 2].any()
    _equals_the_recording(spec, sim, pools, ref)
    assert pools["hedge"][0].in_flight_count == 400 and list(pools["hedge"][0]._in_flight) == list(range(1, 401))


def test_64_replicas_equal_64_single_runs():
    names = ["hedge_2_delay_at_the_link_latency", "crashed_hedge_target_restarts", "late_primary_response_after_the_timeout",
             "hedge_behind_a_fallback_server"]
    specs = [dict(HG.FIXTURES[names[i % 4]], end_s=2.0) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = HG.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=2300)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph)
        got = HG.results(specs[i], sim, pools)
        one_sim, one_pools = _run(specs[i], seed=2300 + i)
        _same(got, HG.results(specs[i], one_sim, one_pools), i)
        seen.add((got["total_events"], tuple(got["sink_t_ns"][:50].tolist())))
    assert len(seen) > 48


def test_16_groups_as_parts_equal_one_heap_and_the_recording():
    """16 disconnected groups in ONE Simulation, one of 48 and one of 49 nodes: the parts run side by side (hs_graph_run_parts), a
    Fallback's fallback entity in the part of its wrapper, and leave what one heap over all of them leaves, which is what the
    reference's one heap left."""
    spec = HG.groups_spec()
    ref = HR.get("case", spec)
    sizes = sorted(HG.group_sizes(spec))
    assert len(sizes) == 16 and 48 in sizes and 49 in sizes              # csrc/hs_graph.hip kLdsNodesBatch = 48
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1 and sim._graph_parts == 16
    got = _equals_the_recording(spec, sim, pools, ref)
    _equals_the_recording(spec, one_sim, one_pools, ref)
    assert (got["hg_stats"][:, 0] > 10).all() and (got["fb_stats"][:, 3] > 3).all()


def test_a_batch_that_mixes_hedged_and_other_graphs():
    """hs_graph_run_many over two graphs with the new wrappers and two of older families: the whole batch runs the hedge instantiation,
    and every handle leaves what it leaves alone."""
    import mixed_specs as MX

    mine = [HG.FIXTURES["hedge_over_a_jittered_lossy_link"], HG.FIXTURES["crashed_primary"]]
    others = [MX.FIXTURES["client_server_batch_processor"], MX.FIXTURES["gate_flush_into_a_timeout_wrapper"]]
    runs = [HG.engine(s) for s in mine] + [MX.engine(s) for s in others]
    try:
        GraphEngine.run_many([r[3] for r in runs], max(r[4] for r in runs))
        for (sim, pools, g, eng, end_ns, _start, cancelled), spec in zip(runs, mine + others):
            sim._general_finish(g, eng, max(r[4] for r in runs), cancelled, 0.0)
    finally:
        for r in runs:
            r[3].close()
    for (sim, pools, *_), spec in zip(runs[:2], mine):
        _equals_the_recording(spec, sim, pools, HR.get("case", spec))
    for (sim, pools, *_), spec in zip(runs[2:], others):
        MX.compare(spec["name"], MX.results(spec, sim, pools), MX.MIXED.get("case", spec))


def test_object_state_after_a_run():
    """The public interface after Simulation.run(): frozen stats, the properties, `_in_flight` in the reference's form."""
    spec = HG.FIXTURES["crashed_hedge_target_restarts"]
    sim, pools = _run(spec)
    h = pools["hedge"][0]
    assert isinstance(h.stats, hs.HedgeStats) and h.stats.total_requests == h._next_request_id > 20 and h.in_flight_count == len(h._in_flight) > 3
    rid, entry = next(iter(h._in_flight.items()))
    assert set(entry) == {"start_time", "completed", "hedges_sent", "responses_received"} and isinstance(entry["start_time"], hs.Instant)
    assert entry["completed"] is False and entry["hedges_sent"] == 3 and rid >= 1
    with pytest.raises(Exception):
        h.stats.total_requests = 0
    spec = HG.FIXTURES["crashed_fallback_entity"]
    sim, pools = _run(spec)
    f = pools["fallback"][0]
    assert isinstance(f.stats, hs.FallbackStats) and f.stats.fallback_failures == 0 and f.stats.fallback_invocations == f.stats.primary_failures > 5
    assert {e["state"] for e in f._in_flight.values()} <= {"primary", "fallback"} and "fallback" in {e["state"] for e in f._in_flight.values()}
    assert sim._hedge_by_kind.shape == (N.HEDGE_KINDS,) and sim._hedge_by_kind[3:].all() and not sim._hedge_by_kind[:3].any()


def test_setters_and_getters_of_the_c_abi():
    """hs_graph_set_hedge / hs_graph_set_fallback come before the first run and once per node; node = -1 returns the counts alone."""
    spec = HG.FIXTURES["hedge_behind_a_fallback_server"]
    sim, pools, g, eng, end_ns, _start, _c = HG.engine(spec)
    hn, fn = g.node_of[id(pools["hedge"][0])], g.node_of[id(pools["fallback"][0])]
    lib = eng._lib
    with eng:
        assert eng.hedge(hn)["table_capacity"] == 256 == eng.hedge(fn)["table_capacity"] and eng.hedge_events().tolist() == [0] * 7
        assert lib.hs_graph_set_hedge(eng._h, hn, 1000, 1, 0) == N.HS_E_STATE                 # configured already
        assert lib.hs_graph_set_hedge(eng._h, fn, 1000, 1, 0) == N.HS_E_INVALID               # not a Hedge
        assert lib.hs_graph_set_fallback(eng._h, hn, 0, 1000, 0) == N.HS_E_INVALID
        eng.run_until(end_ns)
        assert lib.hs_graph_set_fallback(eng._h, fn, 0, 1000, 0) == N.HS_E_STATE
        events = eng.hedge_events()
        s = eng.summary()
        assert events.all() and s.events_processed == sum(s.events_by_kind) + int(eng.faults()[1].sum()) + int(events.sum())
        w = eng.hedge(fn)
        assert w["total_requests"] == w["next_request_id"] == w["primary_successes"] + w["fallback_successes"] + w["in_flight_count"]
    import copy

    bare = copy.copy(g.arrays)
    bare.hg_params = None                                                                     # a handle whose wrappers are never configured
    with GraphEngine(bare, seed=1) as raw:
        with pytest.raises(N.EngineError, match="without its parameters"):
            raw.run_until(10 ** 9)
        assert lib.hs_graph_set_hedge(raw._h, hn, 1000, N.HEDGE_MAX_HEDGES + 1, 0) == N.HS_E_UNSUPPORTED
        assert lib.hs_graph_set_hedge(raw._h, hn, 1000, 0, 0) == N.HS_E_INVALID and b"max_hedges must be >= 1, got 0" in lib.hs_graph_last_error(raw._h)
