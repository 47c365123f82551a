"""GPU: BatchProcessor, ConveyorBelt and GateController on the single-heap loop (csrc/hs_graph.hip kEvBpItem .. kEvGtClose: handlers
that construct N Events at once, a timeout its own entity cancels, 39 heap-entry kinds) against the recorded live reference
(tests/golden/live_flow/, written by tests/golden/make_golden_flow.py).  Every comparison is exact equality: Sink records, per-entity
statistics, the three entities' counters and what they still hold, event totals including the new kinds, events_cancelled, the final
`_crashed` flags.  No case is skipped or excluded (test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import client_specs as CS
import family_checks as FC
import flow_specs as FL
import graph_family as GF
import happy_simulator_amd as hs
import resilience_specs as XS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
FR = FL.FLOW
_FIRST = FL.EV_FLOW_FIRST


def _equals_the_recording(spec, sim, pools, ref):
    got = FL.results(spec, sim, pools)
    FL.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == 39 and not got["other_by_kind"].any()
    return got


def _run(spec, **kw):
    sim, pools = FL.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "BatchProcessor, ConveyorBelt or GateController" in sim._station_refusal
    return sim, pools


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of flow_specs, and every one has a recording."""
    names = [s["name"] for s in FL.all_specs()]
    assert len(names) == len(set(names)) == len(FL.FIXTURES) + FL.N_RANDOM and FL.N_RANDOM >= 100 and len(FL.FIXTURES) >= 30
    for spec in FL.all_specs():
        assert FR.get("case", spec)["total_events"] <= 40_000
    assert len(FL.TRACED) >= 6
    for name in FL.TRACED:
        assert len(FR.get("case", FL.FIXTURES[name])["trace"]) > 0
    used = np.zeros(len(FL.EV_FLOW), np.int64)
    for spec in FL.all_specs():
        used += FR.get("case", spec)["by_kind"][_FIRST:]
    assert (used > 50).all(), used                                           # every new kind, dozens of times


@pytest.mark.parametrize("name", sorted(FL.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = FL.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, FR.get("case", spec))


@pytest.mark.parametrize("k", range(FL.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = FL.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, FR.get("case", spec))


def test_what_the_issue_says_about_the_reference():
    sim, pools = _run(FL.FIXTURES["gate_conveyor_processor_chain"])
    g, c, b = pools["flow"]
    assert g.stats == hs.GateStats(25, 15, 20, 2, False) and g.queue_depth == 5 and g.is_open is False
    assert c.stats == hs.ConveyorStats(15, 0, 10) and c.items_in_transit == 0
    assert b.stats == hs.BatchProcessorStats(6, 15, 6) and b.buffer_depth == 0
    assert sim.summary.total_events_processed == 274 and pools["sink"][0].events_received == 15
    assert sim._flow_by_kind.tolist() == [15, 6, 6, 25, 15, 50, 2, 2]
    sim, pools = _run(FL.FIXTURES["batch_size_one_with_timeout"])            # batch_size = 1 releases on the second item, never on the first
    assert pools["flow"][0].stats == hs.BatchProcessorStats(2, 4, 0) and sim.summary.events_cancelled == 2
    assert sim.summary.total_events_processed == 23 and sim._flow_by_kind[1] == 0     # both timeouts were cancelled: popped, not processed
    sim, pools = _run(FL.FIXTURES["gate_paused_open_event_dropped"])         # the paused gate never saw its first `_GateOpen`
    assert pools["flow"][0].stats.open_cycles == 1 and sim._flow_by_kind[6] == 2


@pytest.mark.parametrize("name", FL.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event in
    the one processing order of the whole graph -- the Requests a flush lands on one nanosecond among them -- and the engine's count of
    every kind equals the trace's."""
    spec = FL.FIXTURES[name]
    ref = FR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = FL.engine(spec)
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        events = eng.flow_events()
    assert by_kind == [int((trace[:, 1] == k).sum()) for k in range(N.EV_KINDS)]
    assert internal.tolist() == [int((trace[:, 1] == N.EV_KINDS + k).sum()) for k in range(4)]
    assert events[:N.FLOW_KINDS].tolist() == [int((trace[:, 1] == _FIRST + k).sum()) for k in range(N.FLOW_KINDS)] and events[:N.FLOW_KINDS].sum() > 0
    assert events[N.FLOW_KINDS] == ref["events_cancelled"]
    want = FC.live_rows(trace)
    at_sink = g.arrays.kind[node] == N.NODE_SINK
    assert np.array_equal(np.stack([t[at_sink], node[at_sink]], axis=1), want[:, [0, 2]])


def test_windows_equal_one_run():
    for name in ("gate_conveyor_processor_chain", "gate_flushes_five_into_a_conveyor_at_capacity", "processor_paused_timeout_dropped",
                 "probes_on_the_three_metrics", "scheduled_requests_on_a_gate_events_nanosecond", "two_batches_in_process"):
        spec = FL.FIXTURES[name]
        ends = [0.25, 0.5, 0.5, 1.0, 1.2, 1.6, 2.0000001, spec["end_s"]]     # uneven windows, ends on gate and tie nanoseconds among them
        sim, pools, _ = FL.engine_run(spec, ends)
        _equals_the_recording(spec, sim, pools, FR.get("case", spec))
    spec = FL.FIXTURES["auto_terminating_run"]                               # ... and the auto-terminating run in two steps
    sim, pools, _ = FL.engine_run(spec, [0.45, None])
    _equals_the_recording(spec, sim, pools, FR.get("case", spec))


def test_a_flush_of_1100_grows_the_heap_in_front_of_one_event():
    """A closed gate with 1 100 queued Requests opens.  The handle starts with the smallest heap the engine makes (heap_capacity = 1:
    1 024 entries + 4 per node), which the queued Requests do not touch -- they sit in the gate's list, not in the heap.  The one
    `_GateOpen` needs 1 100 entries: the launch stops in front of it, the heap grows, and the flush happens whole; run side by side
    (hs_graph_run_many) the heap passes the 1 024 entries that mode keeps in LDS."""
    spec = FL.big_flush_spec()
    ref = FR.get("case", spec)
    sim, _pools = FL.build(spec)
    n = sim.lowered().arrays.n
    assert ref["flow_stats"][0, :2].tolist() == [1100, 1100] and 4 * n + 1024 < 1100 and 1100 > 1024     # the flush alone exceeds both
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = FL.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            launches = eng.summary().launches
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        assert launches >= 2 or side_by_side
        _equals_the_recording(spec, sim, pools, ref)
        node_t = pools["sink"][0].completion_times
        assert len(node_t) == 1100 and len({x.nanoseconds for x in node_t}) == 1                        # all on the nanosecond of the open


def test_batches_of_300_while_the_request_pool_grows():
    spec = FL.big_batch_spec()
    ref = FR.get("case", spec)
    sim, _pools = FL.build(spec)
    n = sim.lowered().arrays.n
    alive = int(ref["flow_stats"][0, 3] + ref["depth"].sum() + ref["active"].sum())
    assert ref["flow_stats"][0, 0] == 7 and alive > 4 * n + 1024                                        # more Requests alive than the smallest pool holds
    sim, pools, _ = FL.engine_run(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1)
    got = _equals_the_recording(spec, sim, pools, ref)
    roomy_sim, roomy_pools, _ = FL.engine_run(spec, [spec["end_s"]], heap_capacity=1 << 14, request_capacity=1 << 14, record_capacity=1 << 14)
    FC.same(got, FL.results(spec, roomy_sim, roomy_pools))


def test_64_replicas_equal_64_single_runs():
    base = FL.FIXTURES["partial_batches_on_timeout"]
    other = FL.FIXTURES["probes_on_the_three_metrics"]
    specs = [dict(base if i % 2 == 0 else other, end_s=2.5) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = FL.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=900)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph) and sim._graph.arrays.has_flows
        got = FL.results(specs[i], sim, pools)
        one_sim, one_pools = _run(specs[i], seed=900 + i)
        FC.same(got, FL.results(specs[i], one_sim, one_pools), i)
        seen.add((got["total_events"], tuple(got["flow_stats"].ravel().tolist())))
    assert len(seen) > 48


def test_32_groups_as_parts_equal_one_heap():
    """32 disconnected Source -> GateController -> ConveyorBelt -> BatchProcessor -> Server -> Sink groups in ONE Simulation: the parts
    run side by side (hs_graph_run_parts) and leave what one heap over all of them leaves."""
    import happy_simulator_amd.simulation as S

    spec = FL.groups_spec(32)
    sim, pools = _run(spec)
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1 and sim._graph_parts == 32
    got = FL.results(spec, sim, pools)
    FC.same(got, FL.results(spec, one_sim, one_pools))
    stats = got["flow_stats"].reshape(32, 3, 6)
    assert (stats[:, 0, 3] == 2).all() and (stats[:, 1, 0] > 0).all() and (stats[:, 2, 0] > 0).all() and got["events_cancelled"] > 0
    # ... and without a timeout nothing is ever cancelled: the groups do run as parts
    for fl in spec["flows"]:
        if fl["kind"] == "batch":
            fl["ts"] = 0.0
    sim, pools = _run(spec)
    assert sim._graph_parts == 32
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    FC.same(FL.results(spec, sim, pools), FL.results(spec, one_sim, one_pools))


def _union_spec():
    """Two flow groups, the Client group of a recorded Client fixture and the TimeoutWrapper group of a recorded wrapper fixture as
    the disconnected components of ONE spec (their Servers, links, Sinks, Sources and faults renumbered)."""
    spec = FL.groups_spec(2, name="flow_union")
    for fl in spec["flows"]:
        if fl["kind"] == "batch":
            fl["ts"] = 0.0                    # (no timeout: no cancelled Event can stand in front of the end, the parts stay parts)
    spec.update(links=[], clients=[], wrappers=[], faults=[])
    for m in (CS.FIXTURES["fixed_retry_crash_with_restart"], XS.FIXTURES["timeout_link_jitter"]):
        off = dict(server=len(spec["servers"]), link=len(spec["links"]), client=len(spec["clients"]), wrapper=len(spec["wrappers"]), sink=spec["n_sinks"])
        assert not (m["routers"] or m["limiters"] or m["lbs"] or m.get("probes") or m.get("schedule") or m.get("auto") or m.get("start_ns"))

        def at(r, off=off):
            if r is None:
                return None
            return r + off["server"] if isinstance(r, int) else [r[0], r[1] + off[r[0]]]

        spec["servers"] += [dict(sv, out=at(sv["out"])) for sv in m["servers"]]
        spec["links"] += [dict(lk, to=at(lk["to"])) for lk in m["links"]]
        spec["clients"] += [dict(c, to=at(c["to"])) for c in m.get("clients") or []]
        spec["wrappers"] += [dict(w, to=at(w["to"])) for w in m.get("wrappers") or []]
        spec["faults"] += [dict(ft, on=at(ft["on"])) for ft in m.get("faults") or []]
        spec["sources"] += [dict(sc, to=at(sc["to"])) for sc in m["sources"]]
        spec["n_sinks"] += m["n_sinks"]
    return spec


def test_a_union_with_a_client_member_and_a_wrapper_member_as_parts_equals_one_heap():
    """Two flow groups next to the graph of a recorded Client fixture and that of a recorded TimeoutWrapper fixture, in ONE
    Simulation: four parts side by side -- a flow part, a Client part and a wrapper part in one launch of the sixth instantiation --
    leave what one heap over all of them leaves."""
    import happy_simulator_amd.simulation as S

    spec = _union_spec()

    def everything(sim, pools):
        out = FL.results(spec, sim, pools)
        out.update(XS.wrapper_results(pools))
        out.update(CS.client_results(pools))
        out["client_by_kind"], out["resilience_by_kind"] = np.asarray(sim._client_by_kind), np.asarray(sim._resilience_by_kind)
        return out

    sim, pools = _run(spec)
    assert sim._graph_parts == 4
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    got = everything(sim, pools)
    FC.same(got, everything(one_sim, one_pools))
    assert got["cl_stats"][0, 2] > 0 and got["wrap_stats"][0, 0] > 0 and (got["flow_stats"][:, 0] > 0).all()
    assert got["client_by_kind"].sum() > 0 and got["resilience_by_kind"].sum() > 0 and np.delete(got["flow_by_kind"], 1).all()


def test_a_flow_free_handle_in_a_batch_with_flow_handles():
    """hs_graph_run_many: a plain graph, a wrapper graph and a Client graph share the launch (the sixth instantiation of the loop) with
    flow graphs and report what they report alone."""
    import rate_limiter_specs as RS

    plain_spec, wrapped, client = RS.FIXTURES["token_constant"], XS.FIXTURES["timeout_link_jitter"], CS.FIXTURES["lossy_link"]
    with_flows = [FL.FIXTURES["gate_conveyor_processor_chain"], FL.FIXTURES["partial_batches_on_timeout"]]
    built = []

    def build_fn():
        k = len(built)
        sim, pools = FL.build(with_flows[k]) if k < 2 else GF.build((wrapped, client, plain_spec)[k - 2])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 5, base_seed=60)
    assert len(results) == 5
    for i in range(2):
        one_sim, one_pools = _run(with_flows[i], seed=60 + i)
        FC.same(FL.results(with_flows[i], *built[i]), FL.results(with_flows[i], one_sim, one_pools), i)
    for i, (spec, family) in enumerate(((wrapped, "resilience"), (client, "client"), (plain_spec, "rate_limiter")), start=2):
        one_sim, one_pools = GF.build(spec, seed=60 + i)
        one_sim.run()
        FC.same(GF.results(spec, *built[i], family), GF.results(spec, one_sim, one_pools, family), family)
        assert not built[i][0]._graph.arrays.has_flows


def test_a_node_that_was_never_configured_is_a_state_error():
    sim, _pools = FL.build(FL.FIXTURES["conveyor_unlimited"])
    g = sim.lowered()
    g.arrays.flow_params = None                                                # (the handle is created without the set_flow call)
    with GraphEngine(g.arrays, seed=1) as eng:
        with pytest.raises(N.EngineError, match="without its parameters") as e:
            eng.run_until(10 ** 9)
        assert e.value.code == N.HS_E_STATE


def test_the_engine_refuses_what_the_host_refuses():
    """hs_graph_create / hs_graph_set_flow / hs_graph_schedule_gate on hand-made arrays."""
    sim, pools = FL.build(FL.FIXTURES["gate_conveyor_processor_chain"])
    a = sim.lowered().arrays
    gate, conv, proc = (int(np.nonzero(a.kind == k)[0][0]) for k in (N.NODE_GATE, N.NODE_CONVEYOR, N.NODE_BATCH_PROCESSOR))
    with GraphEngine(a, seed=1) as eng:
        with pytest.raises(N.EngineError, match="configured already") as e:
            eng._check(eng._lib.hs_graph_set_flow(eng._h, gate, 0, 0, 0, 1))
        assert e.value.code == N.HS_E_STATE
        with pytest.raises(N.EngineError, match="is not a GateController"):
            eng.schedule(conv, 0, None, True)
        eng.schedule(gate, 0, None, False)
    keep = a.flow_params.copy()
    for node, row, text, code in ((proc, [0, 0, 0, 0], "batch_size must be > 0, got 0", N.HS_E_INVALID),
                                  (proc, [4, -1, 0, 0], "process_time must be >= 0", N.HS_E_INVALID),
                                  (proc, [(1 << 20) + 1, 0, 0, 0], "is beyond the 1048576 items of one batch", N.HS_E_UNSUPPORTED),
                                  (conv, [0, -5, 0, 0], "transit_time must be >= 0", N.HS_E_INVALID),
                                  (gate, [(1 << 20) + 1, 0, 0, 0], "is beyond 1048576 items", N.HS_E_UNSUPPORTED)):
        a.flow_params[node] = row
        with pytest.raises(N.EngineError, match=text) as e:
            GraphEngine(a, seed=1)
        assert e.value.code == code
        a.flow_params[:] = keep
    end = a.target.copy()
    a.kind[int(np.nonzero(a.kind == N.NODE_SERVER)[0][0])] = N.NODE_TIMEOUT_WRAPPER     # a wrapper in front of ... -> Sink is fine; in front of the gate it is not
    a.target[int(np.nonzero(a.kind == N.NODE_TIMEOUT_WRAPPER)[0][0])] = gate
    with pytest.raises(N.EngineError, match="a completion hook on an item they hold is not lowered") as e:
        GraphEngine(a, seed=1)
    assert e.value.code == N.HS_E_UNSUPPORTED
    a.target[:] = end
