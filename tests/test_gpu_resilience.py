"""GPU: Bulkhead and TimeoutWrapper on the single-heap loop (csrc/hs_graph.hip kEvBhReq .. kEvTwTimeout and the completion hook at
every place a handler returns) against the recorded live reference (tests/golden/live_resilience/, written by
tests/golden/make_golden_resilience.py).  Every comparison is exact equality: Sink records, per-entity statistics, both wrappers'
counters, wait-queue ids and in-flight ids, event totals including the new kinds, the final `_crashed` flags.  No case is skipped or
excluded (test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import fault_specs as FS
import family_checks as FC
import graph_family as GF
import resilience_specs as XS
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine
from recorded import RESILIENCE as XR

pytestmark = pytest.mark.gpu

# what the engine has no counterpart for (the reference heap's length, the recorder's time-travel count) or what is compared in a form
# of its own (by_kind: the engine reports the public fifteen kinds, the internal ones per graph; trace: test_record_order_follows_the_trace)
_NOT_COMPARED = {"trace", "by_kind", "pending_events", "time_travel"}
_FIRST_HC, _FIRST_WRAPPER = N.EV_KINDS + 4, N.EV_KINDS + 7
_BY_KIND_SLICES = [("by_kind", N.EV_KINDS), ("internal_by_kind", _FIRST_HC), ("health_by_kind", _FIRST_WRAPPER), ("resilience_by_kind", _FIRST_WRAPPER + 6)]


def _equals_the_recording(spec, sim, pools, ref):
    got = GF.results(spec, sim, pools, "resilience")
    FC.compare(spec["name"], got, ref, _NOT_COMPARED, _BY_KIND_SLICES)
    return got


def _run(spec, **kw):
    sim, pools = GF.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "Bulkhead or TimeoutWrapper" in sim._station_refusal
    return sim, pools


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of resilience_specs, and every one has a recording."""
    names = [s["name"] for s in XS.all_specs()]
    assert len(names) == len(set(names)) == len(XS.FIXTURES) + XS.N_RANDOM and XS.N_RANDOM >= 120 and len(XS.FIXTURES) >= 40
    for spec in XS.all_specs():
        XR.get("case", spec)
    assert len(XS.TRACED) == 6
    for name in XS.TRACED:
        assert len(XR.get("case", XS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(XS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = XS.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, XR.get("case", spec))


@pytest.mark.parametrize("k", range(XS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = XS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, XR.get("case", spec))


def test_what_the_issue_says_about_the_reference():
    sim, pools = _run(XS.FIXTURES["bulkhead_link_twenty_requests"])       # 20 Requests through Bulkhead -> NetworkLink -> Server
    assert sim._resilience_by_kind[:2].tolist() == [20, 38] and pools["wrapper"][0].stats.total_requests == 20
    sim, pools = _run(XS.FIXTURES["paused_server_leaks_permits"])         # one permit lost per Request dropped at the paused Server
    b = pools["wrapper"][0]
    assert (b.active_count, b.queue_depth, b.available_permits) == (4, 3, 0) and b.stats.rejected_requests > 200
    assert sorted(b._in_flight) == sorted(set(b._in_flight)) and len(b._in_flight) == 4 and len(b._wait_queue) == 3
    sim, pools = _run(XS.FIXTURES["bulkhead_server_burst"])
    assert pools["wrapper"][0].stats.peak_concurrent == 2 and pools["wrapper"][0].active_count == 0
    sim, pools = _run(XS.FIXTURES["timeout_wrapper_crash_without_restart"])
    t = pools["wrapper"][0]
    assert t.in_flight_count > 0 and t._crashed is True and t._next_request_id == t.stats.total_requests


@pytest.mark.parametrize("name", XS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event that
    was not dropped by a crash, in the one processing order of the whole graph; and the engine's count of every kind equals the
    trace's."""
    spec = XS.FIXTURES[name]
    trace = XR.get("case", spec)["trace"]
    sim, _pools, g, eng, end_ns, _start, _c = FC.engine(spec)
    with eng:
        eng.run_until(end_ns)
        node, t, _v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        events = eng.wrapper_events()
    assert by_kind == [int((trace[:, 1] == k).sum()) for k in range(N.EV_KINDS)]
    assert internal.tolist() == [int((trace[:, 1] == N.EV_KINDS + k).sum()) for k in range(4)]
    assert events.tolist() == [int((trace[:, 1] == _FIRST_WRAPPER + k).sum()) for k in range(6)] and events.sum() > 0
    want = FC.live_rows(trace)
    at_sink = g.arrays.kind[node] == N.NODE_SINK
    assert len(want) > 0 and np.array_equal(np.stack([t[at_sink], node[at_sink]], axis=1), want[:, [0, 2]])


def _run_to_ends_with_tables(spec, ends_s, **caps):
    """FC.engine_run and every TimeoutWrapper's table capacity at the end."""
    def tables(eng, g):
        return [eng.wrapper(int(i))["table_capacity"] for i in np.nonzero(g.arrays.kind == N.NODE_TIMEOUT_WRAPPER)[0]]

    return FC.engine_run(spec, ends_s, read=tables, **caps)


def test_windows_equal_one_run():
    for name in ("bulkhead_crash_with_restart", "timeout_response_after_the_wrappers_restart", "probes_on_the_four_metrics",
                 "link_delay_equals_max_wait_time"):
        spec = XS.FIXTURES[name]
        ends = [0.25, 0.5, 0.5, 1.2, 1.9, 3.0000001, spec["end_s"]]          # 7 uneven windows, ends on tie and fault nanoseconds among them
        sim, pools, _ = _run_to_ends_with_tables(spec, ends)
        _equals_the_recording(spec, sim, pools, XR.get("case", spec))


def test_in_flight_table_grown_from_one_place_equals_the_reference():
    """A TimeoutWrapper's table that starts with ONE place: the launch stops in front of every Request that would not fit, the host
    doubles the table (the ids in flight move with it) and the run goes on -- with leaked ids, a crash and late responses on the way."""
    for name in ("timeout_response_after_the_wrappers_restart", "timeout_wrapper_crash_without_restart", "probes_on_the_four_metrics"):
        spec = XS.FIXTURES[name]
        sim, pools, tables = _run_to_ends_with_tables(spec, [spec["end_s"]], table_capacity=1)
        assert tables and min(tables) >= 4, tables                          # (grown from one place)
        got = _equals_the_recording(spec, sim, pools, XR.get("case", spec))
        roomy_sim, roomy_pools, roomy_tables = _run_to_ends_with_tables(spec, [spec["end_s"]], table_capacity=4096)
        assert roomy_tables == [4096] * len(tables)
        FC.same(got, GF.results(spec, roomy_sim, roomy_pools, "resilience"), name)


def test_growth_from_capacities_of_one_equals_a_run_with_room():
    """Heap, Request pool, record log and in-flight table start at their smallest under a backlog: hundreds of Requests wait in a
    Bulkhead's queue (threaded through the Request pool) and at a slow Server while the pool is moved several times."""
    spec = XS._g("growth_under_a_backlog", [XS.bh(["link", 0], 3, 400, 2.0), XS.tw(["link", 1], 0.4)], servers=[XS.srv(0.2, cap=None)],
                 links=[XS.link(0, 0.3, "exp", 0.2), XS.link(0, 0.1, "exp", 0.3)], sources=[XS.src(["wrapper", 0], 100.0), XS.src(["wrapper", 1], 100.0)],
                 faults=[XS.pause(["link", 0], 1.0, 1.3)], end_s=4.0, seed=5)
    grown_sim, grown_pools, tables = _run_to_ends_with_tables(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1, table_capacity=1)
    roomy_sim, roomy_pools, _ = _run_to_ends_with_tables(spec, [spec["end_s"]], heap_capacity=1 << 16, request_capacity=1 << 16, record_capacity=1 << 16,
                                                             table_capacity=1 << 12)
    grown, roomy = GF.results(spec, grown_sim, grown_pools, "resilience"), GF.results(spec, roomy_sim, roomy_pools, "resilience")
    assert roomy["wrap_stats"][0, 6] > 100 and roomy["wrap_stats"][1, 2] > 10 and roomy["depth"].sum() > 100 and tables[0] >= 32
    FC.same(grown, roomy)


def test_64_replicas_equal_64_single_runs():
    base = XS.FIXTURES["bulkhead_crash_with_restart"]
    other = XS.FIXTURES["timeout_response_after_the_wrappers_restart"]
    specs = [dict(base if i % 2 == 0 else other, end_s=2.5) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = GF.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=700)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph) and sim._graph.arrays.has_wrappers
        got = GF.results(specs[i], sim, pools, "resilience")
        one_sim, one_pools = _run(specs[i], seed=700 + i)
        FC.same(got, GF.results(specs[i], one_sim, one_pools, "resilience"), i)
        seen.add((got["total_events"], tuple(got["wrap_stats"].ravel().tolist())))
    assert len(seen) > 48


def test_32_groups_as_parts_equal_one_heap():
    """32 disconnected Source -> wrapper -> NetworkLink -> Server -> Sink groups, one Server paused per group, in ONE Simulation: the
    parts run side by side (hs_graph_run_parts) and leave what one heap over all of them leaves."""
    import happy_simulator_amd.simulation as S

    spec = XS.groups_spec(32)
    sim, pools = _run(spec)
    assert sim._graph_parts == 32
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    got = GF.results(spec, sim, pools, "resilience")
    FC.same(got, GF.results(spec, one_sim, one_pools, "resilience"))
    assert (got["wrap_stats"][0::2, 7] > 0).all() and (got["wrap_stats"][1::2, 2] > 0).all()      # permits leaked, requests timed out


def test_a_wrapper_free_handle_in_a_batch_with_a_wrapper_handle():
    """hs_graph_run_many: a graph without faults and without wrappers shares the launch (the fourth instantiation of the loop) with
    wrapper graphs and reports what it reports alone."""
    import rate_limiter_specs as RS

    plain_spec = RS.FIXTURES["token_constant"]
    wrapped = [XS.FIXTURES["bulkhead_link_jitter_out_of_order"], XS.FIXTURES["timeout_link_jitter"]]
    built = []

    def build_fn():
        k = len(built)
        sim, pools = GF.build(wrapped[k]) if k < 2 else GF.build(plain_spec)
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 3, base_seed=40)
    assert len(results) == 3
    for i in range(2):
        one_sim, one_pools = _run(wrapped[i], seed=40 + i)
        FC.same(GF.results(wrapped[i], *built[i], "resilience"), GF.results(wrapped[i], one_sim, one_pools, "resilience"), i)
    sim, pools = built[2]
    assert not sim._graph.arrays.has_wrappers and not sim._faults
    one_sim, one_pools = GF.build(plain_spec, seed=42)
    one_sim.run()
    FC.same(GF.results(plain_spec, sim, pools, "rate_limiter"), GF.results(plain_spec, one_sim, one_pools, "rate_limiter"), "plain")
    assert sim.summary.total_events_processed == one_sim.summary.total_events_processed


def test_a_wrapper_node_that_was_never_configured_is_a_state_error():
    sim, _pools = GF.build(XS.FIXTURES["bulkhead_link_constant"])
    g = sim.lowered()
    g.arrays.wrap_params = None                                                # (the handle is created without the wrapper call)
    with GraphEngine(g.arrays, seed=1) as eng:
        with pytest.raises(N.EngineError, match="without its parameters") as e:
            eng.run_until(10 ** 9)
        assert e.value.code == N.HS_E_STATE


def test_wrapper_parameters_after_the_first_run_are_a_state_error():
    sim, _pools, g, eng, end_ns, _s, _c = FC.engine(XS.FIXTURES["bulkhead_link_constant"])
    node = int(np.nonzero(g.arrays.kind == N.NODE_BULKHEAD)[0][0])
    with eng:
        with pytest.raises(N.EngineError) as e:                                # a wrapper is configured once
            eng._check(eng._lib.hs_graph_set_wrapper(eng._h, node, 2, 0, -1.0, 0.0, 0))
        assert e.value.code == N.HS_E_STATE
        eng.run_until(end_ns)
        with pytest.raises(N.EngineError) as e:
            eng._check(eng._lib.hs_graph_set_wrapper(eng._h, node, 2, 0, -1.0, 0.0, 0))
        assert e.value.code == N.HS_E_STATE


def test_the_engine_refuses_what_the_host_refuses():
    """hs_graph_create / hs_graph_set_wrapper on hand-made arrays: a wrapper in front of a wrapper through a link, max_concurrent one
    above the bound, the reference's own ValueErrors."""
    sim, _pools = GF.build(XS.FIXTURES["bulkhead_two_links"])
    g = sim.lowered()
    a = g.arrays
    node = int(np.nonzero(a.kind == N.NODE_BULKHEAD)[0][0])
    a.wrap_params[node, 0] = N.BULKHEAD_MAX_CONCURRENT + 1
    with pytest.raises(N.EngineError, match="max_concurrent = 65537 is beyond") as e:
        GraphEngine(a, seed=1)
    assert e.value.code == N.HS_E_UNSUPPORTED
    a.wrap_params[node, 0] = 0
    with pytest.raises(N.EngineError, match="max_concurrent must be >= 1, got 0"):
        GraphEngine(a, seed=1)
    a.wrap_params[node, 0] = N.BULKHEAD_MAX_CONCURRENT                        # at the bound: taken
    GraphEngine(a, seed=1).close()
    last_link = int(np.nonzero(a.kind == N.NODE_LINK)[0][-1])
    end = a.target.copy()
    a.target[[i for i in np.nonzero(a.kind == N.NODE_LINK)[0] if a.kind[a.target[i]] != N.NODE_LINK][0]] = node     # ... -> link -> the Bulkhead itself
    with pytest.raises(N.EngineError, match="two completion hooks on one Event") as e:
        GraphEngine(a, seed=1)
    assert e.value.code == N.HS_E_UNSUPPORTED and last_link >= 0
    a.target[:] = end
