"""GPU: HealthChecker and the LoadBalancer's health marks on the single-heap loop (csrc/hs_graph.hip kEvHcCycle / kEvHcResp /
kEvHcTimeout, lb_mark and the selection over the healthy list) against the recorded live reference (tests/golden/live_health/,
written by tests/golden/make_golden_health.py).  Every comparison is exact equality: Sink records, per-entity statistics, the
LoadBalancers' per-backend counts, health flags and mark counts, the checkers' statistics and per-backend states, event totals
including the health and fault counts, the final `_crashed` flags.  No case is skipped or excluded
(test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import family_checks as FC
import graph_family as GF
import health_specs as HS
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine
from recorded import HEALTH as HR

pytestmark = pytest.mark.gpu

# what the engine has no counterpart for (the reference heap's length, the recorder's time-travel count) or what is compared in a form
# of its own (by_kind: the engine reports the public fifteen kinds, the internal ones per graph; trace: test_record_order_follows_the_trace)
_NOT_COMPARED = {"trace", "by_kind", "pending_events", "time_travel", "health_events", "probe_drops"}
_FIRST_HC = N.EV_KINDS + 4
_BY_KIND_SLICES = [("by_kind", N.EV_KINDS), ("internal_by_kind", _FIRST_HC), ("health_by_kind", _FIRST_HC + 3)]


def _equals_the_recording(spec, sim, pools, ref):
    got = GF.results(spec, sim, pools, "health")
    FC.compare(spec["name"], got, ref, _NOT_COMPARED, _BY_KIND_SLICES)
    return got


def _run(spec, **kw):
    sim, pools = GF.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and ("health" in sim._station_refusal or "fault" in sim._station_refusal)
    return sim, pools


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of health_specs, and every one has a recording."""
    names = [s["name"] for s in HS.all_specs()]
    assert len(names) == len(set(names)) == len(HS.FIXTURES) + HS.N_RANDOM and HS.N_RANDOM >= 120
    for spec in HS.all_specs():
        HR.get("case", spec)
    assert len(HS.TRACED) == 6 and len(HS.WIDE) == 9
    for name in HS.TRACED:
        assert len(HR.get("case", HS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(HS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = HS.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, HR.get("case", spec))


@pytest.mark.parametrize("k", range(HS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = HS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, HR.get("case", spec))


def test_what_the_issue_says_about_the_reference():
    """3 Servers behind a RoundRobin LoadBalancer, interval 1.0, timeout 0.25, CrashNode("s1", 3.3, restart_at=9.7), 20 s."""
    sim, pools = _run(HS.FIXTURES["crash_then_restart_of_one_backend"])
    hc, lb = pools["checker"][0], pools["lb"][0]
    assert hc.stats.checks_performed == 63 and hc.stats.checks_timed_out == 6
    assert (lb.stats.backends_marked_unhealthy, lb.stats.backends_marked_healthy) == (1, 1) and lb.healthy_count == 3
    assert hc.get_backend_state(pools["server"][1]).last_check_passed is True
    sim, pools = _run(HS.FIXTURES["all_backends_down_then_one_back"])
    lb = pools["lb"][0]
    assert lb.stats.no_backend_available > 0 and [b.name for b in lb.healthy_backends] == ["srv1"]
    sim, pools = _run(HS.FIXTURES["checker_crash_with_restart"])         # the cycle chain ended: backends stay is_checking
    hc = pools["checker"][0]
    checking = [b.name for b in pools["server"] if hc.get_backend_state(b).is_checking]
    assert len(checking) > 0 and sorted(hc._pending_checks) == sorted(checking) and hc._crashed is False


@pytest.mark.parametrize("name", HS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event that
    was not dropped by a crash, probes included, in the one processing order of the whole graph; and the engine's count of every
    kind equals the trace's."""
    spec = HS.FIXTURES[name]
    trace = HR.get("case", spec)["trace"]
    sim, _pools, g, eng, end_ns, _start, _c = FC.engine(spec)
    with eng:
        eng.run_until(end_ns)
        node, t, _v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        events = eng.health_events()
    assert by_kind == [int((trace[:, 1] == k).sum()) for k in range(N.EV_KINDS)]
    assert internal.tolist() == [int((trace[:, 1] == N.EV_KINDS + k).sum()) for k in range(4)]
    assert events.tolist() == [int((trace[:, 1] == _FIRST_HC + k).sum()) for k in range(3)] and events[0] > 0
    want = FC.live_rows(trace)
    at_sink = g.arrays.kind[node] == N.NODE_SINK
    assert len(want) > 0 and np.array_equal(np.stack([t[at_sink], node[at_sink]], axis=1), want[:, [0, 2]])


def _run_to_ends_with_coop_count(spec, ends_s, flags=0, **caps):
    """FC.engine_run and the number of cooperative selections at the end."""
    return FC.engine_run(spec, ends_s, flags, read=lambda eng, g: eng.coop_selects(), **caps)


def test_windows_equal_one_run():
    for name in ("crash_then_restart_of_one_backend", "constant_ticks_on_the_cycle_nanoseconds", "weighted_round_robin_heaviest_backend_out"):
        spec = HS.FIXTURES[name]
        ends = [0.7, 1.0, 1.0, 2.25, 3.3, 5.0000001, spec["end_s"]]          # 7 uneven windows, ends on cycle and fault nanoseconds among them
        sim, pools, _ = _run_to_ends_with_coop_count(spec, ends)
        _equals_the_recording(spec, sim, pools, HR.get("case", spec))


def test_growth_from_capacities_of_one_equals_the_reference():
    """Heap, Request pool and record log start at their smallest: a cycle over 130 backends needs 261 heap entries and 130 Requests at
    once, and a probe that a crash dropped without freeing would show here."""
    for name in ("wrr_130_backends", "checker_crash_with_restart"):
        spec = HS.FIXTURES[name]
        sim, pools, _ = _run_to_ends_with_coop_count(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1)
        _equals_the_recording(spec, sim, pools, HR.get("case", spec))


def test_growth_under_a_backlog_equals_a_run_with_room():
    """Thousands of Requests queued behind slow backends while a checker cycles every 50 ms: the Request pool outgrows its first size
    (4 n + 1 024) several times, with cycles -- which need a Request and two heap entries per backend at once -- in between."""
    spec = HS._pool("growth_under_a_backlog", "least_conn", 3, rate=2500.0, mean=0.5, end_s=2.0, seed=5,
                    checkers=[HS.checker(interval=0.05, timeout=0.02, ht=1, ut=2)], faults=[HS.crash(["server", 1], 0.52, 1.31)])
    grown_sim, grown_pools, _ = _run_to_ends_with_coop_count(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1)
    roomy_sim, roomy_pools, _ = _run_to_ends_with_coop_count(spec, [spec["end_s"]], heap_capacity=1 << 16, request_capacity=1 << 16, record_capacity=1 << 16)
    grown, roomy = GF.results(spec, grown_sim, grown_pools, "health"), GF.results(spec, roomy_sim, roomy_pools, "health")
    assert roomy["depth"].sum() > 3000 and roomy["checker_stats"][0, 0] > 100 and roomy["lb_marks"][0, :2].tolist() == [1, 1]
    FC.same(grown, roomy)


@pytest.mark.parametrize("name", HS.WIDE)
def test_cooperative_and_lane_serial_selection_leave_the_same_bits(name):
    """33, 65 and 130 backends with unhealthy slots at 0, 31, 32, 63, 64 and the last, which stay out until the cycle at 3 s marks them
    healthy again, two more go out on the way: the wavefront's selection over the list with those holes (the default from
    kCoopMinBackends healthy backends on, and forced) and the lone lane's scan (forced) are the reference's.  The run stops at 2.9 s to
    see that Requests were forwarded while none went to a slot that was out."""
    spec = HS.FIXTURES[name]
    ref = HR.get("case", spec)
    nb = len(spec["servers"])
    out = [q for _j, q in spec["unhealthy"]]
    assert out == sorted({q for q in (0, 31, 32, 63, 64, nb - 1) if q < nb})
    results = []
    for flags in (0, N.GRAPH_DEBUG_COOPERATIVE, N.GRAPH_DEBUG_LANE_SERIAL):
        sim, pools, g, eng, end_ns, start_ns, cancelled = FC.engine(spec)
        lb = g.node_of[id(pools["lb"][0])]
        off = int(g.arrays.rt_off[lb])
        with eng:
            if flags:
                eng.set_debug_flags(flags)
            eng.run_until(start_ns + hs.Instant.from_seconds(HS.WIDE_OUT_UNTIL_S - 0.1).nanoseconds)
            taken = eng.stats()["rt_taken"][off:off + nb]
            early_coop = eng.coop_selects()
            h = eng.health(lb)
            assert taken.sum() > 100 and taken[out].sum() == 0 and not h["healthy"][out].any(), (flags, taken.sum(), taken[out].tolist())
            eng.run_until(end_ns)
            coop = eng.coop_selects()
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        got = _equals_the_recording(spec, sim, pools, ref)
        back = HS.wide_returning(spec)
        assert len(back) >= len(out) - 1 and got["lb_backend_total_requests"][back].sum() > 0 and got["lb_healthy"][back].all()      # ... and they came back, with traffic
        results.append(got)
        if flags == N.GRAPH_DEBUG_LANE_SERIAL:
            assert early_coop == 0 and coop == 0
        elif flags == N.GRAPH_DEBUG_COOPERATIVE:
            assert early_coop > 100 and coop > 0
        else:                                                  # 33 backends have kCoopMinBackends healthy ones only between the return at 3 s and
            assert (early_coop > 0) == (nb > 33) and coop > 0, (nb, early_coop, coop)      # the next mark: both sides of the threshold in one run
    FC.same(results[0], results[1])
    FC.same(results[0], results[2])


def test_replicas_in_one_batch_with_a_checker_free_handle():
    """hs_graph_run_many: eight replicas with different faults and, in the same launch, a graph without any health state."""
    import fault_specs as FS

    base = HS.FIXTURES["lb_crashed_while_marks_arrive"]
    specs = [dict(base, faults=[HS.crash(["server", i % 3], 0.5 + 0.4 * i, None if i % 3 == 0 else 4.0 + 0.3 * i), HS.pause(["lb", 0], 0.3 * i, 1.0 + 0.3 * i)])
             for i in range(8)]
    plain_spec = FS.FIXTURES["two_faults_two_entities"]
    built = []

    def build_fn():
        k = len(built)
        sim, pools = GF.build(specs[k]) if k < 8 else GF.build(plain_spec)
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 9, base_seed=900)
    assert len(results) == 9
    seen = set()
    for i, (sim, pools) in enumerate(built[:8]):
        assert isinstance(sim._graph, GeneralGraph) and sim._graph.arrays.has_health
        got = GF.results(specs[i], sim, pools, "health")
        one_sim, one_pools = _run(specs[i], seed=900 + i)
        FC.same(got, GF.results(specs[i], one_sim, one_pools, "health"), i)
        seen.add((got["total_events"], tuple(got["lb_marks"].ravel().tolist())))
    assert len(seen) > 4
    sim, pools = built[8]
    assert not sim._graph.arrays.has_health
    one_sim, one_pools = GF.build(plain_spec, seed=908)
    one_sim.run()
    FC.same(GF.results(plain_spec, sim, pools, "faults"), GF.results(plain_spec, one_sim, one_pools, "faults"), "plain")


def test_eight_groups_as_parts_equal_one_heap():
    """Eight LoadBalancer groups, each with its checker and one crash / restart, in ONE Simulation: the parts run side by side
    (hs_graph_run_parts), a checker in its LoadBalancer's part."""
    import happy_simulator_amd.simulation as S

    spec = HS.groups_spec(8)
    sim, pools = _run(spec)
    assert sim._graph_parts == 8
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    got = GF.results(spec, sim, pools, "health")
    FC.same(got, GF.results(spec, one_sim, one_pools, "health"))
    assert got["lb_marks"][:, 0].tolist() == [1] * 8 and got["lb_marks"][:, 1].tolist() == [1] * 8
    assert got["checker_stats"][:, 3].min() >= 2 and got["health_by_kind"][0] >= 8 * 8


def test_a_checker_node_that_was_never_configured_is_a_state_error():
    sim, _pools = GF.build(HS.FIXTURES["pause_of_one_backend"])
    g = sim.lowered()
    g.arrays.hc_params, g.arrays.lb_healthy = None, None                     # (the handle is created without any health call)
    hc = int(np.nonzero(g.arrays.kind == N.NODE_HEALTH_CHECKER)[0][0])
    with GraphEngine(g.arrays, seed=1) as eng:
        eng.schedule(hc, 0)
        with pytest.raises(N.EngineError, match="HealthChecker without its LoadBalancer") as e:
            eng.run_until(10 ** 9)
        assert e.value.code == N.HS_E_STATE


def test_health_state_after_the_first_run_is_a_state_error():
    sim, _pools, g, eng, end_ns, _s, _c = FC.engine(HS.FIXTURES["pause_of_one_backend"])
    lb = int(np.nonzero(g.arrays.kind == N.NODE_LB)[0][0])
    hc = int(np.nonzero(g.arrays.kind == N.NODE_HEALTH_CHECKER)[0][0])
    with eng:
        with pytest.raises(N.EngineError) as e:                              # a checker is configured once
            eng._check(eng._lib.hs_graph_set_health_checker(eng._h, hc, lb, 1.0, 0.5, 2, 3, 1))
        assert e.value.code == N.HS_E_STATE
        eng.run_until(end_ns)
        flags = np.ones(3, np.uint8)
        with pytest.raises(N.EngineError) as e:
            eng._check(eng._lib.hs_graph_set_lb_health(eng._h, lb, flags.ctypes.data, 3))
        assert e.value.code == N.HS_E_STATE
