"""GPU: FaultSchedule with CrashNode / PauseNode on the single-heap loop (csrc/hs_graph.hip kEvFaultOn / kEvFaultOff and the drop at
dispatch) against the recorded live reference (tests/golden/live_faults/, written by tests/golden/make_golden_faults.py).  Every
comparison is exact equality: Sink records, per-entity statistics, limiter and LoadBalancer state, probe samples, event totals
including the fault count, the first Event beyond the end, the final `_crashed` flags.  No case is skipped or excluded
(test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import fault_specs as FS
import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import rate_limiter_specs as RS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine
from recorded import FAULTS as FR

pytestmark = pytest.mark.gpu

# what the engine has no counterpart for (the reference heap's length, the recorder's time-travel count) or what is compared in a
# form of its own (by_kind: the engine reports the public fifteen kinds, the four internal ones per node / per graph; trace:
# test_record_order_follows_the_trace)
_NOT_COMPARED = {"trace", "by_kind", "pending_events", "time_travel"}
_FAULT_ON, _FAULT_OFF = FC.FAULT_ON, FC.FAULT_OFF
# the four internal kinds are counted like the public ones (an Event dropped at a crashed limiter is counted, not handled)
_BY_KIND_SLICES = [("by_kind", N.EV_KINDS), ("internal_by_kind", N.EV_KINDS + 4)]


def _equals_the_recording(spec, sim, pools, ref):
    got = GF.results(spec, sim, pools, "faults")
    FC.compare(spec["name"], got, ref, _NOT_COMPARED, _BY_KIND_SLICES)
    assert got["fault_events"] == int(ref["by_kind"][_FAULT_ON] + ref["by_kind"][_FAULT_OFF])
    assert np.all(got["lim_events"].sum(axis=0) <= got["internal_by_kind"][:2])
    return got


def _run(spec, **kw):
    sim, pools = GF.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "fault" in sim._station_refusal
    return sim, pools


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of fault_specs, and every one has a recording."""
    names = [s["name"] for s in FS.all_specs()]
    assert len(names) == len(set(names)) == len(FS.FIXTURES) + FS.N_RANDOM and FS.N_RANDOM >= 120
    for spec in FS.all_specs():
        FR.get("case", spec)
    for name in FS.TRACED:
        assert len(FR.get("case", FS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(FS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = FS.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, FR.get("case", spec))


@pytest.mark.parametrize("k", range(FS.N_RANDOM))
def test_random_graph_with_faults_equals_the_reference(k):
    spec = FS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, FR.get("case", spec))


def test_the_reference_quirks_the_issue_lists():
    """What the recordings pin about the reference, read off the product's own objects."""
    sim, pools = _run(FS.FIXTURES["cancelled_before_construction"])       # cancelled too early: the fault fires, stats say 1
    assert pools["fault_schedule"].stats == hs.FaultStats(1, 0, 0, 1) and sim._fault_events_processed == 2
    assert sim.summary.events_cancelled == 0
    sim, pools = _run(FS.FIXTURES["cancelled_after_construction"])        # its two Events pop as cancelled
    assert pools["fault_schedule"].stats == hs.FaultStats(2, 0, 0, 1) and sim.summary.events_cancelled == 2
    sim, pools = _run(FS.FIXTURES["source_crash_restart"])                # a crashed Source dies for good
    assert pools["source"][0]._crashed is False and max(pools["sink"][0].completion_ns) < 4 * 10 ** 9
    sim, pools = _run(FS.FIXTURES["fault_is_the_event_beyond_the_end"])
    assert sim._current_time.nanoseconds == 3_000_010_000 and pools["server"][0]._crashed is True
    sim, pools = _run(FS.FIXTURES["auto_terminate_pending_restart"])      # daemons do not keep the run alive
    assert pools["server"][0]._crashed is True and sim._fault_events_processed == 1
    for k in RS.POLICIES:
        sim, pools = _run(FS.FIXTURES[f"limiter_{k}_crash"])              # the dropped poll leaves _poll_scheduled set
        lim = pools["limiter"][0]
        assert lim._poll_scheduled and lim.queue_depth > 0 and lim._crashed is False


@pytest.mark.parametrize("name", FS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event and
    every Request at a limiter that was NOT dropped by a crash, in the one processing order of the whole graph; and the engine's
    count of every kind equals the trace's."""
    spec = FS.FIXTURES[name]
    trace = FR.get("case", spec)["trace"]
    sim, _pools, g, eng, end_ns, _start, _c = FC.engine(spec)
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        n_fault = int(internal[2] + internal[3])
    assert by_kind == [int((trace[:, 1] == k).sum()) for k in range(N.EV_KINDS)]
    assert n_fault == int((trace[:, 1] >= _FAULT_ON).sum()) >= 2
    kind = g.arrays.kind[node]
    arrivals = ((kind == N.NODE_RATE_LIMITER) & (v != N.LIMITER_DRAINED)) | (kind == N.NODE_SINK)
    # the Events the reference popped while their target was crashed produced nothing
    want = FC.live_rows(trace, (N.EV_KINDS, N.EV_NAMES.index("sink")))
    assert len(want) > 0 and np.array_equal(np.stack([t[arrivals], node[arrivals]], axis=1), want[:, [0, 2]])


def test_windows_equal_one_run():
    for name in ("server_crash_c2_bounded", "lockstep_tick_grid", "limiter_token_crash"):
        spec = FS.FIXTURES[name]
        ends = [0.7, 1.3, 1.3, 2.0, 2.6, 3.1, spec["end_s"]]             # (ends on the faults' own nanoseconds among them)
        sim, pools, _ = FC.engine_run(spec, ends)
        _equals_the_recording(spec, sim, pools, FR.get("case", spec))


def test_growth_from_capacities_of_one_equals_the_plain_run():
    """Heap, Request pool and record log start at one entry: a Request that a crash dropped without freeing would show here."""
    spec = FS._chain("growth", [FS.crash(["server", 0], 0.2, 0.5), FS.pause(["sink", 0], 0.7, 0.9)], rate=2000.0, mean=0.0004, end_s=1.2, seed=3)
    grown_sim, grown_pools, _ = FC.engine_run(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1)
    plain_sim, plain_pools = _run(spec)
    grown, plain = GF.results(spec, grown_sim, grown_pools, "faults"), GF.results(spec, plain_sim, plain_pools, "faults")
    assert plain["generated"][0] - plain["accepted"][0] > 400 and plain["completed"][0] - plain["received"][0] > 200    # both drops happened
    FC.same(grown, plain)


def test_replicas_with_different_schedules_equal_single_runs():
    specs = [dict(FS.FIXTURES["two_faults_two_entities"],
                  faults=[FS.crash(["server", i % 2], 0.5 + 0.2 * i, None if i % 3 == 0 else 2.0 + 0.1 * i), FS.pause(["sink", (i + 1) % 2], 0.3 * i, 1.0 + 0.3 * i)])
             for i in range(8)]
    built = []

    def build_fn():
        sim, pools = GF.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 8, base_seed=700)
    assert len(results) == 8
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph)
        got = GF.results(specs[i], sim, pools, "faults")
        one_sim, one_pools = _run(specs[i], seed=700 + i)
        FC.same(got, GF.results(specs[i], one_sim, one_pools, "faults"), i)
        seen.add((got["total_events"], tuple(got["crashed"].tolist())))
    assert len(seen) > 4


@pytest.mark.parametrize("grid", [False, True])
def test_600_chains_as_parts_equal_one_heap(grid):
    """600 disconnected chains, a third of them with a fault, in ONE Simulation: the parts run side by side, a fault Event in the part
    of the entity it names.  grid=True: lock-step constant Sources and one fault on a tick nanosecond -- that part is undecided and the
    run is handed to the one heap."""
    import happy_simulator_amd.simulation as S

    spec = FS.chains_spec(600, f"chains_{grid}", grid=grid, kind="constant" if grid else "poisson")
    sim, pools = _run(spec)
    assert sim._graph_parts == 1 if grid else sim._graph_parts > 1
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    got = GF.results(spec, sim, pools, "faults")
    FC.same(got, GF.results(spec, one_sim, one_pools, "faults"))
    assert got["fault_events"] > 200 and got["crashed"].sum() > 30


def test_flags_in_lds_and_in_hbm_give_the_same_result():
    """240 nodes on ONE heap: rows and flags stay in HBM; as parts of four nodes: in LDS -- and both are the reference's."""
    import happy_simulator_amd.simulation as S

    spec = FS.FIXTURES["nodes_beyond_lds"]
    ref = FR.get("case", spec)
    sim, pools = _run(spec)
    assert sim._graph.arrays.n > 192 and sim._graph_parts > 1
    got = _equals_the_recording(spec, sim, pools, ref)
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    FC.same(got, _equals_the_recording(spec, one_sim, one_pools, ref))
    # ... and a small graph alone on the large kernel (rows in LDS) against the side-by-side kernel (its own LDS rows)
    small = FS.FIXTURES["two_faults_two_entities"]
    a_sim, a_pools, _ = FC.engine_run(small, [small["end_s"]])
    _equals_the_recording(small, a_sim, a_pools, FR.get("case", small))


def test_a_fault_after_the_first_run_is_a_state_error():
    sim, _pools, _g, eng, end_ns, _s, _c = FC.engine(FS.FIXTURES["pause_sink"])
    with eng:
        eng.run_until(end_ns)
        with pytest.raises(N.EngineError) as e:
            eng.add_fault(0, 1, True)
        assert e.value.code == N.HS_E_STATE
        with pytest.raises(N.EngineError):
            GraphEngine.add_fault(eng, 10 ** 6, 1, True)
