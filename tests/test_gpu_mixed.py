"""GPU: graphs that mix the entity families of the single-heap loop (csrc/hs_graph.hip, the widest instantiation of graph_loop: every
handler of every family in one kernel) against the recorded live reference (tests/golden/live_mixed/, written by
tests/golden/make_golden_mixed.py).  Every comparison is exact equality: Sink records, every per-entity statistic of every family's
result reader, all by_kind slices, events_cancelled, the final `_crashed` flags, probes.  No case is skipped or excluded
(test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import mixed_specs as MX
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
MR = MX.MIXED
_NOT_COMPARED = MX.NOT_COMPARED
_BY_KIND_SLICES = MX.BY_KIND_SLICES
_FIRST_HC, _FIRST_WRAPPER, _FIRST_CLIENT, _FIRST_FLOW = N.EV_KINDS + 4, N.EV_KINDS + 7, N.EV_KINDS + 13, N.EV_KINDS + 16


def _equals_the_recording(spec, sim, pools, ref):
    got = MX.results(spec, sim, pools)
    FC.compare(spec["name"], got, ref, _NOT_COMPARED, _BY_KIND_SLICES)
    assert len(ref["by_kind"]) == 39
    return got


def _run(spec, **kw):
    sim, pools = MX.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph)
    return sim, pools


def _one_heap(spec):
    import happy_simulator_amd.simulation as S

    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        return _run(spec)
    finally:
        S.MAX_PARTS = old


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of mixed_specs, and every one has a recording."""
    names = [s["name"] for s in MX.all_specs()]
    assert len(names) == len(set(names)) == len(MX.FIXTURES) + MX.N_RANDOM and MX.N_RANDOM >= 150 and len(MX.FIXTURES) >= 24
    for spec in MX.all_specs():
        assert MR.get("case", spec)["total_events"] <= 40_000
    assert len(MX.TRACED) >= 8
    for name in MX.TRACED:
        assert len(MR.get("case", MX.FIXTURES[name])["trace"]) > 0
    assert not MX.REFUSED                                                     # (nothing accepted stays uncompared, nothing is set aside)


@pytest.mark.parametrize("name", sorted(MX.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = MX.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, MR.get("case", spec))


@pytest.mark.parametrize("k", range(MX.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = MX.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, MR.get("case", spec))


@pytest.mark.parametrize("name", MX.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event in
    the one processing order of the whole graph, and the engine's count of every kind of every family equals the trace's."""
    spec = MX.FIXTURES[name]
    ref = MR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = MX.engine(spec)
    a = g.arrays
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        health = eng.health_events() if a.has_health else np.zeros(3, np.int64)
        wrappers = eng.wrapper_events() if a.has_wrappers else np.zeros(6, np.int64)
        clients = eng.client_events() if a.has_clients else np.zeros(3, np.int64)
        flows = eng.flow_events() if a.has_flows else np.zeros(N.FLOW_KINDS + 1, np.int64)
    count = lambda first, n: [int((trace[:, 1] == first + k).sum()) for k in range(n)]  # noqa: E731
    assert by_kind == count(0, N.EV_KINDS)
    assert internal.tolist() == count(N.EV_KINDS, 4)
    assert np.asarray(health).tolist() == count(_FIRST_HC, 3) and np.asarray(wrappers).tolist() == count(_FIRST_WRAPPER, 6)
    assert np.asarray(clients).tolist() == count(_FIRST_CLIENT, 3) and flows[:N.FLOW_KINDS].tolist() == count(_FIRST_FLOW, N.FLOW_KINDS)
    want = FC.live_rows(trace)
    at_sink = a.kind[node] == N.NODE_SINK
    assert np.array_equal(np.stack([t[at_sink], node[at_sink]], axis=1), want[:, [0, 2]])


# window ends on gate, checker-cycle and client-timeout nanoseconds among uneven ones
_WINDOWS = {"gate_flush_into_a_client_fixed_retry": [0.25, 0.5, 0.5, 1.0, 1.05, 1.5, 2.0000001, 2.05],
            "gate_into_a_checked_load_balancer_wrr": [0.5, 0.7, 1.0, 1.2, 1.6, 2.0, 2.2, 2.5, 3.0],
            "client_target_is_a_checked_bounded_backend": [0.4, 0.55, 0.8, 1.2, 1.25, 2.0, 2.375],
            "one_schedule_four_origins_on_a_gate_events_nanosecond": [0.5, 0.5, 1.0, 1.1, 1.25, 2.0, 2.1],
            "probes_on_every_family": [0.1, 0.25, 1.0, 1.3, 2.0, 2.2, 3.0, 3.5],
            "crashed_processor_behind_a_clients_server": [0.3, 1.0, 1.05, 1.25, 2.0, 2.05]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    spec = MX.FIXTURES[name]
    sim, pools, _ = MX.engine_run(spec, _WINDOWS[name] + [None])
    _equals_the_recording(spec, sim, pools, MR.get("case", spec))


def test_an_auto_terminating_run_in_two_steps():
    spec = MX.FIXTURES["auto_terminating_run_with_three_daemon_families"]
    sim, pools, _ = MX.engine_run(spec, [0.55, None])
    _equals_the_recording(spec, sim, pools, MR.get("case", spec))


def test_a_flush_of_1100_into_a_bulkhead_grows_the_heap_in_front_of_one_event():
    """A closed gate with 1 100 queued Requests opens in front of a Bulkhead with 4 permits and 40 queue places.  The handle starts
    with the smallest heap the engine makes (1 024 entries + 4 per node); the one `_GateOpen` needs 1 100 entries: the launch stops in
    front of it, the heap grows, the flush happens whole and the Bulkhead hands out its permits in the flush's order.  Side by side
    (hs_graph_run_many) the heap passes the 1 024 entries that mode keeps in LDS."""
    spec = MX.big_flush_spec()
    ref = MR.get("case", spec)
    sim, _pools = MX.build(spec)
    n = sim.lowered().arrays.n
    assert ref["flow_stats"][0, :2].tolist() == [1100, 1100] and 4 * n + 1024 < 1100 and 1100 > 1024     # the flush alone exceeds both
    roomy_sim, roomy_pools, _ = MX.engine_run(spec, [None], heap_capacity=1 << 14, request_capacity=1 << 14, record_capacity=1 << 14)
    roomy = _equals_the_recording(spec, roomy_sim, roomy_pools, ref)
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = MX.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            launches = eng.summary().launches
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        assert launches >= 2 or side_by_side
        FC.same(_equals_the_recording(spec, sim, pools, ref), roomy, side_by_side)


def test_a_retry_storm_behind_a_batch_processor_while_every_buffer_grows():
    spec = MX.retry_storm_spec()
    ref = MR.get("case", spec)
    assert ref["cl_stats"][0, 3] >= 800 and ref["flow_stats"][0, 0] > 20
    sim, pools, _ = MX.engine_run(spec, [None], heap_capacity=1, request_capacity=1, record_capacity=1)
    got = _equals_the_recording(spec, sim, pools, ref)
    roomy_sim, roomy_pools, _ = MX.engine_run(spec, [None], heap_capacity=1 << 14, request_capacity=1 << 14, record_capacity=1 << 14)
    FC.same(got, MX.results(spec, roomy_sim, roomy_pools))


def test_64_replicas_equal_64_single_runs():
    base = MX.FIXTURES["checked_backends_into_a_processor_a_client_and_a_bulkhead"]
    other = MX.FIXTURES["probes_on_every_family"]
    specs = [dict(base if i % 2 == 0 else other, end_s=2.5) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = MX.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=1100)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph) and sim._graph.arrays.has_flows and sim._graph.arrays.has_clients and sim._graph.arrays.has_wrappers
        got = MX.results(specs[i], sim, pools)
        one_sim, one_pools = _run(specs[i], seed=1100 + i)
        FC.same(got, MX.results(specs[i], one_sim, one_pools), i)
        seen.add((got["total_events"], tuple(got["flow_stats"].ravel().tolist())))
    assert len(seen) > 48


def test_32_groups_as_parts_equal_one_heap_and_the_recording():
    """32 disconnected Source -> limiter -> GateController -> Client -> link -> Server -> Bulkhead -> Server -> Sink groups in ONE
    Simulation: the parts run side by side (hs_graph_run_parts) and leave what one heap over all of them leaves, which is what the
    reference's one heap left."""
    spec = MX.groups_spec(32)
    ref = MR.get("case", spec)
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1 and sim._graph_parts == 32
    got = _equals_the_recording(spec, sim, pools, ref)
    FC.same(got, _equals_the_recording(spec, one_sim, one_pools, ref))
    assert len(MX.families_of(ref)) == 4 and (got["cl_stats"][:, 0] > 0).all() and (got["wrap_stats"][:, 0] > 0).all() and (got["flow_stats"][:, 3] == 2).all()


@pytest.mark.parametrize("which, nodes", [(0, 49), (1, 48)])
def test_groups_around_the_node_window_equal_one_heap_and_the_recording(which, nodes):
    """Parts of 49 nodes are beyond the 48 node rows a side-by-side run keeps in LDS (kLdsNodesBatch), parts of 48 fill them."""
    from happy_simulator_amd.graph_engine import split_parts

    spec = MX.wide_groups_specs()[which]
    ref = MR.get("case", spec)
    sim, pools = _run(spec)
    sizes = [len(ids) for ids, _pos, _b in split_parts(sim._graph.arrays)]
    assert sizes == [nodes, nodes] and (nodes > 48) == (which == 0) and sim._graph_parts == 2          # it does cross the window / fill it
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1
    got = _equals_the_recording(spec, sim, pools, ref)
    FC.same(got, _equals_the_recording(spec, one_sim, one_pools, ref))
