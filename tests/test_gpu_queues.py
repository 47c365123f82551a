"""GPU: Servers whose queue is a LIFOQueue, an AdaptiveLIFO or a CoDelQueue on the single-heap loop (csrc/hs_graph.hip, the
queue-policy instantiation of graph_loop) against the recorded live reference (tests/golden/live_queues/, written by
tests/golden/make_golden_queues.py).  Every comparison is exact equality: Sink records, every per-entity statistic of every family's
result reader, all by_kind slices, every stats field and every state variable of every policy object.  No case is skipped or
excluded (test_every_recorded_case_is_compared)."""
import math

import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import queue_specs as QS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
QR = QS.QUEUES
_FIRST_HC, _FIRST_WRAPPER, _FIRST_CLIENT, _FIRST_FLOW = N.EV_KINDS + 4, N.EV_KINDS + 7, N.EV_KINDS + 13, N.EV_KINDS + 16


def _equals_the_recording(spec, sim, pools, ref):
    got = QS.results(spec, sim, pools)
    QS.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == 39 and "q_state" in ref
    return got


def _run(spec, **kw):
    sim, pools = QS.build(spec, **kw)
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
    """The parametrised tests below run every fixture and every random graph of queue_specs, and every one has a recording."""
    names = [s["name"] for s in QS.all_specs()]
    assert len(names) == len(set(names)) == len(QS.FIXTURES) + QS.N_RANDOM and QS.N_RANDOM >= 120 and len(QS.FIXTURES) >= 36
    for spec in QS.all_specs():
        assert QR.get("case", spec)["total_events"] <= 40_000
    assert len(QS.TRACED) >= 6
    for name in QS.TRACED:
        assert len(QR.get("case", QS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(QS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = QS.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, QR.get("case", spec))
    assert sim._graph.arrays.has_queue_policies


@pytest.mark.parametrize("k", range(QS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = QS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, QR.get("case", spec))


@pytest.mark.parametrize("name", QS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event in
    the one processing order of the whole graph, and the engine's count of every kind equals the trace's -- the policies add none."""
    spec = QS.FIXTURES[name]
    ref = QR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = QS.engine(spec)
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


def _enqueue_and_pop_times(name, n=3):
    """A few nanoseconds at which the traced reference run enqueued at / popped from Server 0, as seconds since the start."""
    spec = QS.FIXTURES[name]
    trace = QR.get("case", spec)["trace"]
    start = int(spec.get("start_ns", 0))
    out = []
    for kind in (N.EV_NAMES.index("enqueue"), N.EV_NAMES.index("poll")):
        rows = trace[trace[:, 1] == kind]
        out += [(int(rows[len(rows) * (j + 1) // (n + 1), 0]) - start) / 1e9 for j in range(n)]
    return out


# window ends on enqueue and pop nanoseconds among uneven ones
_WINDOWS = {"lifo_unbounded_overloaded": [0.31, 0.9], "alifo_threshold_3_switches_modes": [0.25, 2.0000001], "codel_c2_enters_leaves_and_re_enters": [0.7, 3.3],
            "codel_one_nanosecond_interval_drains_the_queue": [1.0, 1.05], "lifo_then_codel_in_tandem": [0.5, 0.5], "alifo_behind_a_gate_flush": [1.0, 2.0],
            "codel_checked_backend": [0.25, 1.0, 2.1]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    spec = QS.FIXTURES[name]
    ends = sorted(_WINDOWS[name] + _enqueue_and_pop_times(name))
    sim, pools = QS.engine_run(spec, ends + [None])
    _equals_the_recording(spec, sim, pools, QR.get("case", spec))


@pytest.mark.parametrize("name", ["lifo_unbounded_overloaded", "alifo_threshold_3_switches_modes", "codel_c2_enters_leaves_and_re_enters",
                                  "codel_one_nanosecond_interval_drains_the_queue", "codel_behind_a_gate_flush"])
def test_growth_from_capacity_one(name):
    """Heap, Request and record capacity 1: every buffer grows across relaunches while Requests wait in a policy's queue (their links
    and CoDel's enqueue times move with the Request array)."""
    spec = QS.FIXTURES[name]
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = QS.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, QR.get("case", spec))


def test_64_replicas_equal_64_single_runs():
    base = QS.FIXTURES["codel_c2_enters_leaves_and_re_enters"]
    other = QS.FIXTURES["alifo_checked_backend"]
    specs = [dict(base if i % 2 == 0 else other, end_s=2.0) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = QS.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=1200)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph) and sim._graph.arrays.has_queue_policies
        got = QS.results(specs[i], sim, pools)
        one_sim, one_pools = _run(specs[i], seed=1200 + i)
        FC.same(got, QS.results(specs[i], one_sim, one_pools), i)
        seen.add((got["total_events"], tuple(got["q_state"].ravel().tolist())))
    assert len(seen) > 48


def test_32_groups_as_parts_equal_one_heap_and_the_recording():
    """32 disconnected Source -> Server(policy) -> Server -> Sink chains in ONE Simulation: the parts run side by side
    (hs_graph_run_parts), every policy row with its Server, and leave what one heap over all of them leaves, which is what the
    reference's one heap left."""
    spec = QS.groups_spec(32)
    ref = QR.get("case", spec)
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1 and sim._graph_parts == 32
    got = _equals_the_recording(spec, sim, pools, ref)
    FC.same(got, _equals_the_recording(spec, one_sim, one_pools, ref))
    assert len(got["q_state"]) == 32 and set(got["q_state"][:, 1].tolist()) == {1, 2, 3}


def test_a_batch_that_mixes_handles_with_and_without_policies():
    """hs_graph_run_many over a handle with a CoDelQueue behind a Bulkhead, one with an AdaptiveLIFO behind a Client and the same two
    graphs with FIFO Servers (the wrapper and the Client keep them on the single-heap loop): the
    whole batch runs the queue-policy instantiation, and every handle leaves what it leaves alone."""
    with_policy = [QS.FIXTURES["codel_behind_a_small_bulkhead"], QS.FIXTURES["alifo_behind_a_client_with_fixed_retry"]]
    without = [QS.without_policies(s) for s in with_policy]
    specs = [with_policy[0], without[0], with_policy[1], without[1]]
    made = [QS.engine(s) for s in specs]
    assert [m[2].arrays.has_queue_policies for m in made] == [True, False, True, False]
    assert len({m[4] for m in made}) == 1
    try:
        GraphEngine.run_many([m[3] for m in made], made[0][4])
        for m in made:
            m[0]._general_finish(m[2], m[3], m[4], m[6], 0.0)
    finally:
        for m in made:
            m[3].close()
    for k in (0, 2):
        _equals_the_recording(specs[k], made[k][0], made[k][1], QR.get("case", specs[k]))
    for spec, m in zip(specs, made):
        one_sim, one_pools = _run(spec)
        FC.same(QS.results(spec, m[0], m[1]), QS.results(spec, one_sim, one_pools), spec["name"])


def test_codel_control_law_step_equals_cpython():
    """hs_debug_codel_next: Duration.from_seconds(interval / math.sqrt(count)) in ns on the device, one pair per thread, for counts
    1 .. 65 536 and four intervals, against CPython bit for bit."""
    lib = N.lib()
    intervals = (0.1, 0.02, 0.3, 1e-9)
    count = np.tile(np.arange(1, 65_537, dtype=np.int64), len(intervals))
    interval = np.repeat(np.array(intervals, np.float64), 65_536)
    out = np.full(len(count), -1, np.int64)
    rc = lib.hs_debug_codel_next(0, len(count), count.ctypes.data, interval.ctypes.data, out.ctypes.data)
    assert rc == N.HS_OK, (lib.hs_graph_last_error(None) or b"").decode()
    want = np.array([int(iv / math.sqrt(c) * 1e9) for iv in intervals for c in range(1, 65_537)], np.int64)
    assert np.array_equal(out, want), np.nonzero(out != want)[0][:8]
    assert want[65_536 * 3] == 1 and (want[65_536 * 3 + 1:] == 0).all()     # interval 1e-9: 0 ns from count = 2 on
