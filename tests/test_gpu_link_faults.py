"""GPU: InjectLatency and InjectPacketLoss on links registered in a Network, on the single-heap loop (csrc/hs_graph.hip, the
link-fault instantiation of graph_loop) against the recorded live reference (tests/golden/live_link_faults/, written by
tests/golden/make_golden_link_faults.py).  Every comparison is exact equality: Sink records, every per-entity statistic of every
family's result reader, all by_kind slices, every link's packet_loss_rate and latency object, the fault in force per link, the values
read from every LOSS stream, every Network's traffic_matrix().  No case is skipped or excluded
(test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import link_fault_specs as LS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
LR = LS.LINK_FAULTS
_FIRST_HC, _FIRST_WRAPPER, _FIRST_CLIENT, _FIRST_FLOW = N.EV_KINDS + 4, N.EV_KINDS + 7, N.EV_KINDS + 13, N.EV_KINDS + 16


def _equals_the_recording(spec, sim, pools, ref):
    got = LS.results(spec, sim, pools)
    LS.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == 39 and "link_active_fault" in ref and "link_loss_draws" in ref
    return got


def _run(spec, **kw):
    sim, pools = LS.build(spec, **kw)
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
    """The parametrised tests below run every fixture and every random graph of link_fault_specs, and every one has a recording."""
    names = [s["name"] for s in LS.all_specs()]
    assert len(names) == len(set(names)) == len(LS.FIXTURES) + LS.N_RANDOM and LS.N_RANDOM >= 100 and len(LS.FIXTURES) >= 24
    for spec in LS.all_specs():
        ref = LR.get("case", spec)
        assert ref["total_events"] <= 40_000 and ref["by_kind"][17:19].sum() + ref["events_cancelled"] + ref["time_travel"] + ref["pending_events"] > 0
    assert len(LS.TRACED) >= 6
    for name in LS.TRACED:
        assert len(LR.get("case", LS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(LS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = LS.FIXTURES[name]
    if spec.get("windows"):
        sim, pools = LS.engine_run(spec, list(spec["windows"]) + [None])      # the reference ran it in these windows
    else:
        sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, LR.get("case", spec))


@pytest.mark.parametrize("k", range(LS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = LS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, LR.get("case", spec))


@pytest.mark.parametrize("name", LS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event in
    the one processing order of the whole graph, and the engine's count of every kind equals the trace's -- a link fault's two Events
    are the kinds fault_on / fault_off at the link's node."""
    spec = LS.FIXTURES[name]
    ref = LR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = LS.engine(spec)
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
    # the link-fault rows of the trace name the nodes the product lowered the links to
    link_nodes = {g.node_of[id(lk)] for lk in pools["link"]}
    n_link_rows = sum(2 for ft in spec["faults"] if LS.is_link_fault(ft) and not ft.get("cancel"))
    fault_rows = trace[(trace[:, 1] == FC.FAULT_ON) | (trace[:, 1] == FC.FAULT_OFF)]
    assert n_link_rows == 0 or set(fault_rows[:, 2].tolist()) & link_nodes
    # live_rows replays a crash flag per node off the fault rows: a link fault's rows carry the link's node without crashing it, so
    # they leave the trace first -- one row per link-fault Event of the Simulation, by (time, kind, node)
    keep = np.ones(len(trace), bool)
    for f in sim._general_faults(g):
        if len(f) == 5 and not f[3]:
            hit = np.nonzero(keep & (trace[:, 0] == f[1]) & (trace[:, 1] == (FC.FAULT_ON if f[2] else FC.FAULT_OFF)) & (trace[:, 2] == f[0]))[0]
            keep[hit[:1]] = False
    assert (~keep).sum() > 0
    want = FC.live_rows(trace[keep])
    at_sink = (a.kind[node] == N.NODE_SINK)
    assert np.array_equal(np.stack([t[at_sink], node[at_sink]], axis=1), want[:, [0, 2]])


def _fault_times(spec):
    """Every activation and deactivation time of the spec's faults, in seconds, inside the run."""
    out = set()
    for ft in spec["faults"]:
        out.update(x for x in (ft["at"], ft.get("end"), ft.get("restart")) if x is not None and 0.0 < x < spec["end_s"])
    return sorted(out)


# window ends ON activation and deactivation nanoseconds, among uneven ones
_WINDOWS = {"latency_window": [0.3, 1.4000001], "loss_window_on_a_lossless_link": [0.77], "two_overlapping_latency_faults_on_one_link": [1.75],
            "windows_that_outlast_the_run": [2.999], "crashed_link_while_its_fault_events_fire": [0.5, 2.3],
            "activation_on_the_nanosecond_a_request_reaches_the_link": [1.0, 1.5], "schedule_that_mixes_crash_pause_and_both_link_faults": [1.45],
            "latency_spike_behind_a_client": [1.08, 1.2], "lost_packet_under_a_timeout_wrapper_hook": [1.7]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    spec = LS.FIXTURES[name]
    ends = sorted(_WINDOWS[name] + _fault_times(spec))
    sim, pools = LS.engine_run(spec, ends + [None])
    _equals_the_recording(spec, sim, pools, LR.get("case", spec))


@pytest.mark.parametrize("name", ["loss_window_on_a_lossless_link", "two_overlapping_latency_faults_on_one_link", "lost_packet_under_a_bulkhead_hook",
                                  "schedule_that_mixes_crash_pause_and_both_link_faults", "auto_terminating_run"])
def test_growth_from_capacity_one(name):
    """Heap, Request and record capacity 1: every buffer grows across relaunches while link faults are pending and in force."""
    spec = LS.FIXTURES[name]
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = LS.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, LR.get("case", spec))


def test_64_replicas_equal_64_single_runs():
    base = LS.FIXTURES["schedule_that_mixes_crash_pause_and_both_link_faults"]
    other = LS.FIXTURES["two_overlapping_loss_faults_on_one_link"]
    specs = [dict(base if i % 2 == 0 else other, end_s=2.0) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = LS.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=1300)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph)
        got = LS.results(specs[i], sim, pools)
        one_sim, one_pools = _run(specs[i], seed=1300 + i)
        FC.same(got, LS.results(specs[i], one_sim, one_pools), i)
        seen.add((got["total_events"], tuple(got["link_loss_draws"].tolist()), tuple(got["packets_dropped"].tolist())))
    assert len(seen) > 48


def test_32_groups_as_parts_equal_one_heap_and_the_recording():
    """32 disconnected Source -> link -> Server -> Sink chains in ONE Simulation with a fault on every link: the parts run side by side
    (hs_graph_run_parts), every fault Event in the part of its link, and leave what one heap over all of them leaves, which is what the
    reference's one heap left."""
    spec = LS.groups_spec(32)
    ref = LR.get("case", spec)
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1 and sim._graph_parts == 33            # (the 32 chains, and the Network: a node nothing reaches)
    got = _equals_the_recording(spec, sim, pools, ref)
    FC.same(got, _equals_the_recording(spec, one_sim, one_pools, ref))
    assert got["link_loss_draws"].sum() > 100 and got["packets_dropped"].sum() > 20


def test_a_batch_that_mixes_faulted_and_unfaulted_graphs():
    """hs_graph_run_many over two handles with link faults and the same two graphs without them (one keeps a node fault, one a lossy
    link and no fault at all): the whole batch runs the link-fault instantiation, and every handle leaves what it leaves alone."""
    faulted = [LS.FIXTURES["crashed_link_while_its_fault_events_fire"], LS.FIXTURES["two_overlapping_loss_faults_on_one_link"]]
    bare = [LS.without_link_faults(s) for s in faulted]
    specs = [faulted[0], bare[0], faulted[1], bare[1]]
    made = [LS.engine(s) for s in specs]
    assert [any(len(f) == 5 for f in m[0]._general_faults(m[2])) for m in made] == [True, False, True, False]
    assert len({m[4] for m in made}) == 1
    try:
        GraphEngine.run_many([m[3] for m in made], made[0][4])
        for m in made:
            m[0]._general_finish(m[2], m[3], m[4], m[6], 0.0)
    finally:
        for m in made:
            m[3].close()
    for k in (0, 2):
        _equals_the_recording(specs[k], made[k][0], made[k][1], LR.get("case", specs[k]))
    for spec, m in zip(specs, made):
        one_sim, one_pools = _run(spec)
        FC.same(LS.results(spec, m[0], m[1]), LS.results(spec, one_sim, one_pools), spec["name"])


_WINDOWED = sorted(n for n, s in LS.FIXTURES.items() if s.get("windows"))


@pytest.mark.parametrize("name", _WINDOWED)
def test_object_state_after_every_window(name):
    """The results are bound behind EVERY window of a windowed run, as the reference's objects can be read between two windows: each
    link's packet_loss_rate and latency object -- the original, or the `_CompoundLatency` of the activation in force -- equal what the
    reference's link held behind the same window (ends on activation nanoseconds and inside fault windows among them)."""
    spec = LS.FIXTURES[name]
    ref = LR.get("case", spec)
    ends = list(spec["windows"]) + [None]
    assert len(_WINDOWED) >= 3 and set(LS.WINDOW_KEYS) <= set(ref) and len(ref["window_link_loss_rate"]) == len(ends)
    sim, pools, g, eng, end_ns, start_ns, cancelled = LS.engine(spec)
    seen = set()
    with eng:
        for k, t in enumerate(ends):
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
            got = LS.link_state(pools)
            for key, have in got.items():
                want = ref["window_" + key][k]
                assert have.dtype == want.dtype and have.shape == want.shape and have.tobytes() == want.tobytes(), (name, k, key, have.tolist(), want.tolist())
            lk = pools["link"][0]
            seen.add((type(lk.latency).__name__, lk.packet_loss_rate))
            if type(lk.latency).__name__ == "_CompoundLatency":
                assert isinstance(lk.latency._base, hs.ConstantLatency) and isinstance(lk.latency._extra, hs.ConstantLatency)
                assert lk.latency._mean_latency == lk.latency._base.mean + lk.latency._extra.mean
    assert len(seen) >= 2                                   # the state changed between two windows
    _equals_the_recording(spec, sim, pools, ref)


def test_object_state_after_a_run():
    """What run() leaves on the user's objects while a window outlasts it: the latency object and the rate of the activation in force,
    get_latency on the host, traffic_matrix() off the written-back counters."""
    spec = LS.FIXTURES["windows_that_outlast_the_run"]
    sim, pools = _run(spec)
    lk, nw = pools["link"][0], pools["network"][0]
    assert type(lk.latency).__name__ == "_CompoundLatency" and isinstance(lk.latency._base, hs.ConstantLatency) and lk.latency._base.mean == 0.02
    assert isinstance(lk.latency._extra, hs.ConstantLatency) and lk.latency._extra.mean == 30.0 / 1000.0
    assert lk.latency._mean_latency == 0.02 + 30.0 / 1000.0 and lk.latency.get_latency(hs.Instant.Epoch).nanoseconds == 50_000_000
    assert lk.packet_loss_rate == min(1.0, 0.0 + 0.2)
    (st,) = nw.traffic_matrix()
    assert (st.source, st.destination) == ("link0", "srv0") and st.packets_sent == lk.packets_sent > 0 and st.packets_dropped == lk.packets_dropped > 0
    assert (nw.events_routed, nw.events_dropped_no_route, nw.events_dropped_partition) == (0, 0, 0)
    spec = LS.FIXTURES["latency_window"]
    sim, pools = _run(spec)
    assert type(pools["link"][0].latency) is hs.ConstantLatency and pools["link"][0].packet_loss_rate == 0.0
