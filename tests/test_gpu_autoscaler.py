"""GPU: an AutoScaler over a LoadBalancer on the single-heap loop (csrc/hs_graph.hip, the scaler instantiation of graph_loop) against
the recorded live reference (tests/golden/live_autoscaler/, written by tests/golden/make_golden_autoscaler.py).  Every comparison is
exact equality: Sink records, every per-entity statistic of every family's result reader, all by_kind slices (row 39:
`_autoscaler_evaluate`), every AutoScalerStats field, the scaling history element for element, `_next_instance_id`, the last action and
its time, the managed instances, the LoadBalancer's members in order, `get_backend_info` of a removed instance, the strategy's
weights and current weights, and the Server statistics of every instance the run activated.  No case is skipped or excluded
(test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import autoscaler_specs as AS
import family_checks as FC
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
AR = AS.AUTOSCALER


def _equals_the_recording(spec, sim, pools, ref):
    got = AS.results(spec, sim, pools)
    AS.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == 40 and "as_state" in ref and "as_history" in ref and "as_instance_stats" in ref
    return got


def _run(spec, **kw):
    sim, pools = AS.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "AutoScaler" in sim._station_refusal
    return sim, pools


def _one_heap(spec):
    import happy_simulator_amd.simulation as S

    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        return _run(spec)
    finally:
        S.MAX_PARTS = old


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of autoscaler_specs, and every one has a recording."""
    names = [s["name"] for s in AS.all_specs()]
    assert len(names) == len(set(names)) == len(AS.FIXTURES) + AS.N_RANDOM and AS.N_RANDOM >= 100 and len(AS.FIXTURES) >= 30
    for spec in AS.all_specs():
        ref = AR.get("case", spec)
        assert ref["total_events"] <= 20_000 and ref["by_kind"][AS.EV_AS_EVAL] > 0 and ref["python"][:2] < [3, 12]
    assert len(AS.TRACED) >= 8
    for name in AS.TRACED:
        assert len(AR.get("case", AS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(AS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = AS.FIXTURES[name]
    if spec.get("windows"):
        sim, pools = AS.engine_run(spec, list(spec["windows"]) + [None])      # the reference ran it in these windows
    else:
        sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, AR.get("case", spec))


@pytest.mark.parametrize("k", range(AS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = AS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, AR.get("case", spec))


@pytest.mark.parametrize("name", AS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event in
    the one processing order of the whole graph -- at the node numbers the pool's instances were lowered to --, every Probe sample,
    and the engine's count of every kind equals the trace's."""
    spec = AS.FIXTURES[name]
    ref = AR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = AS.engine(spec)
    a = g.arrays
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        health, wrappers, clients = eng.health_events(), eng.wrapper_events() if a.has_wrappers else np.zeros(6, np.int64), (
            eng.client_events() if a.has_clients else np.zeros(3, np.int64))
        flows = eng.flow_events() if a.has_flows else np.zeros(N.FLOW_KINDS + 1, np.int64)
        evals = eng.scaler_events()
    count = lambda first, n: [int((trace[:, 1] == first + k).sum()) for k in range(n)]  # noqa: E731
    assert by_kind == count(0, N.EV_KINDS) and internal.tolist() == count(N.EV_KINDS, 4)
    assert np.asarray(health).tolist() == count(N.EV_KINDS + 4, 3) and np.asarray(wrappers).tolist() == count(N.EV_KINDS + 7, 6)
    assert np.asarray(clients).tolist() == count(N.EV_KINDS + 13, 3) and flows[:N.FLOW_KINDS].tolist() == count(N.EV_KINDS + 16, N.FLOW_KINDS)
    assert [evals] == count(AS.EV_AS_EVAL, 1) and evals > 0
    # the evaluate rows of the trace name the node the product lowered the scaler to; instance rows lie behind the Simulation's own nodes
    assert set(trace[trace[:, 1] == AS.EV_AS_EVAL][:, 2].tolist()) == {g.node_of[id(s)] for s in pools["scaler"]}
    assert trace[:, 2].max() < a.n and (trace[:, 2] >= g.n_own).any() == bool(ref["as_state"][:, 6].any())
    want = FC.live_rows(trace, kinds=(N.EV_NAMES.index("sink"), N.EV_NAMES.index("probe")))
    kept = (a.kind[node] == N.NODE_SINK) | (a.kind[node] == N.NODE_PROBE)
    assert np.array_equal(np.stack([t[kept], node[kept]], axis=1), want[:, [0, 2]])


# window ends ON evaluation nanoseconds, among uneven ones
_WINDOWS = {"target_utilization_scales_out_and_in": [0.5, 1.7000001, 2.5], "queue_depth_scales_out_and_in": [1.0, 1.0, 3.3],
            "cooldowns_block_scale_out_and_scale_in": [0.25, 2.0], "removed_instance_completes_work_afterwards": [4.5, 5.0],
            "started_twice": [0.0, 1.5], "crashed_scaler_never_ticks_again": [1.1, 1.5], "wlc_qd": [2.75], "gate_flush_in_front_of_the_pool": [1.0, 1.25],
            "probe_on_current_count": [0.25, 3.0], "two_scaled_load_balancers": [1.9]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    spec = AS.FIXTURES[name]
    sim, pools = AS.engine_run(spec, _WINDOWS[name] + [None])
    _equals_the_recording(spec, sim, pools, AR.get("case", spec))


@pytest.mark.parametrize("name", ["step_scaling_scales_out_and_in", "started_twice", "wrr_tu", "instances_in_front_of_a_bulkhead",
                                  "scale_in_with_nothing_managed"])
def test_growth_from_capacity_one(name):
    """Heap, Request and record capacity 1: every buffer -- the scaling history among them -- grows across relaunches."""
    spec = AS.FIXTURES[name]
    ref = AR.get("case", spec)
    assert ref["as_state"][0, 12] >= 5                     # more records than the history's first capacity of 1
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = AS.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, ref)


_WINDOWED = sorted(n for n, s in AS.FIXTURES.items() if s.get("windows"))


@pytest.mark.parametrize("name", _WINDOWED)
def test_object_state_after_every_window(name):
    """The results are bound behind EVERY window of a windowed run: each scaler's statistics, its last action and time, its
    `_next_instance_id` and its LoadBalancer's members equal what the reference's objects held behind the same window."""
    spec = AS.FIXTURES[name]
    ref = AR.get("case", spec)
    ends = list(spec["windows"]) + [None]
    assert len(_WINDOWED) >= 3 and AS.WINDOW_KEYS <= set(ref) and len(ref["window_as_state"]) == len(ends)
    sim, pools, g, eng, end_ns, start_ns, cancelled = AS.engine(spec)
    with eng:
        for k, t in enumerate(ends):
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
            got = AS.scaler_state(pools)
            assert got["as_state"].tolist() == ref["window_as_state"][k].tolist(), (name, k)
            assert got["as_members"] == ref["window_as_members"][k], (name, k)
    _equals_the_recording(spec, sim, pools, ref)


def test_32_replicas_equal_32_single_runs():
    base, other = AS.FIXTURES["wrr_tu"], AS.FIXTURES["started_twice_with_cooldowns"]
    specs = [dict(base if i % 2 == 0 else other, end_s=3.0) for i in range(32)]
    built = []

    def build_fn():
        sim, pools = AS.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 32, base_seed=1700)
    assert len(results) == 32
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph)
        got = AS.results(specs[i], sim, pools)
        if i < 8:
            one_sim, one_pools = _run(specs[i], seed=1700 + i)
            one = AS.results(specs[i], one_sim, one_pools)
            assert set(got) == set(one)
            for key in one:
                assert (got[key] == one[key]) if isinstance(one[key], list) else np.array_equal(np.asarray(got[key]), np.asarray(one[key])), (i, key)
        seen.add((got["total_events"], tuple(got["as_state"][0].tolist())))
    assert len(seen) > 24


def test_16_groups_as_parts_equal_one_heap_and_the_recording():
    """16 disconnected scaled chains in ONE Simulation: the parts run side by side (hs_graph_run_parts), every pool in the part of its
    LoadBalancer, and leave what one heap over all of them leaves, which is what the reference's one heap left."""
    spec = AS.groups_spec(16)
    ref = AR.get("case", spec)
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1
    got = _equals_the_recording(spec, sim, pools, ref)
    _equals_the_recording(spec, one_sim, one_pools, ref)
    assert got["as_state"][:, 1].sum() > 16


def test_a_batch_that_mixes_scaled_and_other_graphs():
    """hs_graph_run_many over two scaled graphs, a health-checked one and a plain mixed one: the whole batch runs the scaler
    instantiation, and every handle leaves what it leaves alone."""
    import mixed_specs as MX

    scaled = [AS.FIXTURES["least_conn_step"], AS.FIXTURES["crashed_scaler_never_ticks_again"]]
    others = [dict(MX.FIXTURES["gate_into_a_checked_load_balancer_wrr"], end_s=5.0), dict(MX.FIXTURES["client_server_batch_processor"], end_s=5.0)]
    made = [AS.engine(s) for s in scaled] + [FC.engine(s) for s in others]
    assert len({m[4] for m in made}) == 1
    try:
        GraphEngine.run_many([m[3] for m in made], made[0][4])
        for m in made:
            m[0]._general_finish(m[2], m[3], m[4], m[6], 0.0)
    finally:
        for m in made:
            m[3].close()
    for spec, m in zip(scaled, made):
        _equals_the_recording(spec, m[0], m[1], AR.get("case", spec))
    for spec, m in zip(others, made[2:]):
        one_sim, one_pools = MX.build(spec)
        one_sim.run()
        FC.same(MX.results(spec, m[0], m[1]), MX.results(spec, one_sim, one_pools), spec["name"])


def test_a_pool_one_instance_too_small_ends_the_run_with_an_error():
    """The engine-level hook: the same graph with the last pool instance taken off the LoadBalancer's targets and the pool's size one
    below what the run needs.  The run returns HS_E_OVERFLOW with a message that names the scaler -- it never goes on silently."""
    spec = AS.FIXTURES["step_scaling_scales_out_and_in"]
    need = int(AR.get("case", spec)["as_state"][0, 6])     # instances the run creates
    sim, pools = AS.build(spec)
    g = sim.lowered()
    a = g.arrays
    node = g.node_of[id(pools["scaler"][0])]
    lb_node = int(a.target[node])
    size = int(a.as_params[node, 8])
    assert size > need > 1 and int(a.rt_off[lb_node]) + int(a.rt_cnt[lb_node]) == len(a.rt_targets)
    drop = size - (need - 1)
    a.rt_targets = np.ascontiguousarray(a.rt_targets[:len(a.rt_targets) - drop])
    a.rt_cnt[lb_node] -= drop
    a.as_params[node, 8] = need - 1
    if a.lb_weights is not None:
        a.lb_weights = np.ascontiguousarray(a.lb_weights[:len(a.rt_targets)])
    a.lb_healthy = np.ascontiguousarray(a.lb_healthy[:len(a.rt_targets)])
    end_ns, start_ns, sched, _cancelled = sim._general_prepare(g, False)
    with GraphEngine(a, seed=spec["seed"], start_ns=start_ns) as eng:
        for entry in sched:
            eng.schedule(*entry)
        with pytest.raises(N.EngineError) as err:
            eng.run_until(end_ns)
    assert err.value.code == N.HS_E_OVERFLOW and f"needs instance {need}" in str(err.value) and f"AutoScaler node {node}" in str(err.value), str(err.value)


def test_object_state_after_a_run():
    """What run() leaves on the user's objects."""
    spec = AS.FIXTURES["fresh_id_after_a_scale_in"]
    sim, pools = _run(spec)
    sc, lb_ = pools["scaler"][0], pools["lb"][0]
    assert isinstance(sc.stats, hs.AutoScalerStats) and sc.stats.scale_out_count > 0 and sc.stats.scale_in_count > 0
    assert all(isinstance(ev, hs.ScalingEvent) and ev.action in ("scale_out", "scale_in") for ev in sc.scaling_history)
    assert [ev.reason for ev in sc.scaling_history if ev.action == "scale_out"][0].startswith("Added ")
    assert lb_.all_backends == pools["server"] + sc._managed_servers and sc.current_count == len(lb_.all_backends)
    assert sc.downstream_entities() == [lb_] + sc._managed_servers
    made = pools["factory"][0].made
    removed = [s for s in made[:sc._next_instance_id] if s not in sc._managed_servers]
    assert removed and all(lb_.get_backend_info(s) is None for s in removed) and all(s.stats_accepted > 0 for s in removed)
    untouched = made[sc._next_instance_id:]
    assert untouched and all(s.stats_accepted == 0 and s._requests_completed == 0 for s in untouched)
    assert set(sim.summary.entities) == {e.name for e in sim._entities}     # a pool instance appears in no summary
