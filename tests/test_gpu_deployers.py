"""GPU: a RollingDeployer over a LoadBalancer on the single-heap loop (csrc/hs_graph.hip, the deployer instantiation of graph_loop)
against the recorded live reference (tests/golden/live_deployers/, written by tests/golden/make_golden_deployers.py).  Every comparison
is exact equality: Sink records, every per-entity statistic of every family's result reader, all by_kind slices (rows 40 .. 46: the
deployer's seven Events), every RollingDeployerStats field, the DeploymentState, `_next_instance_id`, `_health_fail_count`,
`_health_pass_count`, the four backend lists, the LoadBalancer's members IN ORDER with their total_requests and weights,
`get_backend_info` of a removed backend, the strategy's weights and current weights, and the Server statistics of every instance the
run activated.  No case is skipped or excluded (test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import deployer_specs as DS
import family_checks as FC
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
DR = DS.DEPLOYERS


def _equals_the_recording(spec, sim, pools, ref):
    got = DS.results(spec, sim, pools)
    DS.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == DS.N_KINDS and "rd_state" in ref and "rd_members" in ref and "rd_instance_stats" in ref
    return got


def _run(spec, **kw):
    sim, pools = DS.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "RollingDeployer" in sim._station_refusal
    return sim, pools


def _one_heap(spec):
    import happy_simulator_amd.simulation as S

    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        return _run(spec)
    finally:
        S.MAX_PARTS = old


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of deployer_specs, and every one has a recording."""
    names = [s["name"] for s in DS.all_specs()]
    assert len(names) == len(set(names)) == len(DS.FIXTURES) + DS.N_RANDOM and DS.N_RANDOM >= 100 and len(DS.FIXTURES) >= 30
    for spec in DS.all_specs():
        ref = DR.get("case", spec)
        assert ref["total_events"] <= 20_000 and ref["by_kind"][DS.EV_RD_FIRST] > 0
    assert 3 * len(DS.TRACED) >= len(DS.FIXTURES)
    for name in DS.TRACED:
        assert len(DR.get("case", DS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(DS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = DS.FIXTURES[name]
    if spec.get("windows"):
        sim, pools = DS.engine_run(spec, list(spec["windows"]) + [None])      # the reference ran it in these windows
    else:
        sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, DR.get("case", spec))


@pytest.mark.parametrize("k", range(DS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = DS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, DR.get("case", spec))


@pytest.mark.parametrize("name", DS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event in
    the one processing order of the whole graph -- at the node numbers the pool's instances were lowered to --, and the engine's count
    of every kind equals the trace's."""
    spec = DS.FIXTURES[name]
    ref = DR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = DS.engine(spec)
    a = g.arrays
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        events = eng.deployer_events()
    count = lambda first, n: [int((trace[:, 1] == first + k).sum()) for k in range(n)]  # noqa: E731
    assert by_kind == count(0, N.EV_KINDS) and internal.tolist() == count(N.EV_KINDS, 4)
    assert events.tolist() == count(DS.EV_RD_FIRST, N.DEPLOYER_KINDS) and events[0] > 0
    # the deployer rows of the trace name the node the product lowered the deployer to; instance rows lie behind the Simulation's own nodes
    assert set(trace[trace[:, 1] >= DS.EV_RD_FIRST][:, 2].tolist()) == {g.node_of[id(d)] for d in pools["deployer"]}
    assert trace[:, 2].max() < a.n and (trace[:, 2] >= g.n_own).any() == bool(ref["rd_state"][:, 12].any())
    want = FC.live_rows(trace, kinds=(N.EV_NAMES.index("sink"), N.EV_NAMES.index("probe")))
    kept = (a.kind[node] == N.NODE_SINK) | (a.kind[node] == N.NODE_PROBE)
    assert np.array_equal(np.stack([t[kept], node[kept]], axis=1), want[:, [0, 2]])


# window ends ON the deployer's nanoseconds, among uneven ones
_WINDOWS = {"batch_1_threshold_1_completes": [0.5, 1.0, 1.7000001], "default_settings_batch_2_rolls_back": [1.0, 1.0, 1.5, 2.0],
            "rollback_with_a_pass_in_flight_walks_on_to_completed": [1.5, 1.5, 2.0], "second_deploy_inside_the_first": [1.25, 1.5],
            "crashed_deployer": [1.1, 1.5, 2.7], "wlc_two_deploys": [1.0, 2.75], "two_deployed_load_balancers": [1.9],
            "removed_initial_backend_finishes_its_queue": [0.75, 0.9]}


@pytest.mark.parametrize("name", sorted(_WINDOWS))
def test_windows_equal_one_run(name):
    spec = DS.FIXTURES[name]
    sim, pools = DS.engine_run(spec, _WINDOWS[name] + [None])
    _equals_the_recording(spec, sim, pools, DR.get("case", spec))


@pytest.mark.parametrize("name", ["batch_2_threshold_1", "slow_interval_health_checks_multiply", "wrr_two_deploys", "sixty_six_members_one_batch"])
def test_growth_from_capacity_one(name):
    """Heap, Request and record capacity 1: every buffer grows across relaunches -- a health check over a whole batch waits in front
    of the pop until the heap and the Requests have room for all its probes and timeouts."""
    spec = DS.FIXTURES[name]
    ref = DR.get("case", spec)
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = DS.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, ref)


_WINDOWED = sorted(n for n, s in DS.FIXTURES.items() if s.get("windows"))


@pytest.mark.parametrize("name", _WINDOWED)
def test_object_state_after_every_window(name):
    """The results are bound behind EVERY window of a windowed run: each deployer's statistics, state, lists and its LoadBalancer's
    members equal what the reference's objects held behind the same window."""
    spec = DS.FIXTURES[name]
    ref = DR.get("case", spec)
    ends = list(spec["windows"]) + [None]
    assert len(_WINDOWED) >= 3 and DS.WINDOW_KEYS <= set(ref) and len(ref["window_rd_state"]) == len(ends)
    sim, pools, g, eng, end_ns, start_ns, cancelled = DS.engine(spec)
    with eng:
        for k, t in enumerate(ends):
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
            got = DS.deployer_state(pools)
            assert got["rd_state"].tolist() == ref["window_rd_state"][k].tolist(), (name, k)
            assert got["rd_members"] == ref["window_rd_members"][k], (name, k)
            assert got["rd_lists"] == ref["window_rd_lists"][k], (name, k)
    _equals_the_recording(spec, sim, pools, ref)


def test_32_replicas_equal_32_single_runs():
    base, other = DS.FIXTURES["wrr_two_deploys"], DS.FIXTURES["default_settings_batch_2_rolls_back"]
    specs = [dict(base if i % 2 == 0 else other, end_s=3.0) for i in range(32)]
    built = []

    def build_fn():
        sim, pools = DS.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 32, base_seed=1700)
    assert len(results) == 32
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph)
        got = DS.results(specs[i], sim, pools)
        if i < 8:
            one_sim, one_pools = _run(specs[i], seed=1700 + i)
            one = DS.results(specs[i], one_sim, one_pools)
            assert set(got) == set(one)
            for key in one:
                assert (got[key] == one[key]) if isinstance(one[key], list) else np.array_equal(np.asarray(got[key]), np.asarray(one[key])), (i, key)
        seen.add((got["total_events"], tuple(got["sink_t_ns"][:50].tolist())))
    assert len(seen) > 24


def test_16_groups_as_parts_equal_one_heap_and_the_recording():
    """16 disconnected deployed chains in ONE Simulation: the parts run side by side (hs_graph_run_parts), every pool in the part of its
    LoadBalancer, and leave what one heap over all of them leaves, which is what the reference's one heap left."""
    spec = DS.groups_spec(16)
    ref = DR.get("case", spec)
    sim, pools = _run(spec)
    one_sim, one_pools = _one_heap(spec)
    assert one_sim._graph_parts == 1 and sim._graph_parts > 1
    got = _equals_the_recording(spec, sim, pools, ref)
    _equals_the_recording(spec, one_sim, one_pools, ref)
    assert got["rd_state"][:, 3].sum() >= 16


def test_a_batch_that_mixes_deployed_and_other_graphs():
    """hs_graph_run_many over two deployed graphs, a health-checked one and a plain mixed one: the whole batch runs the deployer
    instantiation, and every handle leaves what it leaves alone."""
    import mixed_specs as MX

    deployed = [DS.FIXTURES["least_conn_two_deploys"], DS.FIXTURES["crashed_deployer"]]
    others = [dict(MX.FIXTURES["gate_into_a_checked_load_balancer_wrr"], end_s=8.0), dict(MX.FIXTURES["client_server_batch_processor"], end_s=8.0)]
    made = [DS.engine(s) for s in deployed] + [FC.engine(s) for s in others]
    assert len({m[4] for m in made}) == 1
    try:
        GraphEngine.run_many([m[3] for m in made], made[0][4])
        for m in made:
            m[0]._general_finish(m[2], m[3], m[4], m[6], 0.0)
    finally:
        for m in made:
            m[3].close()
    for spec, m in zip(deployed, made):
        _equals_the_recording(spec, m[0], m[1], DR.get("case", spec))
    for spec, m in zip(others, made[2:]):
        one_sim, one_pools = MX.build(spec)
        one_sim.run()
        FC.same(MX.results(spec, m[0], m[1]), MX.results(spec, one_sim, one_pools), spec["name"])


@pytest.mark.parametrize("name", ["batch_1_threshold_1_completes", "batch_2_threshold_1", "batch_equal_to_the_backend_count"])
def test_a_pool_one_instance_too_small_ends_the_run_with_an_error(name):
    """The engine-level hook: the same graph with the last pool instance taken off the LoadBalancer's targets and the pool's size one
    below what the run needs.  The run returns HS_E_OVERFLOW with a message that names the deployer and the first instance the pool
    lacks -- also where a batch of several asks for it (batch_size 2 and 3) -- it never goes on silently."""
    spec = DS.FIXTURES[name]
    need = int(DR.get("case", spec)["rd_state"][0, 12])    # instances the run creates
    sim, pools = DS.build(spec)
    g = sim.lowered()
    a = g.arrays
    node = g.node_of[id(pools["deployer"][0])]
    lb_node = int(a.target[node])
    size = int(a.rd_params[node, 4])
    assert size == need > 1 and int(a.rt_off[lb_node]) + int(a.rt_cnt[lb_node]) == len(a.rt_targets)
    a.rt_targets = np.ascontiguousarray(a.rt_targets[:len(a.rt_targets) - 1])
    a.rt_cnt[lb_node] -= 1
    a.rd_params[node, 4] = need - 1
    if a.lb_weights is not None:
        a.lb_weights = np.ascontiguousarray(a.lb_weights[:len(a.rt_targets)])
    a.lb_healthy = np.ascontiguousarray(a.lb_healthy[:len(a.rt_targets)])
    end_ns, start_ns, sched, _cancelled = sim._general_prepare(g, False)
    with GraphEngine(a, seed=spec["seed"], start_ns=start_ns) as eng:
        for entry in sched:
            eng.schedule(*entry)
        with pytest.raises(N.EngineError) as err:
            eng.run_until(end_ns)
    assert err.value.code == N.HS_E_OVERFLOW and f"needs instance {need}" in str(err.value) and f"RollingDeployer node {node}" in str(err.value), str(err.value)


def test_end_time_infinity_ends_with_the_deployment():
    """The deployer's Events are no daemons: an auto-terminating run goes on until the deployment is over."""
    spec = DS.FIXTURES["end_time_infinity_ends_with_the_deployment"]
    sim, pools = _run(spec)
    assert sim._end_time == hs.Instant.Infinity and pools["deployer"][0].state.status == "completed"
    _equals_the_recording(spec, sim, pools, DR.get("case", spec))


def test_object_state_after_a_run():
    """What run() leaves on the user's objects."""
    spec = DS.FIXTURES["default_settings_batch_2_rolls_back"]
    sim, pools = _run(spec)
    dp, lb_ = pools["deployer"][0], pools["lb"][0]
    assert isinstance(dp.stats, hs.RollingDeployerStats) and isinstance(dp.state, hs.DeploymentState) and dp.stats.deployments_rolled_back == 1
    made = pools["factory"][0].made
    assert [b.name for b in lb_.all_backends] == ["srv2", "rd0_v2_3"] and lb_.all_backends[1] is made[2]
    removed = [s for s in pools["server"] + made[:dp._next_instance_id] if s not in lb_.all_backends]
    assert len(removed) == 4 and all(lb_.get_backend_info(s) is None for s in removed) and all(s.stats_accepted > 0 for s in removed)
    assert dp.downstream_entities() == [lb_] + dp._old_backends + dp._new_backends
    assert set(dp._health_pass_count) <= {s.name for s in made} and dp._next_instance_id == 3
    assert set(sim.summary.entities) == {e.name for e in sim._entities}     # a pool instance appears in no summary


# ---- the compaction of the member list behind a removal: the lone lane and all 64 lanes
def _removals(n):
    """Which members leave: the first, the last, every other one, a whole 64-entry chunk, everything, nothing."""
    keep = np.ones(n, bool)
    out = {}
    for name, gone in (("first", [0]), ("last", [n - 1]), ("every_other", range(0, n, 2)), ("the_other_half", range(1, n, 2)),
                       ("first_chunk", range(0, min(64, n))), ("last_chunk", range(max(0, n - 64), n)), ("second_chunk", range(64, min(128, n))),
                       ("everything", range(n)), ("nothing", [])):
        k = keep.copy()
        k[list(gone)] = False
        out[name] = k
    return out


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_both_compactions_leave_the_same_list(n):
    """Member lists at and around the chunk boundaries, in an order that is no slot order: every removal pattern leaves, on either
    path, the members that stay in the order they had."""
    rng = np.random.default_rng(n)
    n_slots = n + 7
    members = rng.permutation(n_slots)[:n]                                 # insertion order, not slot order
    for name, keep in _removals(n).items():
        flags = np.zeros(n_slots, np.uint8)
        flags[members[keep]] = 1
        want = members[keep].tolist()
        lone = GraphEngine.compact_members(members, flags, wave=False)
        wave = GraphEngine.compact_members(members, flags, wave=True)
        assert lone == want, (n, name, "lone lane")
        assert wave == want, (n, name, "64 lanes")


@pytest.mark.parametrize("name", ["sixty_six_members_one_batch", "rollback_with_a_pass_in_flight_walks_on_to_completed", "wrr_two_deploys"])
def test_a_run_is_the_same_on_either_compaction_path(name):
    """hs_debug_graph_flags bit 0 keeps every compaction on the lone lane, bit 1 hands every one to the wavefront: the run leaves what the
    reference left either way, and the counters say which path ran.  By default a list of 66 members goes to the 64 lanes, one of
    a few members stays on the lone lane."""
    spec = DS.FIXTURES[name]
    ref = DR.get("case", spec)
    counts = {}
    for flags in (N.GRAPH_DEBUG_LANE_SERIAL, N.GRAPH_DEBUG_COOPERATIVE, 0):
        sim, pools, g, eng, end_ns, _start, cancelled = DS.engine(spec)
        with eng:
            eng.set_debug_flags(flags)
            eng.run_until(end_ns)
            counts[flags] = eng.deployer_compactions()
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, ref)
    lone, wave = counts[N.GRAPH_DEBUG_LANE_SERIAL], counts[N.GRAPH_DEBUG_COOPERATIVE]
    assert lone[0] > 0 and lone[1] == 0 and wave[1] > 0 and sum(wave) == sum(lone)
    assert counts[0] == (wave if name == "sixty_six_members_one_batch" else lone)
