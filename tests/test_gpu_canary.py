"""GPU: a CanaryDeployer over a LoadBalancer on the single-heap loop (csrc/hs_graph.hip, the deployer instantiation of graph_loop)
against the recorded live reference (tests/golden/live_canary/, written by tests/golden/make_golden_canary.py).  Every comparison is
exact equality: Sink records, every per-entity statistic of every family's result reader, all by_kind slices (rows 47 .. 52: the canary
deployer's six Events), every CanaryDeployerStats field, the CanaryState (canary_traffic_pct as a binary64), `canary`,
`_baseline_backends`, `_stage_start_time`, the LoadBalancer's members in order with their total_requests, the strategy's weights and
current weights -- behind every window of the windowed fixtures -- and the canary's own Server statistics.  No case is skipped or
excluded (test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import canary_specs as CS
import family_checks as FC
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine

pytestmark = pytest.mark.gpu
CR = CS.CANARY


def _equals_the_recording(spec, sim, pools, ref):
    got = CS.results(spec, sim, pools)
    CS.compare(spec["name"], got, ref)
    assert len(ref["by_kind"]) == CS.N_KINDS and "cn_state" in ref and "cn_weights" in ref and "cn_traffic_pct" in ref
    return got


def _run(spec, **kw):
    sim, pools = CS.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "CanaryDeployer" in sim._station_refusal
    return sim, pools


def test_every_recorded_case_is_compared():
    names = [s["name"] for s in CS.all_specs()]
    assert len(names) == len(set(names)) == len(CS.FIXTURES) + CS.N_RANDOM and CS.N_RANDOM >= 100
    for spec in CS.all_specs():
        ref = CR.get("case", spec)
        assert ref["total_events"] <= 20_000 and ref["python"][:2] < [3, 12]
    assert 3 * len(CS.TRACED) >= len(CS.FIXTURES)
    for name in CS.TRACED:
        assert len(CR.get("case", CS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(CS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = CS.FIXTURES[name]
    if spec.get("windows"):
        sim, pools = CS.engine_run(spec, list(spec["windows"]) + [None])      # the reference ran it in these windows
    else:
        sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, CR.get("case", spec))


@pytest.mark.parametrize("k", range(CS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = CS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, CR.get("case", spec))


@pytest.mark.parametrize("name", CS.TRACED)
def test_record_order_follows_the_trace(name):
    """Every Sink event in the one processing order of the whole graph, and the engine's count of every kind equals the trace's."""
    spec = CS.FIXTURES[name]
    trace = CR.get("case", spec)["trace"]
    sim, pools, g, eng, end_ns, _start, _c = CS.engine(spec)
    a = g.arrays
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        events = eng.canary_events()
    count = lambda first, n: [int((trace[:, 1] == first + k).sum()) for k in range(n)]  # noqa: E731
    assert by_kind == count(0, N.EV_KINDS) and events.tolist() == count(CS.EV_CN_FIRST, N.CANARY_KINDS) and events[0] > 0
    assert set(trace[trace[:, 1] >= CS.EV_CN_FIRST][:, 2].tolist()) == {g.node_of[id(d)] for d in pools["canary"]}
    want = FC.live_rows(trace, kinds=(N.EV_NAMES.index("sink"), N.EV_NAMES.index("probe")))
    kept = (a.kind[node] == N.NODE_SINK) | (a.kind[node] == N.NODE_PROBE)
    assert np.array_equal(np.stack([t[kept], node[kept]], axis=1), want[:, [0, 2]])


_WINDOWED = sorted(n for n, s in CS.FIXTURES.items() if s.get("windows"))


@pytest.mark.parametrize("name", _WINDOWED)
def test_object_state_and_weights_after_every_window(name):
    """Behind EVERY window: the deployer's statistics and state, its LoadBalancer's members and the strategy's weights as the reference's
    objects held them behind the same window."""
    spec = CS.FIXTURES[name]
    ref = CR.get("case", spec)
    ends = list(spec["windows"]) + [None]
    assert len(_WINDOWED) >= 3 and CS.WINDOW_KEYS <= set(ref) and len(ref["window_cn_state"]) == len(ends)
    sim, pools, g, eng, end_ns, start_ns, cancelled = CS.engine(spec)
    with eng:
        for k, t in enumerate(ends):
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
            got = CS.canary_state(pools)
            assert got["cn_state"].tolist() == ref["window_cn_state"][k].tolist(), (name, k)
            assert got["cn_traffic_pct"].tobytes() == np.asarray(ref["window_cn_traffic_pct"][k]).tobytes(), (name, k)
            assert got["cn_members"] == ref["window_cn_members"][k] and got["cn_weights"] == ref["window_cn_weights"][k], (name, k)
    _equals_the_recording(spec, sim, pools, ref)


@pytest.mark.parametrize("name", ["quick_stages_to_promotion_wrr", "sixty_six_baselines_promoted"])
def test_growth_from_capacity_one(name):
    spec = CS.FIXTURES[name]
    ref = CR.get("case", spec)
    for side_by_side in (False, True):
        sim, pools, g, eng, end_ns, _start, cancelled = CS.engine(spec, heap_capacity=1, request_capacity=1, record_capacity=1)
        with eng:
            if side_by_side:
                GraphEngine.run_many([eng], end_ns)
            else:
                eng.run_until(end_ns)
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, ref)


def test_the_promotion_is_the_same_on_either_compaction_path():
    """66 baselines leave in ONE compaction: on the lone lane, by all 64 lanes, and by default (64 lanes from 32 members on)."""
    spec = CS.FIXTURES["sixty_six_baselines_promoted"]
    ref = CR.get("case", spec)
    counts = {}
    for flags in (N.GRAPH_DEBUG_LANE_SERIAL, N.GRAPH_DEBUG_COOPERATIVE, 0):
        sim, pools, g, eng, end_ns, _start, cancelled = CS.engine(spec)
        with eng:
            eng.set_debug_flags(flags)
            eng.run_until(end_ns)
            counts[flags] = eng.deployer_compactions()
            sim._general_finish(g, eng, end_ns, cancelled, 0.0)
        _equals_the_recording(spec, sim, pools, ref)
    assert counts[N.GRAPH_DEBUG_LANE_SERIAL] == (1, 0) and counts[N.GRAPH_DEBUG_COOPERATIVE] == (0, 1) and counts[0] == (0, 1)


def test_16_groups_as_parts_equal_the_recording():
    spec = CS.groups_spec(16)
    sim, pools = _run(spec)
    assert sim._graph_parts > 1
    got = _equals_the_recording(spec, sim, pools, CR.get("case", spec))
    assert got["cn_state"][:, 0].sum() == 16


def test_8_replicas_equal_single_runs():
    spec = dict(CS.FIXTURES["quick_stages_to_promotion_wlc"], end_s=4.0)
    built = []

    def build_fn():
        built.append(CS.build(spec))
        return built[-1][0]

    hs.ParallelRunner().run_replicas(build_fn, 8, base_seed=900)
    for i, (sim, pools) in enumerate(built[:4]):
        one_sim, one_pools = _run(spec, seed=900 + i)
        got, one = CS.results(spec, sim, pools), CS.results(spec, one_sim, one_pools)
        for key in one:
            assert (got[key] == one[key]) if isinstance(one[key], list) else np.array_equal(np.asarray(got[key]), np.asarray(one[key])), (i, key)


def test_object_state_after_a_run():
    spec = CS.FIXTURES["quick_stages_to_promotion_wrr"]
    sim, pools = _run(spec)
    cn, lb_ = pools["canary"][0], pools["lb"][0]
    assert isinstance(cn.stats, hs.CanaryDeployerStats) and isinstance(cn.state, hs.CanaryState) and cn.state.status == "completed"
    assert cn.canary is pools["factory"][0].made[0] and lb_.all_backends == [cn.canary] and cn._baseline_backends == pools["server"]
    assert all(lb_.get_backend_info(s) is None for s in pools["server"]) and cn.state.canary_traffic_pct == 1.0
    assert lb_.strategy._weights == {s.name: 1 for s in pools["server"] + [cn.canary]}
    assert cn.downstream_entities() == [lb_, cn.canary] + pools["server"]
