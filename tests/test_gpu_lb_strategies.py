"""GPU: the WeightedRoundRobin / IPHash / LeastConnections / WeightedLeastConnections strategies against the LIVE reference as
recorded (tests/golden/live_strategies/, tests/golden/make_golden_strategies.py), through `hs.Simulation` and through the C ABI.
Every comparison is exact equality -- integers, int64-ns timestamps, binary64 sums; no tolerance anywhere.

  * every named fixture and every recorded random case equals the reference on everything recorded;
  * the pipeline (csrc/hs_lb.hip) and the single-heap loop (csrc/hs_graph.hip) agree on WeightedRoundRobin and IPHash;
  * at the benchmarked size WeightedRoundRobin with unit weights IS RoundRobin, and with skewed weights the per-backend counts are
    the selection table's;
  * the wave-cooperative least-loaded selection equals the lane-serial one at 8 .. 4 096 backends;
  * replicas, parts and windows leave what single runs / one heap / one run leave.
"""
import hashlib

import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import helpers as H
import strategy_specs as SS
from happy_simulator_amd import _native as N
from happy_simulator_amd import lowering as L
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine
from happy_simulator_amd.lb_engine import LbBackendArrays, LbSourceArrays, LoadBalancerEngine
from recorded import STRATEGIES as SR

pytestmark = pytest.mark.gpu

# everything recorded is compared but the trace (the fixtures' processing order: test_lb_strategies_host.py reads it)
_NOT_COMPARED = {"trace"}
_BY_KIND_SLICES = [("by_kind", N.EV_KINDS)]


def _equals_the_recording(spec, sim, ents, what=None):
    FC.compare(what or spec["name"], SS.results(spec, sim, ents), SR.get("case", spec), _NOT_COMPARED, _BY_KIND_SLICES)


def _run_and_compare(spec):
    sim, ents = SS.build(spec)
    sim.run()
    _equals_the_recording(spec, sim, ents)
    return sim, ents


@pytest.mark.parametrize("name", sorted(SS.FIXTURES))
def test_named_fixtures_equal_the_live_reference(name):
    spec = SS.FIXTURES[name]
    sim, ents = _run_and_compare(spec)
    kinds = {lb["strategy"] for lb in spec["lbs"]}
    if kinds & {"least_conn", "wlc"}:
        assert isinstance(sim.lowered(), GeneralGraph)
        assert len(spec["lbs"]) > 1 or "feedback" in sim._station_refusal      # (ONE such LoadBalancer: the pipeline names its reason)
    if name in ("wrr_poisson", "ip_hash_poisson", "wrr_2048_backends"):
        assert isinstance(sim.lowered(), L.LbGraph)                    # the pipeline's shape ...
        sim2, ents2 = SS.build(spec)                                   # ... and the same fixture on the single-heap loop
        SS.force_single_heap(sim2, spec).run()
        _equals_the_recording(spec, sim2, ents2, name + " (single heap)")
    for lb, lbs in zip(ents["lbs"], spec["lbs"]):
        if lbs["strategy"] == "wrr":
            assert lb.strategy._selections == lb.stats.requests_forwarded
            table = hs.WeightedRoundRobin.selection_table(lbs["weights"])
            np.testing.assert_array_equal([lb.get_backend_info(b).total_requests for b in lb.all_backends],
                                          np.bincount(table[np.arange(lb.stats.requests_forwarded) % len(table)], minlength=len(lbs["weights"])))


@pytest.mark.parametrize("block", range(10))
def test_recorded_random_cases_equal_the_live_reference(block):
    """150 seeded cases (strategy_specs.random_spec): pipeline shapes and general graphs.  None may be left out: a recorded case the
    engine refuses is a failure."""
    paths = set()
    for k in range(block * 15, block * 15 + 15):
        spec = SS.random_spec(k)
        sim, _ents = _run_and_compare(spec)
        paths.add(type(sim.lowered()).__name__)
    assert "GeneralGraph" in paths


@pytest.mark.parametrize("k", range(0, 150, 3))
def test_pipeline_shapes_agree_on_both_paths(k):
    """The pipeline-shaped random cases once more, forced onto the single-heap loop (the WeightedRoundRobin and IPHash ones ran on
    the pipeline above): two independent code paths, one recorded answer."""
    spec = SS.random_spec(k)
    sim, ents = SS.build(spec)
    took_pipeline = isinstance(sim.lowered(), L.LbGraph)
    assert took_pipeline == (spec["lbs"][0]["strategy"] in ("wrr", "ip_hash")), spec["name"]
    sim2, ents2 = SS.build(spec)
    SS.force_single_heap(sim2, spec).run()
    _equals_the_recording(spec, sim2, ents2, spec["name"] + " (single heap)")


@pytest.mark.parametrize("strategy", ["wrr", "ip_hash"])
def test_pipeline_and_single_heap_agree_at_2048_by_2048(strategy):
    """2 048 Sources x 2 048 backends x 4 s: the pipeline's ranking / table gather and the loop's per-event lookup, array for array."""
    S = B = 2048
    rng = np.random.default_rng(5)
    servers = [dict(mean=0.2, c=int(rng.choice([1, 2])), cap=None if j % 3 else 2, out=["sink", 0]) for j in range(B)]
    lb = dict(strategy=strategy, vnodes=1, backends=list(range(B)))
    if strategy == "wrr":
        lb["weights"] = [int(w) for w in rng.choice([1, 1, 2, 3, 8], size=B)]
    sources = [dict(kind="poisson", rate=1.5, to=["lb", 0], **({"n_clients": 100_000} if strategy == "ip_hash" else {})) for _ in range(S)]
    spec = dict(name=f"both_paths_{strategy}", topology="graph", n_sinks=1, servers=servers, links=[], routers=[], lbs=[lb],
                sources=sources, end_s=4.0, seed=77, server_stream_offset=S)
    sim, ents = SS.build(spec)
    assert isinstance(sim.lowered(), L.LbGraph)
    sim.run()
    sim2, ents2 = SS.build(spec)
    SS.force_single_heap(sim2, spec).run()
    a, b = SS.results(spec, sim, ents), SS.results(spec, sim2, ents2)
    assert a["total_events"] > 100_000
    FC.same(a, b, spec["name"])


def _pipeline_run(strategy, weights=None, S=32768, B=32768, rate=6.0, end_s=60.0, seed=42):
    end_ns = int(end_s * 1_000_000_000)
    src = LbSourceArrays(n=S, src_rate=np.full(S, rate), n_clients=np.full(S, 1, np.int64), src_kind=np.full(S, N.SRC_POISSON, np.uint8))
    be = LbBackendArrays(n=B, names=[f"srv{j}" for j in range(B)], concurrency=np.full(B, 1, np.int32),
                         svc_kind=np.full(B, N.LAT_EXPONENTIAL, np.uint8), svc_mean_s=np.full(B, 0.1))
    with LoadBalancerEngine(src, be, virtual_nodes=1, horizon_ns=end_ns, shared_sink=True, seed=seed, strategy=strategy) as eng:
        if weights is not None:
            eng.set_weights(weights)
        eng.run(end_ns)
        s, st = eng.summary(), eng.stats()
        t, cr = eng.read_sink(0)
        digest = hashlib.sha256(np.ascontiguousarray(t).tobytes() + np.ascontiguousarray(cr).tobytes()).hexdigest()
        out = dict(events=s.events_processed, final_ns=s.final_time_ns, by_kind=np.array(list(s.events_by_kind)), sink_records=s.sink_records,
                   digest=digest, latency=eng.latency_stats(), **st)
    return out


def test_unit_weights_are_round_robin_at_the_benchmarked_size():
    """32 768 -> 32 768 x 60 s: WeightedRoundRobin with every weight 1 -- explicitly set, and left at the default -- equals the
    RoundRobin run bit for bit on every statistic and the Sink digest."""
    rr = _pipeline_run(N.LB_ROUND_ROBIN)
    assert rr["events"] > 100_000_000
    for weights in (np.ones(32768, np.int32), None):
        w = _pipeline_run(N.LB_WEIGHTED_ROUND_ROBIN, weights)
        assert (w["events"], w["final_ns"], w["sink_records"], w["digest"], w["latency"]) == (
            rr["events"], rr["final_ns"], rr["sink_records"], rr["digest"], rr["latency"])
        for k in ("by_kind", "generated", "lb", "total_requests", "accepted", "dropped", "completed", "rejected", "total_service_s",
                  "queue_depth", "active", "sink_received"):
            np.testing.assert_array_equal(w[k], rr[k], err_msg=k)


def test_skewed_weights_at_the_benchmarked_size_follow_the_table():
    B = 32768
    weights = (1 + 3 * (np.arange(B) % 4 == 0) + (np.arange(B) % 1000 == 7)).astype(np.int32)
    w = _pipeline_run(N.LB_WEIGHTED_ROUND_ROBIN, weights)
    table = hs.WeightedRoundRobin.selection_table(weights)
    forwarded = int(w["lb"][1])
    assert forwarded > 11_000_000 and len(table) == int(weights.sum())
    full, rest = divmod(forwarded, len(table))
    want = full * weights.astype(np.int64) + np.bincount(table[:rest], minlength=B)
    np.testing.assert_array_equal(w["total_requests"], want)
    np.testing.assert_array_equal(w["accepted"], want)                 # unbounded queues: everything forwarded is accepted


def _lc_spec(strategy, B, requests=1500, seed=3):
    rng = np.random.default_rng(B)
    mean, end_s = 0.5, 2.0
    spec = SS._lb_case(f"{strategy}_{B}", strategy, B, SS._poisson(4, requests / end_s / 4), mean=mean, end_s=end_s, seed=seed,
                       c=[int(c) for c in rng.choice([1, 2, 3], size=B)],
                       weights=[int(w) for w in rng.choice([1, 2, 3, 5], size=B)] if strategy == "wlc" else None)
    return spec


def _abi_run(spec, flags):
    sim, _ents = SS.build(spec)
    g = SS.lower_single_heap(sim, spec)
    with GraphEngine(g.arrays, seed=spec["seed"]) as eng:
        eng.set_debug_flags(flags)
        eng.run_until(H.ns_from_seconds(spec["end_s"]))
        s = eng.summary()
        return dict(events=s.events_processed, final_ns=s.final_time_ns, by_kind=list(s.events_by_kind), stats=eng.stats(),
                    records=eng.records(), coop=eng.coop_selects(), graph=g)


@pytest.mark.parametrize("strategy", ["least_conn", "wlc"])
@pytest.mark.parametrize("B", [8, 64, 512, 4096])
def test_cooperative_selection_equals_the_lane_serial_one(strategy, B):
    """hs_graph_coop_selects() > 0: all 64 lanes scanned the backends; forced onto the lone lane the run leaves the same bits."""
    spec = _lc_spec(strategy, B)
    serial = _abi_run(spec, N.GRAPH_DEBUG_LANE_SERIAL)
    coop = _abi_run(spec, N.GRAPH_DEBUG_COOPERATIVE)
    default = _abi_run(spec, 0)
    forwarded = int(serial["stats"]["lb"][:, 1].sum())
    assert serial["coop"] == 0 and coop["coop"] == forwarded > 1000
    assert default["coop"] == (forwarded if B >= N.GRAPH_COOP_MIN_BACKENDS else 0)
    for other in (coop, default):
        assert (other["events"], other["final_ns"], other["by_kind"]) == (serial["events"], serial["final_ns"], serial["by_kind"])
        for k in serial["stats"]:
            np.testing.assert_array_equal(other["stats"][k], serial["stats"][k], err_msg=k)
        for a, b in zip(other["records"], serial["records"]):
            np.testing.assert_array_equal(a, b)
    assert serial["stats"]["rt_taken"].sum() == forwarded


@pytest.mark.parametrize("strategy", ["least_conn", "wlc"])
def test_cooperative_selection_with_every_backend_busy(strategy):
    """4 096 backends, 5 000 Requests in one second, services of 5 s on average: after the first sweep every backend has Requests in
    service, so the minimum wanders over ALL slots -- the strided tail `lane + 64 k` has to win where it should, not only never win
    wrongly.  Cooperative against lane-serial, every output."""
    B = 4096
    rng = np.random.default_rng(41)
    spec = SS._lb_case(f"{strategy}_busy", strategy, B, SS._poisson(4, 1250.0), mean=5.0, end_s=1.0, seed=9,
                       c=[int(c) for c in rng.choice([1, 2, 3], size=B)],
                       weights=[int(w) for w in rng.choice([1, 2, 3, 5], size=B)] if strategy == "wlc" else None)
    serial = _abi_run(spec, N.GRAPH_DEBUG_LANE_SERIAL)
    coop = _abi_run(spec, N.GRAPH_DEBUG_COOPERATIVE)
    taken = serial["stats"]["rt_taken"]
    assert taken.sum() > 4500 and (taken > 0).sum() > 0.95 * B and taken[B - 64:].sum() > 0      # the high slots won as well
    assert serial["coop"] == 0 and coop["coop"] == taken.sum()
    assert (coop["events"], coop["final_ns"], coop["by_kind"]) == (serial["events"], serial["final_ns"], serial["by_kind"])
    for k in serial["stats"]:
        np.testing.assert_array_equal(coop["stats"][k], serial["stats"][k], err_msg=k)
    for a, b in zip(coop["records"], serial["records"]):
        np.testing.assert_array_equal(a, b)


def test_one_heavy_backend_leaves_the_row_layout_and_follows_the_table():
    """32 768 -> 32 768 x 60 s with ONE backend of weight 64 (its share is 64 mean shares, far beyond the three the `[k][backend]`
    rows are sized for): the run falls back to the dense layout (hs_lb_layout) and every per-backend count is still the table's."""
    B = 32768
    weights = np.ones(B, np.int32)
    weights[12345] = 64
    weights[::512] = 2
    w = _pipeline_run(N.LB_WEIGHTED_ROUND_ROBIN, weights)
    table = hs.WeightedRoundRobin.selection_table(weights)
    forwarded = int(w["lb"][1])
    full, rest = divmod(forwarded, len(table))
    want = full * weights.astype(np.int64) + np.bincount(table[:rest], minlength=B)
    assert want.max() > 3 * forwarded / B + 64                         # (beyond the allocated rows)
    np.testing.assert_array_equal(w["total_requests"], want)
    np.testing.assert_array_equal(w["accepted"], want)
    assert int(w["completed"].sum()) == w["sink_records"] > 10_000_000


@pytest.mark.parametrize("name", ["lc_8_backends", "lc_64_backends", "wlc_8_backends", "wlc_64_backends", "wlc_score_ties", "lc_lockstep_constant"])
@pytest.mark.parametrize("flags", [N.GRAPH_DEBUG_LANE_SERIAL, N.GRAPH_DEBUG_COOPERATIVE])
def test_both_selection_paths_equal_the_recorded_reference(name, flags):
    spec = SS.FIXTURES[name]
    rec = SR.get("case", spec)
    r = _abi_run(spec, flags)
    assert (r["events"], r["final_ns"]) == (rec["total_events"], rec["final_ns"])
    np.testing.assert_array_equal(r["by_kind"], rec["by_kind"])
    np.testing.assert_array_equal(r["stats"]["rt_taken"], rec["lb_backend_total_requests"])
    node, t, _cr = r["records"]
    np.testing.assert_array_equal(np.sort(t, kind="stable"), np.sort(rec["sink_t_ns"], kind="stable"))
    assert (r["coop"] > 0) == (flags == N.GRAPH_DEBUG_COOPERATIVE)


def test_weights_through_the_c_abi():
    """hs_graph_set_lb_weights: out-of-range weights, a wrong node kind and a wrong count come back HS_E_INVALID; after a run
    HS_E_STATE.  hs_lb_set_weights likewise."""
    spec = SS.FIXTURES["wrr_poisson"]
    sim, ents = SS.build(spec)
    g = SS.lower_single_heap(sim, spec)
    lb_node = g.node_of[id(ents["lbs"][0])]
    lib = N.lib()
    with GraphEngine(g.arrays, seed=spec["seed"]) as eng:
        for node, w in ((lb_node, [1, 0, 1, 1]), (lb_node, [1, 1, 1]), (0, [1, 1, 1, 1]), (g.arrays.n, [1, 1, 1, 1])):
            a = np.array(w, np.int32)
            assert lib.hs_graph_set_lb_weights(eng._h, node, a.ctypes.data, len(a)) == N.HS_E_INVALID
        eng.run_until(H.ns_from_seconds(spec["end_s"]))
        rec = SR.get("case", spec)
        np.testing.assert_array_equal(eng.stats()["rt_taken"], rec["lb_backend_total_requests"])     # (the refused calls changed nothing)
        a = np.array([5, 1, 1, 2], np.int32)
        assert lib.hs_graph_set_lb_weights(eng._h, lb_node, a.ctypes.data, 4) == N.HS_E_STATE
    src = LbSourceArrays(n=2, src_rate=np.full(2, 5.0), n_clients=np.ones(2, np.int64))
    be = LbBackendArrays(n=3, names=["a", "b", "c"])
    with LoadBalancerEngine(src, be, virtual_nodes=1, horizon_ns=10**9, strategy=N.LB_WEIGHTED_ROUND_ROBIN) as eng:
        with pytest.raises(N.EngineError, match="weight must be >= 1, got 0"):
            eng.set_weights([1, 0, 2])
        with pytest.raises(N.EngineError, match="2\\^24"):
            eng.set_weights([1 << 23, 1 << 23, 1])
        eng.set_weights([2, 1, 1])
        eng.run(10**9)
        with pytest.raises(N.EngineError, match="before the first run"):
            eng.set_weights([1, 1, 1])
    for code in (N.LB_LEAST_CONNECTIONS, N.LB_WEIGHTED_LEAST_CONNECTIONS):
        with pytest.raises(N.EngineError, match="feedback"):
            LoadBalancerEngine(src, be, virtual_nodes=1, horizon_ns=10**9, strategy=code)


def test_replicas_of_a_least_connections_graph_equal_single_runs():
    """ParallelRunner.run_replicas: 300 replicas side by side (hs_graph_run_many) == 300 Simulations run alone with seeds base + i."""
    spec = SS.FIXTURES["two_lbs_shared_backends"]
    built = []

    def build_fn():
        sim, ents = SS.build(spec)
        built.append((sim, ents))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 300, base_seed=1000)
    assert len(results) == len(built) == 300 and isinstance(built[0][0].lowered(), GeneralGraph)
    totals = set()
    for i, ((sim, ents), res) in enumerate(zip(built, results)):
        alone, ents1 = SS.build(spec, seed=1000 + i)
        alone.run()
        assert res.summary.total_events_processed == alone.summary.total_events_processed
        sim._summary = res.summary
        FC.same(SS.results(spec, sim, ents), SS.results(spec, alone, ents1), f"replica {i}")
        totals.add(res.summary.total_events_processed)
    assert len(totals) > 100


def test_disconnected_least_connections_graphs_run_as_parts(monkeypatch):
    """A union of LeastConnections / WeightedLeastConnections / WeightedRoundRobin graphs that share nothing runs as parts
    (hs_graph_run_parts) and leaves what the one heap leaves."""
    from random_specs import union_spec

    members = [dict(SS.FIXTURES[n]) for n in ("lc_poisson", "wlc_poisson", "lc_conc_bounded", "wrr_poisson", "lc_64_backends")]
    spec = union_spec(members, name="lc_union")
    sim, ents = SS.build(spec)
    sim.run()
    assert sim._graph_parts == len(members)
    import happy_simulator_amd.simulation as simulation_mod

    monkeypatch.setattr(simulation_mod, "split_parts", lambda arrays, max_parts=0: None)
    one, ents1 = SS.build(spec)
    one.run()
    assert one._graph_parts == 1
    FC.same(SS.results(spec, sim, ents), SS.results(spec, one, ents1), "parts against one heap")
    assert sum(lb.stats.requests_forwarded for lb in ents["lbs"]) > 500


@pytest.mark.parametrize("name", ["lc_conc_bounded", "wlc_64_backends"])
def test_windows_over_a_least_connections_graph_equal_one_run(name):
    """`_run_window` = `_execute_until` again: uneven, repeated and earlier window ends on one handle (every buffer grows on the way,
    so selections straddle launches) == one run, and == the recorded reference."""
    spec = SS.FIXTURES[name]
    sim, _ = SS.build(spec)
    g = SS.lower_single_heap(sim, spec)
    end_ns = H.ns_from_seconds(spec["end_s"])
    with GraphEngine(g.arrays, seed=spec["seed"]) as one:
        one.run_until(end_ns)
        s1, st1, rec1 = one.summary(), one.stats(), one.records()
    with GraphEngine(g.arrays, seed=spec["seed"], heap_capacity=1, request_capacity=1, record_capacity=16) as eng:
        for w in (0.05, 0.05, 0.050000001, 0.7, 0.3, 1.25):
            eng.run_until(H.ns_from_seconds(w))
        eng.run_until(end_ns)
        s2, st2, rec2 = eng.summary(), eng.stats(), eng.records()
    assert s1.events_processed == s2.events_processed == SR.get("case", spec)["total_events"] and s1.final_time_ns == s2.final_time_ns
    for k in st1:
        np.testing.assert_array_equal(st1[k], st2[k], err_msg=k)
    for a, b in zip(rec1, rec2):
        np.testing.assert_array_equal(a, b)
