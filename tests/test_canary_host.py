"""Host side of the CanaryDeployer (no GPU): the constructors, defaults and dataclasses, the deploy() Event, the two evaluators in host
Python against the recorded reference over enumerated inputs, every refusal by its message, the lowered arrays and the new symbols of
the C ABI."""
import dataclasses
import os
import re

import numpy as np
import pytest

import canary_specs as CS
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, split_parts
from happy_simulator_amd.lowering import UnsupportedTopology as UT

CR = CS.CANARY


def _fleet(canary_kw=None, strategy=None, n_init=3, end_s=5.0, extra=(), deploys=1, factory=None, **sim_kw):
    sink = hs.Sink("sink")
    servers = [hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink) for i in range(n_init)]
    lb = hs.LoadBalancer("lb", backends=servers, strategy=strategy)
    factory = factory or (lambda name: hs.Server(name, service_time=hs.ExponentialLatency(0.05), downstream=sink))
    cn = hs.CanaryDeployer("can", lb, factory, **(canary_kw or {}))
    src = hs.Source.poisson(rate=20.0, target=lb, name="src")
    sim = hs.Simulation(sources=[src], entities=servers + [lb, sink] + list(extra) + [cn],
                        **({} if end_s is None else {"end_time": hs.Instant.from_seconds(end_s)}), **sim_kw)
    for _ in range(deploys):
        sim.schedule(cn.deploy())
    return sim, dict(sink=sink, servers=servers, lb=lb, canary=cn, src=src)


def test_constructor_defaults_and_dataclasses_are_the_references():
    lb = hs.LoadBalancer("lb")
    cn = hs.CanaryDeployer("c", lb, lambda name: hs.Server(name))
    assert (cn.name, cn.load_balancer, cn._evaluation_interval, cn.canary, cn._baseline_backends, cn._stage_start_time) == ("c", lb, 5.0, None, [], None)
    assert [(s.traffic_percentage, s.evaluation_period) for s in cn._stages] == [(0.01, 30.0), (0.05, 30.0), (0.25, 30.0), (1.0, 30.0)]
    assert cn._stages == hs.CanaryDeployer.DEFAULT_STAGES and cn._stages is not hs.CanaryDeployer.DEFAULT_STAGES
    assert hs.CanaryDeployer("c", lb, None, stages=[])._stages == hs.CanaryDeployer.DEFAULT_STAGES       # `stages or DEFAULT_STAGES`
    ev = cn._metric_evaluator
    assert isinstance(ev, hs.ErrorRateEvaluator) and (ev._max_error_rate, ev._threshold_multiplier) == (0.05, 2.0)
    lat = hs.LatencyEvaluator()
    assert (lat._max_latency, lat._threshold_multiplier) == (1.0, 1.5)
    assert dataclasses.astuple(cn.stats) == (0,) * 7 and [f.name for f in dataclasses.fields(cn.stats)] == [
        "deployments_started", "deployments_completed", "deployments_rolled_back", "stages_completed", "evaluations_performed",
        "evaluations_passed", "evaluations_failed"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        cn.stats.deployments_started = 1
    assert dataclasses.asdict(cn.state) == dict(status="idle", current_stage=0, total_stages=0, canary_traffic_pct=0.0)
    assert hs.CanaryStage(0.5).evaluation_period == 30.0 and cn.downstream_entities() == [lb] and isinstance(cn, hs.Entity)
    assert N.CANARY_STATUS == ("idle", "in_progress", "promoting", "rolled_back", "completed")


def test_the_deploy_event():
    cn = hs.CanaryDeployer("c", hs.LoadBalancer("lb"), lambda name: hs.Server(name))
    ev = cn.deploy()
    assert (ev.time, ev.event_type, ev.target, ev.daemon, ev.on_complete) == (hs.Instant.Epoch, "_canary_deploy_start", cn, False, [])
    sim, o = _fleet(start_time=hs.Instant.from_seconds(2.0), end_s=4.0, deploys=0)
    ev = o["canary"].deploy()
    assert ev.time == hs.Instant.from_seconds(2.0)
    ev.time = hs.Instant.from_seconds(3.0)
    sim.schedule(ev)
    g = sim.lowered()
    assert sim._general_prepare(g, False)[2] == [(g.node_of[id(o["canary"])], 3 * 10 ** 9)]


class _Stats:
    def __init__(self, completed, rejected):
        self.requests_completed, self.requests_rejected = completed, rejected


class _Backend:
    def __init__(self, completed, rejected, latency):
        self.stats, self.average_service_time = _Stats(completed, rejected), latency


def test_evaluators_are_healthy_like_the_reference():
    """The two evaluators on their own, in host Python, over the recorder's enumerated inputs -- and over hs.Server objects."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_canary.py")
    text = open(path).read()
    ns = {}
    exec(compile(text[text.index("def evaluator_inputs():"):text.index("def record_evaluators(ns):")], path, "exec"), ns)   # (the inputs alone)
    rows = ns["evaluator_inputs"]()
    want = CR.get("evaluators")["healthy"].tolist()
    assert len(rows) == len(want) == 6 * 7 * 6 and 0 < sum(want) < len(want)
    got = [int(CS.make_evaluator(hs, ev).is_healthy(_Backend(*cn), [_Backend(*b) for b in base])) for ev, cn, base in rows]
    assert got == want
    a, b = hs.Server("a"), hs.Server("b")
    a._requests_completed, a._requests_rejected, b._requests_completed, b._requests_rejected = 9, 1, 8, 2
    assert hs.ErrorRateEvaluator(0.5, 1.0).is_healthy(a, [b]) and not hs.ErrorRateEvaluator(0.5, 1.0).is_healthy(b, [a])
    assert not hs.ErrorRateEvaluator(0.05).is_healthy(a, []) and hs.ErrorRateEvaluator().is_healthy(object(), [object()])


def test_every_refusal_by_name():
    def refused(text, make):
        with pytest.raises((UT, NotImplementedError), match=text):
            sim = make()
            sim._general_prepare(sim.lowered(), False)

    class Other:
        def is_healthy(self, canary, baseline_backends):
            return True

    refused("canary deployer 'can': metric evaluator Other is not lowered to the engine", lambda: _fleet(dict(metric_evaluator=Other()))[0])
    refused("canary deployer 'can': 2 deploy\\(\\) Events are scheduled -- a second canary of the same name is never registered",
            lambda: _fleet(deploys=2)[0])
    for strat in (hs.ConsistentHash(), hs.IPHash(), hs.Random()):
        refused(f"strategy {type(strat).__name__} of 'lb' is not lowered under a deployer", lambda s=strat: _fleet(strategy=s)[0])
    for strat in (hs.PowerOfTwoChoices(), hs.LeastResponseTime()):
        refused(f"strategy {type(strat).__name__} is not lowered to the engine", lambda s=strat: _fleet(strategy=s)[0])
    sim, o = _fleet()
    mk = lambda name: hs.Server(name)  # noqa: E731
    with_ = lambda *more: hs.Simulation(sources=[o["src"]], entities=o["servers"] + [o["lb"], o["sink"]] + list(more),  # noqa: E731
                                        end_time=hs.Instant.from_seconds(1.0))
    refused("LoadBalancer 'lb' has the CanaryDeployer 'can' already", lambda: with_(o["canary"], hs.RollingDeployer("roll", o["lb"], mk)))
    refused("LoadBalancer 'lb' has the CanaryDeployer 'can' already", lambda: with_(o["canary"], hs.CanaryDeployer("two", o["lb"], mk)))
    refused("LoadBalancer 'lb' has the AutoScaler 'scaler' already", lambda: with_(hs.AutoScaler("scaler", o["lb"], mk), o["canary"]))
    checker = hs.HealthChecker("hc", o["lb"], interval=0.5, timeout=0.2)
    for ents in ([o["canary"], checker], [checker, o["canary"]]):
        refused("a HealthChecker and a CanaryDeployer on one LoadBalancer are not lowered", lambda e=ents: with_(*e))

    def unhealthy():
        sim, o = _fleet()
        o["lb"].mark_unhealthy(o["servers"][1])
        return sim

    refused("backend 'srv1' of 'lb' is marked unhealthy -- health marks under a deployer are not lowered", unhealthy)
    away = hs.CanaryDeployer("away", hs.LoadBalancer("other"), mk)
    refused("canary deployer 'away': its LoadBalancer is not an entity of this Simulation", lambda: _fleet(extra=[away])[0])
    refused("server_factory returned a Sink for instance 1: only Servers may stand", lambda: _fleet(factory=lambda name: hs.Sink(name))[0])
    outside = hs.Sink("outside")
    refused("the downstream 'outside' of instance 1 is not an entity of this Simulation",
            lambda: _fleet(factory=lambda name: hs.Server(name, downstream=outside))[0])
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-10):
        refused("evaluation_interval = .* must be a finite number of at least one nanosecond", lambda b=bad: _fleet(dict(evaluation_interval=b))[0])
    for stage in (hs.CanaryStage(float("nan"), 1.0), hs.CanaryStage(0.5, float("inf")), hs.CanaryStage("half", 1.0)):
        refused("stage 1 has a traffic_percentage or evaluation_period that is no finite number",
                lambda s=stage: _fleet(dict(stages=[hs.CanaryStage(0.1, 1.0), s]))[0])
    refused("17 stages are beyond the 16", lambda: _fleet(dict(stages=[hs.CanaryStage(0.1, 1.0)] * 17))[0])
    _fleet(dict(stages=[hs.CanaryStage(0.1, 1.0)] * 16))[0].lowered()
    _fleet(end_s=None)[0].lowered()                                        # end_time = Infinity: one instance, no horizon needed
    sim, o = _fleet()
    with pytest.raises(UT, match="the CanaryDeployer 'can' on a ParallelSimulation partition is not lowered"):
        hs.ParallelSimulation([hs.SimulationPartition("p", entities=o["servers"] + [o["lb"], o["sink"], o["canary"]], sources=[o["src"]])],
                              duration=1.0)
    sim, o = _fleet(deploys=0)
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(1.0), event_type="_canary_evaluate", target=o["canary"]))
    with pytest.raises(UT, match="only the Event deploy\\(\\) returns is lowered for a CanaryDeployer"):
        sim._general_prepare(sim.lowered(), False)
    sim, o = _fleet()
    ents = o["servers"] + [o["lb"], o["sink"], o["canary"]]
    refused("'s2' forwards to it: the CanaryDeployer 'can' takes no Requests", lambda: hs.Simulation(
        sources=[o["src"], hs.Source.poisson(rate=1.0, target=o["canary"], name="s2")], entities=ents, end_time=hs.Instant.from_seconds(1.0)))
    front = hs.LoadBalancer("front", backends=[o["canary"]])
    refused("'front' forwards to it: the CanaryDeployer 'can' takes no Requests", lambda: hs.Simulation(
        sources=[o["src"], hs.Source.poisson(rate=1.0, target=front, name="s3")], entities=ents + [front], end_time=hs.Instant.from_seconds(1.0)))
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("can_canary", at=1.0))
    with pytest.raises(UT, match="fault CrashNode names 'can_canary', an instance of the pool of CanaryDeployer 'can'"):
        _fleet(fault_schedule=fs)
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("can", at=1.0))
    _fleet(fault_schedule=fs)[0].lowered()


def test_the_lowered_arrays():
    spec = CS.FIXTURES["canary_next_to_a_rolling_free_load_balancer"]
    sim, pools = CS.build(spec)
    g = sim.lowered()
    a = g.arrays
    assert isinstance(g, GeneralGraph) and "CanaryDeployer" in sim._station_refusal
    own = pools["source"] + pools["server"] + pools["lb"] + pools["sink"] + pools["canary"]
    assert g.nodes[:g.n_own] == own and a.n == g.n_own + 2
    for i, cn in enumerate(pools["canary"]):
        node, lb_node, at = g.node_of[id(cn)], g.node_of[id(cn.load_balancer)], g.n_own + i
        assert a.kind[node] == N.NODE_CANARY_DEPLOYER and a.target[node] == lb_node and g.deployed[lb_node][0] == node
        assert g.nodes[at] is pools["factory"][i].made[0] is cn._pool[0] and cn._pool[0].name == f"cn{i}_canary" and g.dpool_of[at] == (node, 1)
        assert a.kind[at] == N.NODE_SERVER and a.stream_base[at] == len(pools["server"])        # the canary takes k = 1
        off, cnt = int(a.rt_off[lb_node]), int(a.rt_cnt[lb_node])
        assert cnt == len(cn.load_balancer.all_backends) + 1 and a.rt_targets[off + cnt - 1] == at and a.lb_weights[off + cnt - 1] == 1
        c = spec["canaries"][i]
        stages, evaluator, limit, mult, iv = a.cn_params[node]
        assert stages == [tuple(s) for s in c["stages"]] and iv == c["iv"]
        assert (evaluator, limit, mult) == ((N.CANARY_ERROR_RATE, 0.05, 2.0) if c["ev"] is None else (N.CANARY_LATENCY, c["ev"][1], c["ev"][2]))
    assert a.has_canaries and not a.has_deployers and a.has_health and "cn_params" not in vars(a)
    sim.lowered()
    assert [len(f.made) for f in pools["factory"]] == [1, 1]                # the factory is called once
    parts = split_parts(CS.build(CS.groups_spec(16))[0].lowered().arrays)
    assert len(parts) == 16 and all((b.kind == N.NODE_CANARY_DEPLOYER).sum() == 1 and b.cn_params is not None for _i, _p, b in parts)


def test_what_the_recordings_cover():
    refs = [CR.get("case", s) for s in CS.all_specs()]
    state = np.concatenate([r["cn_state"] for r in refs])
    assert (state[:, 7] == CS.STATUS["completed"]).sum() >= 40 and (state[:, 7] == CS.STATUS["rolled_back"]).sum() >= 10
    assert (state[:, 7] == CS.STATUS["in_progress"]).sum() >= 3 and all(r["python"][:2] < [3, 12] for r in refs)
    assert any(any(w > 1 for _k, w in r["cn_weights"][0]) for r in refs) and any(r["cn_weights"][0] == [] for r in refs)
    assert max(len(r["cn_baseline"][0]) for r in refs) >= 66


def test_the_new_symbols_of_the_c_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hs_engine.h")).read()
    for sym in ("hs_graph_set_canary_deployer", "hs_graph_get_canary_deployer"):
        assert sym in N.EXPORTED_SYMBOLS and re.search(r"\bint " + sym + r"\(", header), sym
    assert re.search(r"HS_NODE_CANARY_DEPLOYER = (\d+)", header).group(1) == str(N.NODE_CANARY_DEPLOYER) == "17"
    for name, value in (("HS_CANARY_KINDS", N.CANARY_KINDS), ("HS_CANARY_MAX_STAGES", N.CANARY_MAX_STAGES), ("HS_CANARY_FIELDS", N.CANARY_FIELDS)):
        assert re.search(rf"#define {name} (\d+)", header).group(1) == str(value)
    assert hs.CanaryDeployer.MAX_STAGES == N.CANARY_MAX_STAGES and len(CS.CN_EVENTS) == N.CANARY_KINDS
    status = re.search(r"typedef enum hs_canary_status \{([^}]*)\}", header).group(1)
    assert [s.split("=")[0].strip()[len("HS_CANARY_"):].lower() for s in status.split(",")] == list(N.CANARY_STATUS)
    assert N.EV_KINDS + 4 + 3 + 6 + 3 + N.FLOW_KINDS + 1 + N.DEPLOYER_KINDS + N.CANARY_KINDS == CS.N_KINDS == 53
