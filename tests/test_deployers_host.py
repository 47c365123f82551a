"""Host side of the RollingDeployer (no GPU): the constructor, defaults, dataclasses and the deploy() Event, every refusal by its message,
the pool bound against every recording, the lowered arrays, the parts, the new symbols of the C ABI, and that graphs of the existing
families hold no deployer state."""
import dataclasses
import os
import re

import numpy as np
import pytest

import deployer_specs as DS
import happy_simulator_amd as hs
import mixed_specs as MX
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, deployer_pool_size, split_parts
from happy_simulator_amd.lowering import UnsupportedTopology as UT

DR = DS.DEPLOYERS


def _fleet(deployer_kw=None, strategy=None, n_init=3, end_s=5.0, extra=(), deploys=1, factory=None, lb_in=True, **sim_kw):
    """Source -> LoadBalancer over `n_init` Servers, deployed -> Sink."""
    sink = hs.Sink("sink")
    servers = [hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink) for i in range(n_init)]
    lb = hs.LoadBalancer("lb", backends=servers, strategy=strategy)
    factory = factory or (lambda name: hs.Server(name, service_time=hs.ExponentialLatency(0.05), downstream=sink))
    dp = hs.RollingDeployer("roll", lb, factory, **(deployer_kw or {}))
    src = hs.Source.poisson(rate=20.0, target=lb, name="src")
    sim = hs.Simulation(sources=[src], entities=servers + ([lb] if lb_in else []) + [sink] + list(extra) + [dp],
                        **({} if end_s is None else {"end_time": hs.Instant.from_seconds(end_s)}), **sim_kw)
    for _ in range(deploys):
        sim.schedule(dp.deploy())
    return sim, dict(sink=sink, servers=servers, lb=lb, deployer=dp, src=src)


def test_constructor_defaults_and_dataclasses_are_the_references():
    lb = hs.LoadBalancer("lb")
    dp = hs.RollingDeployer("d", lb, lambda name: hs.Server(name))
    assert (dp.name, dp.load_balancer, dp._batch_size, dp._health_check_interval, dp._healthy_threshold, dp._max_failures) == ("d", lb, 1, 2.0, 2, 1)
    assert (dp._old_backends, dp._new_backends, dp._current_batch_old, dp._current_batch_new, dp._health_pass_count) == ([], [], [], [], {})
    assert (dp._health_fail_count, dp._next_instance_id) == (0, 0) and dp.downstream_entities() == [lb] and isinstance(dp, hs.Entity)
    assert dataclasses.astuple(dp.stats) == (0,) * 7 and [f.name for f in dataclasses.fields(dp.stats)] == [
        "deployments_started", "deployments_completed", "deployments_rolled_back", "instances_replaced", "health_checks_performed",
        "health_checks_passed", "health_checks_failed"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        dp.stats.deployments_started = 1
    assert dataclasses.asdict(dp.state) == dict(status="idle", total_instances=0, replaced=0, failed=0, current_batch=0)
    dp.state.current_batch = 3                                             # (a plain dataclass, as the reference's)
    assert hs.DeploymentState(status="completed").status == "completed" and isinstance(dp.stats, hs.RollingDeployerStats)
    assert N.DEPLOYMENT_STATUS == ("idle", "in_progress", "completed", "rolled_back")


def test_the_deploy_event():
    lb = hs.LoadBalancer("lb")
    dp = hs.RollingDeployer("d", lb, lambda name: hs.Server(name))
    ev = dp.deploy()
    assert (ev.time, ev.event_type, ev.target, ev.daemon, ev.on_complete) == (hs.Instant.Epoch, "_rolling_deploy_start", dp, False, [])
    sim, o = _fleet(start_time=hs.Instant.from_seconds(2.0), end_s=4.0, deploys=0)
    assert o["deployer"].deploy().time == hs.Instant.from_seconds(2.0)     # `now` of the clock the Simulation handed over
    ev = o["deployer"].deploy()
    ev.time = hs.Instant.from_seconds(3.0)                                 # the caller may set its time, as with Client.send_request()
    sim.schedule(ev)
    g = sim.lowered()
    _end, _start, sched, _c = sim._general_prepare(g, False)
    assert sched == [(g.node_of[id(o["deployer"])], 3 * 10 ** 9)]


def test_every_refusal_by_name():
    def refused(text, make):
        with pytest.raises((UT, NotImplementedError), match=text):
            sim = make()
            sim._general_prepare(sim.lowered(), False)

    for strat in (hs.ConsistentHash(), hs.IPHash(), hs.Random()):
        refused(f"strategy {type(strat).__name__} of 'lb' is not lowered under a deployer", lambda s=strat: _fleet(strategy=s)[0])
    sim, o = _fleet()
    mk = lambda name: hs.Server(name)  # noqa: E731
    second = hs.RollingDeployer("second", o["lb"], mk)
    scaler = hs.AutoScaler("scaler", o["lb"], mk)
    checker = hs.HealthChecker("hc", o["lb"], interval=0.5, timeout=0.2)
    with_ = lambda *more: hs.Simulation(sources=[o["src"]], entities=o["servers"] + [o["lb"], o["sink"]] + list(more),  # noqa: E731
                                        end_time=hs.Instant.from_seconds(1.0))
    refused("LoadBalancer 'lb' has the RollingDeployer 'roll' already", lambda: with_(o["deployer"], second))
    refused("LoadBalancer 'lb' has the AutoScaler 'scaler' already", lambda: with_(scaler, o["deployer"]))
    refused("LoadBalancer 'lb' has the AutoScaler 'scaler' already", lambda: with_(o["deployer"], scaler))
    for ents in ([o["deployer"], checker], [checker, o["deployer"]]):
        refused("a HealthChecker and a RollingDeployer on one LoadBalancer are not lowered", lambda e=ents: with_(*e))

    def unhealthy():
        sim, o = _fleet()
        o["lb"].mark_unhealthy(o["servers"][1])
        return sim

    refused("backend 'srv1' of 'lb' is marked unhealthy -- health marks under a deployer are not lowered", unhealthy)
    elsewhere = hs.RollingDeployer("away", hs.LoadBalancer("other"), mk)
    refused("rolling deployer 'away': its LoadBalancer is not an entity of this Simulation", lambda: _fleet(extra=[elsewhere])[0])
    refused("server_factory returned a Sink for instance 1: only Servers may stand", lambda: _fleet(factory=lambda name: hs.Sink(name))[0])
    outside = hs.Sink("outside")
    refused("the downstream 'outside' of instance 1 is not an entity of this Simulation",
            lambda: _fleet(factory=lambda name: hs.Server(name, downstream=outside))[0])
    one = hs.Server("one")
    refused("server_factory returned 'one' for instance 2", lambda: _fleet(factory=lambda name: one)[0])
    refused("batch_size must be an int of at least 1 below 2\\^30, got 0", lambda: _fleet(dict(batch_size=0))[0])
    refused("healthy_threshold must be an int of at least 1 below 2\\^30, got 0", lambda: _fleet(dict(healthy_threshold=0))[0])
    refused("max_failures must be an int below 2\\^30, got 1.5", lambda: _fleet(dict(max_failures=1.5))[0])
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-10):
        refused("health_check_interval = .* must be a finite number of at least one nanosecond", lambda b=bad: _fleet(dict(health_check_interval=b))[0])
    # P = n0 * (2^D - 1): 3 backends and 11 deploy() Events could create 6 141 instances
    refused("11 deploy\\(\\) Events over 3 backends could create up to 6141 instances, beyond the pool of 4096", lambda: _fleet(deploys=11)[0])
    assert _fleet(deploys=10)[0].lowered().arrays.n == 7 + 3 * 1023
    _fleet(end_s=None)[0].lowered()                                        # end_time = Infinity: the pool bound needs no horizon
    sim, o = _fleet()
    with pytest.raises(UT, match="the RollingDeployer 'roll' on a ParallelSimulation partition is not lowered"):
        hs.ParallelSimulation([hs.SimulationPartition("p", entities=o["servers"] + [o["lb"], o["sink"], o["deployer"]], sources=[o["src"]])],
                              duration=1.0)
    # only what deploy() returns is lowered for a deployer; deploy() Events scheduled behind the lowering would outgrow the pool
    sim, o = _fleet()
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(1.0), event_type="_rolling_health_check", target=o["deployer"]))
    with pytest.raises(UT, match="only the Event deploy\\(\\) returns is lowered for a RollingDeployer"):
        sim._general_prepare(sim.lowered(), False)
    sim, o = _fleet()
    g = sim.lowered()
    sim.schedule(o["deployer"].deploy())
    with pytest.raises(UT, match="deploy\\(\\) Events scheduled after the graph was lowered"):
        sim._general_prepare(g, False)
    # a deployer takes no Requests: neither as anyone's target nor as a LoadBalancer's backend
    sim, o = _fleet()
    ents = o["servers"] + [o["lb"], o["sink"], o["deployer"]]
    refused("'s2' forwards to it: the RollingDeployer 'roll' takes no Requests", lambda: hs.Simulation(
        sources=[o["src"], hs.Source.poisson(rate=1.0, target=o["deployer"], name="s2")], entities=ents, end_time=hs.Instant.from_seconds(1.0)))
    front = hs.LoadBalancer("front", backends=[o["deployer"]])
    refused("'front' forwards to it: the RollingDeployer 'roll' takes no Requests", lambda: hs.Simulation(
        sources=[o["src"], hs.Source.poisson(rate=1.0, target=front, name="s3")], entities=ents + [front], end_time=hs.Instant.from_seconds(1.0)))
    # the two strategies no engine lowers at all keep their own refusal on a deployed LoadBalancer
    for strat in (hs.PowerOfTwoChoices(), hs.LeastResponseTime()):
        refused(f"strategy {type(strat).__name__} is not lowered to the engine", lambda s=strat: _fleet(strategy=s)[0])
    # a FaultSchedule may name the deployer; a pool instance is no entity of the Simulation: refused by name when the Simulation is
    # constructed
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("roll", at=1.0))
    _fleet(fault_schedule=fs)[0].lowered()
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("roll_v2_1", at=1.0))
    with pytest.raises(UT, match="fault CrashNode names 'roll_v2_1', an instance of the pool of RollingDeployer 'roll': a pool instance is no "
                                 "entity of the Simulation and cannot be named by a FaultSchedule"):
        _fleet(fault_schedule=fs)
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("nobody", at=1.0))
    with pytest.raises(KeyError, match="^'nobody'$"):                      # (any other unknown name: the name dict's KeyError, as in the reference)
        _fleet(fault_schedule=fs)


def test_the_pool_is_the_documented_bound():
    """P = n0 * (2^D - 1): deployment j replaces at most the members it found, the initial backends and every instance
    made so far."""
    assert [deployer_pool_size(3, d) for d in (0, 1, 2, 3)] == [0, 3, 9, 21] and deployer_pool_size(0, 5) == 0
    used = []
    for spec in DS.recorded_specs():
        sim, pools = DS.build(spec)
        g = sim.lowered()
        ref = DR.get("case", spec)
        for i, dp in enumerate(pools["deployer"]):
            node = g.node_of[id(dp)]
            size = int(g.arrays.rd_params[node, 4])
            n_init = len(dp.load_balancer.all_backends)
            assert size == deployer_pool_size(n_init, len(spec["deployers"][i]["deploys"])) == len(dp._pool)
            assert ref["rd_state"][i, 12] <= size                       # no recorded run of the reference outgrew the pool
            if size:
                used.append(ref["rd_state"][i, 12] / size)
    assert max(used) == 1.0 and len(used) > 100


def test_the_lowered_arrays():
    spec = DS.FIXTURES["two_deployed_load_balancers"]
    sim, pools = DS.build(spec)
    g = sim.lowered()
    a = g.arrays
    assert isinstance(g, GeneralGraph) and sim._station_refusal == "the station, network and pipeline engines do not lower a RollingDeployer or a CanaryDeployer"
    # the Simulation's own nodes first (Sources, then the entities in their order), the pools behind them, deployer by deployer
    own = pools["source"] + pools["server"] + pools["lb"] + pools["sink"] + pools["deployer"]
    assert g.nodes[:g.n_own] == own and g.n_own == len(own)
    sizes = [int(a.rd_params[g.node_of[id(dp)], 4]) for dp in pools["deployer"]]
    assert sizes == [2, 1] and a.n == g.n_own + sum(sizes)
    at = g.n_own
    for i, (dp, size) in enumerate(zip(pools["deployer"], sizes)):
        node, lb_node = g.node_of[id(dp)], g.node_of[id(dp.load_balancer)]
        assert a.kind[node] == N.NODE_ROLLING_DEPLOYER and a.target[node] == lb_node and g.deployed[lb_node][0] == node
        assert g.nodes[at:at + size] == pools["factory"][i].made == dp._pool and [s.name for s in dp._pool] == [f"rd{i}_v2_{k + 1}" for k in range(size)]
        assert (a.kind[at:at + size] == N.NODE_SERVER).all() and [g.dpool_of[n] for n in range(at, at + size)] == [(node, k + 1) for k in range(size)]
        # instance k: the Servers' SERVICE numbering goes on behind the Servers the Simulation lists
        assert a.stream_base[at:at + size].tolist() == [len(pools["server"]) + k for k in range(size)]
        off, cnt = int(a.rt_off[lb_node]), int(a.rt_cnt[lb_node])
        n_init = len(dp.load_balancer.all_backends)
        assert cnt == n_init + size and a.rt_targets[off + n_init:off + cnt].tolist() == list(range(at, at + size))
        d = spec["deployers"][i]
        assert a.rd_params[node].tolist() == [d["batch"], d["iv"], d["thr"], d["fails"], size]
        at += size
    assert a.lb_healthy is not None and a.lb_healthy.all() and a.has_health and a.has_deployers and not a.has_scalers
    assert "rd_params" not in vars(a)                                      # (the arrays' public attributes are what they were)
    # an instance joins at weight 1 whatever the initial backends weigh
    lb_node = g.node_of[id(pools["lb"][1])]
    off = int(a.rt_off[lb_node])
    assert a.lb_weights[off:off + 2].tolist() == [int(pools["lb"][1].strategy.get_weight(pools["server"][2])), 1]
    # the factory is called once per instance, also when the graph is lowered again
    sim.lowered()
    assert [len(f.made) for f in pools["factory"]] == sizes


def test_parts_hold_a_pool_with_its_load_balancer():
    spec = DS.groups_spec(16)
    sim, pools = DS.build(spec)
    g = sim.lowered()
    parts = split_parts(g.arrays)
    assert len(parts) == 16
    for ids, _pos, b in parts:
        (dp_node,) = np.nonzero(b.kind == N.NODE_ROLLING_DEPLOYER)[0]
        lb_node = int(b.target[dp_node])
        size = int(b.rd_params[dp_node, 4])
        assert size == 2 and b.kind[lb_node] == N.NODE_LB and b.rt_cnt[lb_node] == 2 + size and (b.kind == N.NODE_SERVER).sum() == 2 + size
        assert b.n == 6 + size and b.lb_healthy is not None
        assert [g.dpool_of[int(i)][1] for i in ids if int(i) in g.dpool_of] == list(range(1, size + 1))


def test_what_the_recordings_cover():
    """Conditions on what the live reference did (the recorder asserts the named fixtures one by one)."""
    refs = [DR.get("case", s) for s in DS.all_specs()]
    state = np.concatenate([r["rd_state"] for r in refs])
    assert (state[:, 1] > 0).sum() >= 60 and (state[:, 2] > 0).sum() >= 20 and (state[:, 0] > 1).sum() >= 20      # completed, rolled back, two deploys
    assert ((state[:, 1] > 0) & (state[:, 2] > 0)).sum() >= 5              # "completed" behind "rolled_back"
    assert (state[:, 9] > state[:, 8]).any()                               # state.replaced counts the batches' lists, not what left
    assert sum(r["rd_members"][0] == [] for r in refs) >= 3 and any(r["probe_drops"] > 0 for r in refs)
    assert any((r["rd_instance_total_requests"] == -1).any() for r in refs) and any((r["lb_backend_total_requests"] == -1).any() for r in refs)
    assert max(len(r["rd_members"][0]) for r in refs) >= 66
    # an initial backend behind a newer instance in the member list: not among what the reference reaches ("Deployers")
    for r in refs:
        for members in r["rd_members"]:
            kinds = ["_v2_" in m for m in members]
            assert kinds == sorted(kinds)


def test_the_new_symbols_of_the_c_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hs_engine.h")).read()
    for sym in ("hs_graph_set_rolling_deployer", "hs_graph_get_rolling_deployer", "hs_debug_compact_members"):
        assert sym in N.EXPORTED_SYMBOLS and re.search(r"\bint " + sym + r"\(", header), sym
    assert re.search(r"HS_NODE_ROLLING_DEPLOYER = (\d+)", header).group(1) == str(N.NODE_ROLLING_DEPLOYER) == "16"
    assert re.search(r"HS_NODE_AUTO_SCALER = (\d+)", header).group(1) == "15"          # the new kind stands behind it
    for name, value in (("HS_DEPLOYER_KINDS", N.DEPLOYER_KINDS), ("HS_DEPLOYER_MAX_POOL", N.DEPLOYER_MAX_POOL), ("HS_DEPLOYER_FIELDS", N.DEPLOYER_FIELDS)):
        assert re.search(rf"#define {name} (\d+)", header).group(1) == str(value)
    assert hs.RollingDeployer.MAX_POOL == N.DEPLOYER_MAX_POOL and len(DS.RD_EVENTS) == N.DEPLOYER_KINDS
    status = re.search(r"typedef enum hs_deployment_status \{([^}]*)\}", header).group(1)
    assert [s.split("=")[0].strip()[len("HS_DEPLOYMENT_"):].lower() for s in status.split(",")] == list(N.DEPLOYMENT_STATUS)


def test_graphs_without_a_deployer_hold_no_deployer_state():
    """Graphs of the existing families hold no pool, no parameters and no deployer node (that their arrays are byte for byte the
    parent's is tests/test_autoscaler_host.py::test_existing_lowering_is_unchanged_without_a_scaler, which passes unchanged)."""
    seen = 0
    for spec in list(MX.FIXTURES.values())[::4]:
        sim, _pools = MX.build(spec)
        g = sim.lowered()
        if not isinstance(g, GeneralGraph):
            continue
        a = g.arrays
        assert not a.has_deployers and a.rd_params is None and g.n_own == a.n and not g.dpool_of and not g.deployed and not g.deploys
        assert (a.kind != N.NODE_ROLLING_DEPLOYER).all()
        seen += 1
    assert seen >= 5
