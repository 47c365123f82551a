"""Host side of the AutoScaler (no GPU): the constructors, defaults, properties and error texts, the start Event, the three policies'
`evaluate` against the recorded reference over enumerated inputs, every refusal by its message, the lowered arrays (the pool's size is
the documented bound, the stream bases, the node order), and that the lowering of the existing families is unchanged."""
import dataclasses
import hashlib

import numpy as np
import pytest

import autoscaler_specs as AS
import happy_simulator_amd as hs
import link_fault_specs as LS
import mixed_specs as MX
import queue_specs as QS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, scaler_pool_size, split_parts
from happy_simulator_amd.lowering import UnsupportedTopology as UT

AR = AS.AUTOSCALER


def _pool(scaler_kw=None, strategy=None, n_init=1, end_s=5.0, extra=(), starts=1, factory=None, lb_in=True, **sim_kw):
    """Source -> LoadBalancer over `n_init` Servers, scaled -> Sink."""
    sink = hs.Sink("sink")
    servers = [hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink) for i in range(n_init)]
    lb = hs.LoadBalancer("lb", backends=servers, strategy=strategy)
    factory = factory or (lambda name: hs.Server(name, service_time=hs.ExponentialLatency(0.05), downstream=sink))
    sc = hs.AutoScaler("scaler", lb, factory, **(scaler_kw or {}))
    src = hs.Source.poisson(rate=20.0, target=lb, name="src")
    sim = hs.Simulation(sources=[src], entities=servers + ([lb] if lb_in else []) + [sink] + list(extra) + [sc],
                        **({} if end_s is None else {"end_time": hs.Instant.from_seconds(end_s)}), **sim_kw)
    for _ in range(starts):
        sim.schedule(sc.start())
    return sim, dict(sink=sink, servers=servers, lb=lb, scaler=sc, src=src)


def test_constructor_defaults_and_properties_are_the_references():
    lb = hs.LoadBalancer("lb")
    sc = hs.AutoScaler("s", lb, lambda name: hs.Server(name))
    assert (sc.name, sc.load_balancer, sc.min_instances, sc.max_instances, sc.current_count, sc.is_running) == ("s", lb, 1, 10, 0, False)
    assert (sc._evaluation_interval, sc._scale_out_cooldown, sc._scale_in_cooldown) == (10.0, 30.0, 60.0)
    assert isinstance(sc._policy, hs.TargetUtilization) and sc._policy.target == 0.7
    assert (sc._last_scale_time, sc._last_scale_action, sc._next_instance_id, sc._managed_servers, sc.scaling_history) == (None, None, 0, [], [])
    assert sc.downstream_entities() == [lb] and isinstance(sc, hs.Entity)
    assert dataclasses.astuple(sc.stats) == (0,) * 6 and [f.name for f in dataclasses.fields(sc.stats)] == [
        "evaluations", "scale_out_count", "scale_in_count", "instances_added", "instances_removed", "cooldown_blocks"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        sc.stats.evaluations = 1
    ev = hs.ScalingEvent(hs.Instant.Epoch, "scale_out", 1, 2, "Added 1 instances")
    assert [f.name for f in dataclasses.fields(ev)] == ["time", "action", "from_count", "to_count", "reason"]
    ev.to_count = 3                                                        # (a plain dataclass, as the reference's)
    for bad in (0, 0.0, -0.1, 1.0000001, 2):
        with pytest.raises(ValueError, match=r"target must be in \(0, 1\], got "):
            hs.TargetUtilization(bad)
    with pytest.raises(ValueError) as e:
        hs.TargetUtilization(1.5)
    assert str(e.value) == "target must be in (0, 1], got 1.5"
    assert hs.TargetUtilization(1.0).target == 1.0
    q = hs.QueueDepthScaling()
    assert (q._scale_out_threshold, q._scale_in_threshold) == (100, 10)
    steps = [(0.5, 1), (0.9, 2), (0.5, 7), (0.0, -1)]
    assert hs.StepScaling(steps)._steps == sorted(steps, key=lambda s: s[0], reverse=True) == [(0.9, 2), (0.5, 1), (0.5, 7), (0.0, -1)]


def test_the_start_event():
    lb = hs.LoadBalancer("lb")
    sc = hs.AutoScaler("s", lb, lambda name: hs.Server(name))
    ev = sc.start()
    assert sc.is_running and (ev.time, ev.event_type, ev.target, ev.daemon, ev.on_complete) == (hs.Instant.Epoch, "_autoscaler_evaluate", sc, True, [])
    sc.stop()
    assert not sc.is_running
    sim, o = _pool(start_time=hs.Instant.from_seconds(2.0), end_s=4.0)
    assert o["scaler"].start().time == hs.Instant.from_seconds(2.0)       # `now` of the clock the Simulation handed over


class _Backend:
    def __init__(self, active, limit, depth):
        self.utilization, self.depth = active / limit, depth


def test_policies_evaluate_like_the_reference():
    """The three policies on their own, in host Python, over the recorder's enumerated inputs -- and over hs.Server objects."""
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_autoscaler.py")
    src = open(path).read()
    body = src[src.index("def policy_inputs():"):src.index("def record_policies(ns):")]
    ns = {}
    exec(compile(body, path, "exec"), ns)                                  # (the inputs alone: the recorder itself imports the reference)
    rows = ns["policy_inputs"]()
    want = AR.get("policies")["desired"].tolist()
    assert len(rows) == len(want) == 9 * 7 * 4
    got = [AS.make_policy(hs, pol).evaluate([_Backend(*b) for b in load], cur, lo, hi) for pol, load, cur, lo, hi in rows]
    assert got == want
    a, b = hs.Server("a", concurrency=2), hs.Server("b", concurrency=4)
    a._active, b._active, a._queue.depth, b._queue.depth = 2, 1, 3, 0
    assert hs.TargetUtilization(0.5).evaluate([a, b], 2, 1, 10) == int(2 * ((1.0 + 0.25) / 2) / 0.5 + 0.5) == 3
    assert hs.QueueDepthScaling(3, 0).evaluate([a, b], 2, 1, 10) == 3 and hs.StepScaling([(0.6, 2)]).evaluate([a, b], 2, 1, 10) == 4


def test_every_refusal_by_name():
    def refused(text, make):
        with pytest.raises((UT, NotImplementedError), match=text):
            sim = make()
            sim._general_prepare(sim.lowered(), False)

    class Other:
        def evaluate(self, backends, current_count, min_instances, max_instances):
            return current_count

    refused("policy Other is not lowered", lambda: _pool(dict(policy=Other()))[0])
    for strat in (hs.ConsistentHash(), hs.IPHash(), hs.Random()):
        refused(f"strategy {type(strat).__name__} of 'lb' is not lowered under an AutoScaler", lambda s=strat: _pool(strategy=s)[0])
    sim, o = _pool()
    second = hs.AutoScaler("second", o["lb"], lambda name: hs.Server(name))
    refused("LoadBalancer 'lb' has the scaler 'scaler' already", lambda: hs.Simulation(
        sources=[o["src"]], entities=o["servers"] + [o["lb"], o["sink"], o["scaler"], second], end_time=hs.Instant.from_seconds(1.0)))
    checker = hs.HealthChecker("hc", o["lb"], interval=0.5, timeout=0.2)
    for ents in ([o["scaler"], checker], [checker, o["scaler"]]):
        refused("a HealthChecker and an AutoScaler on one LoadBalancer are not lowered", lambda e=ents: hs.Simulation(
            sources=[o["src"]], entities=o["servers"] + [o["lb"], o["sink"]] + e, end_time=hs.Instant.from_seconds(1.0)))

    def unhealthy():
        sim, o = _pool(n_init=2)
        o["lb"].mark_unhealthy(o["servers"][1])
        return sim

    refused("backend 'srv1' of 'lb' is marked unhealthy -- health marks under an AutoScaler are not lowered", unhealthy)
    elsewhere = hs.AutoScaler("away", hs.LoadBalancer("other"), lambda name: hs.Server(name))
    refused("auto scaler 'away': its LoadBalancer is not an entity of this Simulation", lambda: _pool(extra=[elsewhere])[0])
    refused("server_factory returned a Sink for instance 1: only Servers may stand", lambda: _pool(factory=lambda name: hs.Sink(name))[0])
    outside = hs.Sink("outside")
    refused("the downstream 'outside' of instance 1 is not an entity of this Simulation",
            lambda: _pool(factory=lambda name: hs.Server(name, downstream=outside))[0])
    one = hs.Server("one")
    refused("server_factory returned 'one' for instance 2", lambda: _pool(factory=lambda name: one)[0])
    refused("StepScaling with 17 steps is beyond the 16", lambda: _pool(dict(policy=hs.StepScaling([(k / 20, 1) for k in range(17)])))[0])
    _pool(dict(policy=hs.StepScaling([(k / 20, 1) for k in range(16)])))[0].lowered()
    fast = dict(evaluation_interval=0.001, scale_out_cooldown=0.0, scale_in_cooldown=0.0, max_instances=3)
    refused("could create up to 4102 instances, beyond the pool of 4096", lambda: _pool(fast, end_s=4.1)[0])
    assert _pool(fast, end_s=4.09)[0].lowered().arrays.n == 5 + 4092
    refused("end_time = Infinity leaves no horizon to size its instance pool by", lambda: _pool(end_s=None)[0])
    refused("evaluation_interval = 1e-10", lambda: _pool(dict(evaluation_interval=1e-10))[0])
    sim, o = _pool()
    with pytest.raises(UT, match="the AutoScaler 'scaler' on a ParallelSimulation partition is not lowered"):
        hs.ParallelSimulation([hs.SimulationPartition("p", entities=o["servers"] + [o["lb"], o["sink"], o["scaler"]], sources=[o["src"]])],
                              duration=1.0)
    # only what start() returns is lowered for a scaler; start() Events scheduled behind the lowering would outgrow the pool
    sim, o = _pool()
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(1.0), event_type="_autoscaler_evaluate", target=o["scaler"], daemon=True))
    with pytest.raises(UT, match="only the daemon Event start\\(\\) returns, at the Simulation's start, is lowered for an AutoScaler"):
        sim._general_prepare(sim.lowered(), False)
    sim, o = _pool()
    g = sim.lowered()
    sim.schedule(o["scaler"].start())
    with pytest.raises(UT, match="start\\(\\) Events scheduled after the graph was lowered"):
        sim._general_prepare(g, False)
    # a Probe on anything but current_count of a scaler stays an arbitrary attribute
    with pytest.raises(NotImplementedError, match="probe metric 'current_count'"):
        hs.Probe.on(o["lb"], "current_count")


def test_the_pool_is_the_documented_bound():
    """P = R * A: A = max_instances - initial backends, R runs of scale-outs that begin g_in + g_out instants apart."""
    lb = hs.LoadBalancer("lb")
    mk = lambda **kw: hs.AutoScaler("s", lb, None, **kw)  # noqa: E731
    s = 10 ** 9
    # the reference's defaults over an hour: 362 instants, gaps of 2 and 5 instants, 52 runs of at most 9 instances
    assert scaler_pool_size(mk(), 1, 0, 3600 * s) == (1 + 361 // 7) * 9 == 468
    assert scaler_pool_size(mk(max_instances=4, evaluation_interval=0.5, scale_out_cooldown=0.0, scale_in_cooldown=0.0), 1, 0, 5 * s) == (1 + 11 // 2) * 3
    assert scaler_pool_size(mk(max_instances=4, evaluation_interval=0.5, scale_out_cooldown=0.0, scale_in_cooldown=0.0), 1, 0, 5 * s, starts=2) == 12 * 2 * 3
    assert scaler_pool_size(mk(max_instances=4, evaluation_interval=0.5, scale_out_cooldown=0.5, scale_in_cooldown=0.5), 1, 0, 5 * s, starts=2) == (1 + 11 // 2) * 3
    assert scaler_pool_size(mk(max_instances=3), 3, 0, 3600 * s) == 0 and scaler_pool_size(mk(max_instances=3), 5, 0, 3600 * s) == 0
    assert scaler_pool_size(mk(max_instances=2, evaluation_interval=1.0), 1, 5 * s, 4 * s) == 1     # an end before the start: two instants
    # no recorded run of the reference created more instances than the pool holds, and some came close to a third of it
    used = []
    for spec in AS.all_specs():
        sim, pools = AS.build(spec)
        g = sim.lowered()
        ref = AR.get("case", spec)
        for i, sc in enumerate(pools["scaler"]):
            node = g.node_of[id(sc)]
            size = int(g.arrays.as_params[node, 8])
            n_init = len(sc.load_balancer.all_backends)
            assert size == scaler_pool_size(sc, n_init, int(spec.get("start_ns", 0)), int(spec.get("start_ns", 0)) + int(spec["end_s"] * 1e9),
                                            spec["scalers"][i]["starts"])
            assert ref["as_state"][i, 6] <= size
            if size:
                used.append(ref["as_state"][i, 6] / size)
    assert max(used) >= 0.3


def test_the_lowered_arrays():
    spec = AS.FIXTURES["two_scaled_load_balancers"]
    sim, pools = AS.build(spec)
    g = sim.lowered()
    a = g.arrays
    assert isinstance(g, GeneralGraph) and sim._station_refusal == "the station, network and pipeline engines do not lower an AutoScaler"
    # the Simulation's own nodes first (Sources, then the entities in their order), the pools behind them, scaler by scaler
    own = pools["source"] + pools["server"] + pools["lb"] + pools["sink"] + pools["scaler"]
    assert g.nodes[:g.n_own] == own and g.n_own == len(own)
    sizes = [int(a.as_params[g.node_of[id(sc)], 8]) for sc in pools["scaler"]]
    assert a.n == g.n_own + sum(sizes) and all(sz > 0 for sz in sizes)
    at = g.n_own
    for i, (sc, size) in enumerate(zip(pools["scaler"], sizes)):
        node, lb_node = g.node_of[id(sc)], g.node_of[id(sc.load_balancer)]
        assert a.kind[node] == N.NODE_AUTO_SCALER and a.target[node] == lb_node
        assert g.nodes[at:at + size] == pools["factory"][i].made == sc._pool and [s.name for s in sc._pool] == [f"as{i}_server_{k + 1}" for k in range(size)]
        assert (a.kind[at:at + size] == N.NODE_SERVER).all()
        # instance k: the Servers' SERVICE numbering goes on behind the Servers the Simulation lists
        assert a.stream_base[at:at + size].tolist() == [len(pools["server"]) + k for k in range(size)]
        off, cnt = int(a.rt_off[lb_node]), int(a.rt_cnt[lb_node])
        n_init = len(sc.load_balancer.all_backends)
        assert cnt == n_init + size and a.rt_targets[off + n_init:off + cnt].tolist() == list(range(at, at + size))
        assert a.rt_targets[off:off + n_init].tolist() == [g.node_of[id(b)] for b in sc.load_balancer.all_backends]
        sc_spec = spec["scalers"][i]
        assert a.as_params[node].tolist() == [N.AUTOSCALER_TARGET_UTILIZATION if sc_spec["policy"][0] == "tu" else N.AUTOSCALER_QUEUE_DEPTH,
                                              *([sc_spec["policy"][1], 0.0] if sc_spec["policy"][0] == "tu" else sc_spec["policy"][1:]),
                                              sc_spec["lo"], sc_spec["hi"], sc_spec["iv"], sc_spec["out_cd"], sc_spec["in_cd"], size, 1.0]
        at += size
    assert a.lb_healthy is not None and a.lb_healthy.all() and a.has_health and a.has_scalers
    assert (a.stream_base[[g.node_of[id(s)] for s in pools["server"]]] == [0, 1]).all()
    # the factory is called once per instance, also when the graph is lowered again
    sim2, _ = AS.build(spec)
    assert [len(f.made) for f in pools["factory"]] == sizes
    # StepScaling: the steps as the host sorted them
    sim, pools = AS.build(AS.FIXTURES["step_scaling_scales_out_and_in"])
    g = sim.lowered()
    node = g.node_of[id(pools["scaler"][0])]
    assert g.arrays.as_steps[node] == [(0.9, 2), (0.5, 1), (0.0, -1)] and g.arrays.as_params[node, 0] == N.AUTOSCALER_STEP
    # a Probe on current_count
    sim, pools = AS.build(AS.FIXTURES["probe_on_current_count"])
    g = sim.lowered()
    probe_nodes = np.nonzero(g.arrays.kind == N.NODE_PROBE)[0]
    assert g.arrays.probe_metric[probe_nodes].tolist() == [N.PROBE_METRICS["depth"], N.PROBE_SCALER_METRICS["current_count"]]
    assert g.arrays.target[probe_nodes[1]] == g.node_of[id(pools["scaler"][0])]


def test_parts_hold_a_pool_with_its_load_balancer():
    spec = AS.groups_spec(16)
    sim, pools = AS.build(spec)
    g = sim.lowered()
    parts = split_parts(g.arrays)
    assert len(parts) == 16
    for ids, _pos, b in parts:
        (sc_node,) = np.nonzero(b.kind == N.NODE_AUTO_SCALER)[0]
        lb_node = int(b.target[sc_node])
        size = int(b.as_params[sc_node, 8])
        assert b.kind[lb_node] == N.NODE_LB and b.rt_cnt[lb_node] == 1 + size and (b.kind == N.NODE_SERVER).sum() == 1 + size
        assert b.n == 5 + size and b.lb_healthy is not None and len(b.as_steps) == b.n
        assert [g.pool_of[int(i)][1] for i in ids if int(i) in g.pool_of] == list(range(1, size + 1))


def test_what_the_recordings_cover():
    """Conditions on what the live reference did (the recorder asserts the named fixtures one by one)."""
    refs = [AR.get("case", s) for s in AS.all_specs()]
    state = np.concatenate([r["as_state"] for r in refs])
    assert (state[:, 5] > 0).sum() >= 10 and (state[:, 1] > 0).sum() >= 60 and (state[:, 2] > 0).sum() >= 60      # blocks, outs, ins
    assert (state[:, 4] > state[:, 3]).any()                               # instances_removed counts what was asked, not what left
    assert (state[:, 6] > state[:, 11]).sum() >= 30                        # ids are never handed out again
    assert any((r["as_instance_total_requests"] == -1).any() for r in refs) and all(r["python"][:2] < [3, 12] for r in refs)
    assert max(r["as_state"][:, 10].max() for r in refs) >= 66


def test_existing_lowering_is_unchanged_without_a_scaler():
    """The node arrays of the existing families' graphs, byte for byte what the parent commit lowered them to."""
    h = hashlib.sha256()
    specs = [(MX.build, s) for s in MX.FIXTURES.values()] + [(MX.build, MX.random_spec(k)) for k in range(0, 150, 7)]
    specs += [(LS.build, s) for s in LS.FIXTURES.values()] + [(QS.build, s) for s in list(QS.FIXTURES.values())[::3]]
    for build, spec in specs:
        sim, _pools = build(spec)
        g = sim.lowered()
        if not isinstance(g, GeneralGraph):
            continue
        a = g.arrays
        assert not a.has_scalers and g.n_own == a.n and not g.pool_of
        h.update(spec["name"].encode())
        h.update(",".join(type(x).__name__ + ":" + x.name for x in g.nodes).encode())
        for name in sorted(vars(a)):
            v = getattr(a, name)
            if name.startswith("as_") or name.startswith("_"):
                continue
            h.update(name.encode())
            h.update(b"-" if v is None else v if isinstance(v, bytes) else str(v).encode() if isinstance(v, int) else np.ascontiguousarray(v).tobytes())
    assert h.hexdigest() == "e0e7b0a6f6ab70ae0d71af7411627179eced991cd318e1f585ae365c0abaacb2"
