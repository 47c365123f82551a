"""Host side of health checks (no GPU): the mirrors of HealthChecker / HealthCheckStats / BackendHealthState and the LoadBalancer's
marks against the recorded live reference (tests/golden/live_health/), what the lowering hands to the single-heap loop for every
spec, and the named refusals."""
import dataclasses

import numpy as np
import pytest

import graph_family as GF
import health_specs as HS
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph
from recorded import HEALTH as HR


def _pool(strategy=None, n=2):
    sink = hs.Sink("sink")
    servers = [hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink) for i in range(n)]
    lb = hs.LoadBalancer("lb", backends=servers, strategy=strategy)
    src = hs.Source.poisson(rate=5, target=lb, name="src")
    return src, lb, servers, sink


def test_mirrors_equal_the_recorded_defaults():
    ref = HR.get("defaults")
    lb = hs.LoadBalancer("lb", backends=[hs.Server("a"), hs.Server("b")])
    hc = hs.HealthChecker("hc", lb)
    st, bs = hc.stats, hc.get_backend_state(lb.all_backends[0])
    assert [hc.interval, hc.timeout, hc.healthy_threshold, hc.unhealthy_threshold, hc._check_event_type, hc.is_running] == ref["fields"]
    assert (hc.load_balancer is lb) == ref["lb_is"] and [x.name for x in hc.downstream_entities()] == ref["downstream"]
    assert type(st).__name__ == ref["stats_type"] and [f.name for f in dataclasses.fields(st)] == ref["stats_fields"]
    assert [st.checks_performed, st.checks_passed, st.checks_failed, st.checks_timed_out, st.backends_marked_healthy,
            st.backends_marked_unhealthy] == ref["stats"]
    assert type(bs).__name__ == ref["state_type"] and [f.name for f in dataclasses.fields(bs)] == ref["state_fields"]
    assert [bs.consecutive_successes, bs.consecutive_failures, bs.last_check_time is None, bs.last_check_passed is None, bs.is_checking] == ref["state"]
    assert (hc.get_backend_state_by_name("nobody") is None) == ref["state_by_unknown_name"]
    with pytest.raises(dataclasses.FrozenInstanceError) as e:
        st.checks_performed = 1
    assert type(e.value).__name__ == ref["stats_frozen"]
    ev = hc.start()
    assert dict(event_type=ev.event_type, time_ns=ev.time.nanoseconds, target_is=ev.target is hc, daemon=ev.daemon, running=hc.is_running) == ref["start"]
    hc.stop()
    assert hc.is_running == ref["stopped"]


def test_value_errors_have_the_reference_texts():
    ref = HR.get("defaults")["errors"]
    lb = hs.LoadBalancer("lb", backends=[hs.Server("a")])
    got = []
    for kw in (dict(interval=0), dict(interval=-1.5), dict(timeout=0), dict(timeout=-2), dict(interval=1.0, timeout=1.0),
               dict(interval=1.0, timeout=2.5), dict(healthy_threshold=0), dict(unhealthy_threshold=0), dict(interval=0, timeout=0)):
        with pytest.raises(ValueError) as e:
            hs.HealthChecker("x", lb, **kw)
        got.append(str(e.value))
    assert got == ref and all(ref)


def test_load_balancer_marks_equal_the_recording():
    ref = HR.get("defaults")["marks"]
    lb = hs.LoadBalancer("lb", backends=[hs.Server("a"), hs.Server("b")])
    a, b = lb.all_backends
    lb.mark_unhealthy(a)
    lb.mark_unhealthy(a)
    lb.mark_unhealthy(hs.Server("stranger"))
    s1 = lb.stats
    assert [s1.backends_marked_unhealthy, s1.backends_marked_healthy, lb.healthy_count] == ref["after_unhealthy"]
    assert [x.name for x in lb.healthy_backends] == ref["healthy"] and [x.name for x in lb.unhealthy_backends] == ref["unhealthy"]
    assert [lb.get_backend_info(a).is_healthy, lb.get_backend_info(b).is_healthy] == ref["info"]
    lb.mark_healthy(a)
    lb.mark_healthy(b)
    s2 = lb.stats
    assert [s2.backends_marked_unhealthy, s2.backends_marked_healthy, lb.healthy_count] == ref["after_healthy"]


def test_the_lowering_accepts_every_spec():
    """Every recorded spec goes to the single-heap loop with its checker nodes, their parameters and the initial flags; none is left out."""
    specs = HS.all_specs()
    assert len(specs) == len(HS.FIXTURES) + HS.N_RANDOM
    for spec in specs:
        HR.get("case", spec)                                   # (recorded: a missing one raises by name)
        sim, pools = GF.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph) and g.arrays.has_health, spec["name"]
        a = g.arrays
        nodes = np.nonzero(a.kind == N.NODE_HEALTH_CHECKER)[0]
        assert len(nodes) == len(spec["checkers"])
        for i, ck, hc in zip(nodes, spec["checkers"], pools["checker"]):
            assert g.nodes[i] is hc and g.nodes[a.target[i]] is pools["lb"][ck["lb"]]
            running = bool(ck.get("starts", 1)) and not ck.get("stop")
            assert a.hc_params[i].tolist() == [ck["interval"], ck["timeout"], ck["ht"], ck["ut"], float(running)]
        for j, lb in enumerate(pools["lb"]):
            i = g.node_of[id(lb)]
            flags = a.lb_healthy[a.rt_off[i]:a.rt_off[i] + a.rt_cnt[i]].tolist()
            assert flags == [int([j, q] not in spec["unhealthy"]) for q in range(len(spec["lbs"][j]["backends"]))]
        _end, start_ns, sched, _c = sim._general_prepare(g, False)
        want = sum(0 if (ck.get("early") and spec.get("start_ns")) else ck.get("starts", 1) for ck in spec["checkers"])
        assert [n for n, _t in sched] == [n for n, ck in zip(nodes, spec["checkers"])
                                           for _ in range(0 if (ck.get("early") and spec.get("start_ns")) else ck.get("starts", 1))]
        assert len(sched) == want and all(t == start_ns for _n, t in sched)


def test_start_takes_its_time_from_the_simulation():
    src, lb, servers, sink = _pool()
    hc = hs.HealthChecker("hc", lb, interval=1.0, timeout=0.5)
    assert hc.start().time == hs.Instant.Epoch                  # no Simulation yet (health_check.py:212)
    sim = hs.Simulation(start_time=hs.Instant.from_seconds(3), end_time=hs.Instant.from_seconds(9), sources=[src], entities=servers + [lb, sink, hc])
    ev = hc.start()
    assert ev.time == hs.Instant.from_seconds(3) and ev.event_type == "_health_check_cycle" and ev.target is hc
    sim.schedule(ev)
    g = sim.lowered()
    assert sim._general_prepare(g, False)[2] == [(g.node_of[id(hc)], 3 * 10 ** 9)]
    assert "health" in sim._station_refusal


def test_an_unhealthy_backend_alone_sends_the_simulation_to_the_single_heap():
    src, lb, servers, sink = _pool()
    plain = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink])
    assert not isinstance(plain.lowered(), GeneralGraph)
    lb.mark_unhealthy(servers[0])
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink])
    g = sim.lowered()
    assert isinstance(g, GeneralGraph) and g.arrays.lb_healthy.tolist() == [0, 1] and g.arrays.hc_params is None
    assert lb.stats.backends_marked_unhealthy == 1 and lb.healthy_count == 1 and lb.unhealthy_backends == [servers[0]]


@pytest.mark.parametrize("strategy", [hs.ConsistentHash, hs.IPHash, hs.Random])
def test_hashed_and_random_strategies_are_refused_by_name(strategy):
    src, lb, servers, sink = _pool(strategy())
    hc = hs.HealthChecker("hc", lb, interval=1.0, timeout=0.5)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink, hc])
    with pytest.raises(hs.UnsupportedTopology, match=f"{strategy.__name__}.*under a HealthChecker"):
        sim.lowered()
    src, lb, servers, sink = _pool(strategy())
    lb.mark_unhealthy(servers[1])
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink])
    with pytest.raises(hs.UnsupportedTopology, match=f"{strategy.__name__} with an unhealthy backend \\('srv1'\\)"):
        sim.lowered()


def test_the_other_refusals_by_name():
    src, lb, servers, sink = _pool()
    hc, hc2 = hs.HealthChecker("hc", lb, interval=1.0, timeout=0.5), hs.HealthChecker("second", lb, interval=2.0, timeout=0.5)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink, hc, hc2])
    with pytest.raises(hs.UnsupportedTopology, match="'second'.*'lb' has the checker 'hc' already"):
        sim.lowered()
    # a checker whose LoadBalancer is not in the Simulation
    other = hs.LoadBalancer("elsewhere", backends=[hs.Server("x")])
    stray = hs.HealthChecker("stray", other, interval=1.0, timeout=0.5)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink, stray])
    with pytest.raises(hs.UnsupportedTopology, match="'stray': its LoadBalancer is not an entity of this Simulation"):
        sim.lowered()
    # a running checker never lets an auto-terminating run end
    src2, lb2, servers2, sink2 = _pool()
    hc3 = hs.HealthChecker("hc3", lb2, interval=1.0, timeout=0.5)
    sim = hs.Simulation(entities=servers2 + [lb2, sink2, hc3])
    sim.schedule(hc3.start())
    with pytest.raises(hs.UnsupportedTopology, match="running HealthChecker never terminates"):
        sim.run()
    # only the Event start() returns is lowered for a checker
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[src], entities=servers + [lb, sink, hc])
    sim.schedule(hs.Event(time=hs.Instant.Epoch, event_type="Request", target=hc))
    with pytest.raises(hs.UnsupportedTopology, match="only the Event start\\(\\) returns"):
        sim._general_prepare(sim.lowered(), False)
    # a checker takes no Requests: as somebody's downstream it is refused by name
    feeder = hs.Server("feeder", service_time=hs.ExponentialLatency(0.05), downstream=hc)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(2), sources=[hs.Source.poisson(rate=5, target=feeder, name="s2")],
                        entities=servers + [lb, sink, hc, feeder])
    with pytest.raises(hs.UnsupportedTopology, match="'feeder' forwards to it: the HealthChecker 'hc' takes no Requests"):
        sim.lowered()
    # a checker inside a ParallelSimulation partition
    part = hs.SimulationPartition(name="P0", entities=servers + [lb, sink, hc], sources=[src])
    with pytest.raises(hs.UnsupportedTopology, match="partition 'P0': the HealthChecker 'hc'"):
        hs.ParallelSimulation([part], end_time=hs.Instant.from_seconds(2))


def test_parts_keep_a_checker_with_its_load_balancer():
    from happy_simulator_amd.graph_engine import split_parts

    spec = HS.groups_spec(8)
    sim, pools = GF.build(spec)
    g = sim.lowered()
    parts = split_parts(g.arrays)
    assert len(parts) == 8
    for ids, _pos, b in parts:
        hc = np.nonzero(b.kind == N.NODE_HEALTH_CHECKER)[0]
        assert len(hc) == 1 and b.kind[b.target[hc[0]]] == N.NODE_LB and b.has_health
        assert b.hc_params[hc[0]].tolist() == [0.5, 0.2, 1.0, 2.0, 1.0] and b.lb_healthy.tolist() == [1, 1, 1]
