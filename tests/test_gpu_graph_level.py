"""GPU: the level of the single-heap loop a graph runs at (csrc/hs_graph.hip level_of / hs_graph_level).  A lone run takes the lowest
level that dispatches all the graph's kinds; a batch (hs_graph_run_many, hs_graph_run_parts) takes the highest level of its handles --
neither a level too low (the loop would meet a kind it does not dispatch) nor one too high (the same results from a slower kernel,
which no comparison of results sees).  Every case is the smallest graph that forces its level, run for 0.1 s."""
import numpy as np
import pytest

import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GraphEngine, PartRun, split_parts

pytestmark = pytest.mark.gpu
END_S = 0.1


def _svc():
    return hs.ExponentialLatency(0.005)


def _sim(first, entities, rate=200.0, fault=None, **kw):
    fs = None
    if fault is not None:
        fs = hs.FaultSchedule()
        fs.add(fault)
    return hs.Simulation(sources=[hs.Source.poisson(rate=rate, target=first, name="src")], entities=entities, fault_schedule=fs,
                         end_time=hs.Instant.from_seconds(END_S), seed=11, **kw)


def _chain(wrap=None, server_kw=None, fault=None, rate=200.0, tag=""):
    """Source -> [wrap(Server)] -> Server -> Sink"""
    sink = hs.Sink("sink" + tag)
    srv = hs.Server("srv" + tag, service_time=_svc(), downstream=sink, **(server_kw or {}))
    first = wrap(srv) if wrap else srv
    return _sim(first, [srv, sink] + ([first] if wrap else []), rate=rate, fault=fault)


def _pool(n, manage=None, check=False):
    """Source -> LoadBalancer over `n` Servers -> Sink, with what `manage(lb, factory)` puts over the LoadBalancer"""
    sink = hs.Sink("sink")
    servers = [hs.Server(f"srv{i}", service_time=_svc(), downstream=sink) for i in range(n)]
    lb = hs.LoadBalancer("lb", backends=servers)
    extra = []
    if check:
        extra.append(hs.HealthChecker("hc", lb, interval=0.04, timeout=0.02))
    if manage:
        extra.append(manage(lb, lambda name: hs.Server(name, service_time=_svc(), downstream=sink)))
    sim = _sim(lb, servers + [lb, sink] + extra)
    for x in extra:
        sim.schedule(x.start() if hasattr(x, "start") else x.deploy())
    return sim


def _link_fault():
    """Source -> NetworkLink -> Server -> Sink with an InjectLatency on the link"""
    sink = hs.Sink("sink")
    srv = hs.Server("srv", service_time=_svc(), downstream=sink)
    link = hs.NetworkLink("link", latency=hs.ConstantLatency(0.002))
    net = hs.Network("net")
    net.add_link(link, srv, link)                  # (registered as ("link", "srv"): the fault finds it by these names)
    return _sim(link, [srv, link, sink, net], fault=hs.InjectLatency("link", "srv", 5.0, 0.02, 0.06))


LONE = {
    "plain": (N.GRAPH_LEVEL_PLAIN, lambda: _chain()),
    "crash_node": (N.GRAPH_LEVEL_FAULTS, lambda: _chain(fault=hs.CrashNode("srv", at=0.05))),
    "health_checker": (N.GRAPH_LEVEL_HEALTH, lambda: _pool(2, check=True)),
    "bulkhead": (N.GRAPH_LEVEL_RESILIENCE, lambda: _chain(lambda srv: hs.Bulkhead("bh", srv, max_concurrent=2))),
    "client": (N.GRAPH_LEVEL_CLIENT, lambda: _chain(lambda srv: hs.Client("cl", srv, timeout=0.5))),
    "gate_controller": (N.GRAPH_LEVEL_FLOW, lambda: _chain(lambda srv: hs.GateController("gate", srv))),
    "lifo_queue": (N.GRAPH_LEVEL_QUEUES, lambda: _chain(server_kw=dict(queue_policy=hs.LIFOQueue()))),
    "inject_latency": (N.GRAPH_LEVEL_LINK_FAULTS, _link_fault),
    "auto_scaler": (N.GRAPH_LEVEL_SCALER, lambda: _pool(1, lambda lb, mk: hs.AutoScaler("scaler", lb, mk, evaluation_interval=0.03))),
    "rolling_deployer": (N.GRAPH_LEVEL_DEPLOY, lambda: _pool(1, lambda lb, mk: hs.RollingDeployer("roll", lb, mk))),
    "hedge": (N.GRAPH_LEVEL_HEDGE, lambda: _chain(lambda srv: hs.Hedge("hg", srv, 0.004))),
    # ... and two that guard the order of the ladder's rungs
    "canary_deployer_alone": (N.GRAPH_LEVEL_DEPLOY, lambda: _pool(1, lambda lb, mk: hs.CanaryDeployer("can", lb, mk))),
    "client_and_fault": (N.GRAPH_LEVEL_CLIENT, lambda: _chain(lambda srv: hs.Client("cl", srv, timeout=0.5), fault=hs.CrashNode("srv", at=0.05))),
}


def _engine(sim):
    """The Simulation on a single-heap engine of its own (not yet run), set up as Simulation.run() sets it up; (engine, end ns)."""
    g = sim._lower_general()                       # (the plain chain too: Simulation.run() would hand it to the station engines)
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, False)
    assert not cancelled
    return sim._general_engine(g, start_ns, sched, record_capacity=4096), end_ns


def _level(eng, which):
    return eng._lib.hs_graph_level(eng._h, which)


def _results(eng):
    s = eng.summary()
    return ([s.events_processed, s.final_time_ns, s.requests_completed, s.sink_records] + list(s.events_by_kind), [x.tolist() for x in eng.records()])


def test_the_mirrored_constants_are_the_ladder():
    names = ("PLAIN", "FAULTS", "HEALTH", "RESILIENCE", "CLIENT", "FLOW", "QUEUES", "LINK_FAULTS", "SCALER", "DEPLOY", "HEDGE")
    assert [getattr(N, "GRAPH_LEVEL_" + nm) for nm in names] == list(range(11))
    assert len({want for want, _ in LONE.values()}) == 11                               # the lone cases force every level


@pytest.mark.parametrize("name", list(LONE))
def test_a_lone_run_takes_the_lowest_level_that_dispatches_the_graphs_kinds(name):
    want, make = LONE[name]
    eng, end_ns = _engine(make())
    with eng:
        assert _level(eng, 0) == want
        assert _level(eng, 1) == -1                                                     # no launch yet
        assert _level(eng, 2) == -1 and _level(eng, -1) == -1                           # (no such question)
        eng.run_until(end_ns)
        assert _level(eng, 1) == want and _level(eng, 0) == want
        assert eng.summary().events_processed > 0


@pytest.mark.parametrize("other, want", [("hedge", N.GRAPH_LEVEL_HEDGE), ("crash_node", N.GRAPH_LEVEL_FAULTS)])
def test_a_batch_takes_the_highest_level_of_its_handles_and_no_higher(other, want):
    """... and the plain handle computes in it, bit for bit, what a plain handle run alone computes."""
    plain, end_ns = _engine(LONE["plain"][1]())
    high, end_high = _engine(LONE[other][1]())
    alone, _ = _engine(LONE["plain"][1]())
    with plain, high, alone:
        assert end_high == end_ns and _level(plain, 0) == N.GRAPH_LEVEL_PLAIN and _level(high, 0) == want
        GraphEngine.run_many([plain, high], end_ns)
        assert _level(plain, 1) == want and _level(high, 1) == want
        assert _level(plain, 0) == N.GRAPH_LEVEL_PLAIN                                  # (what it holds has not changed)
        alone.run_until(end_ns)
        assert _level(alone, 1) == N.GRAPH_LEVEL_PLAIN
        got, ref = _results(plain), _results(alone)
        assert got == ref and ref[0][0] > 0 and len(ref[1][0]) > 0


def _two_parts(plain_rate, client_rate):
    """One Simulation of two groups no Request crosses -- a plain chain and one behind a Client -- as the engines of its parts."""
    sink_a, sink_b = hs.Sink("sink_a"), hs.Sink("sink_b")
    srv_a = hs.Server("srv_a", service_time=_svc(), downstream=sink_a)
    srv_b = hs.Server("srv_b", service_time=_svc(), downstream=sink_b)
    cl = hs.Client("cl", srv_b, timeout=0.5)
    sim = hs.Simulation(sources=[hs.Source.constant(rate=plain_rate, target=srv_a, name="src_a"),
                                 hs.Source.constant(rate=client_rate, target=cl, name="src_b")],
                        entities=[srv_a, sink_a, srv_b, sink_b, cl], end_time=hs.Instant.from_seconds(END_S), seed=11)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, False)
    parts = split_parts(g.arrays, 2)
    assert not sched and not cancelled and parts is not None and len(parts) == 2
    engines = [GraphEngine(b, seed=11, start_ns=start_ns, record_capacity=4096) for _ids, _pos, b in parts]
    has_client = [bool((b.kind == N.NODE_CLIENT).any()) for _ids, _pos, b in parts]
    assert sorted(has_client) == [False, True]
    return PartRun(g.arrays, parts, engines), engines[has_client.index(False)], engines[has_client.index(True)], end_ns


def test_parts_run_side_by_side_at_the_highest_level_of_the_parts():
    """hs_graph_run_parts: the batch launch runs every part at the Client part's level.  The one event beyond the end is the Client
    part's here (its Source's next tick, at 0.1043 s, stands in front of the plain part's, at 0.108 s): the single step that processes
    it is a launch of that part alone, at its own level -- the same level."""
    run, plain, client, end_ns = _two_parts(plain_rate=37.0, client_rate=211.0)
    try:
        assert _level(plain, 0) == N.GRAPH_LEVEL_PLAIN and _level(client, 0) == N.GRAPH_LEVEL_CLIENT
        assert run.run(end_ns)                                                          # (decided: no part's timestamp group is mixed)
        assert _level(plain, 1) == N.GRAPH_LEVEL_CLIENT and _level(client, 1) == N.GRAPH_LEVEL_CLIENT
        assert plain.summary().final_time_ns <= end_ns < client.summary().final_time_ns   # the Client part took the step beyond the end
    finally:
        for e in run.engines:
            e.close()


def test_the_step_beyond_the_end_is_a_launch_of_the_elected_part_at_its_own_level():
    """The rates the other way round: the plain part holds the earliest event beyond the end, and its most recent launch is the
    single step -- the plain kernel, as before there were levels; the Client part's stays the batch launch."""
    run, plain, client, end_ns = _two_parts(plain_rate=211.0, client_rate=37.0)
    try:
        assert run.run(end_ns)
        assert _level(client, 1) == N.GRAPH_LEVEL_CLIENT and _level(plain, 1) == N.GRAPH_LEVEL_PLAIN
        assert client.summary().final_time_ns <= end_ns < plain.summary().final_time_ns
    finally:
        for e in run.engines:
            e.close()
