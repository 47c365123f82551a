"""Host side of Hedge and Fallback (no GPU): the constructors and the reference's ValueError texts, every refusal by its text, the
lowering of every recorded spec, the coverage of the recordings under tests/golden/live_hedge/ (computed from the files alone), the
default table capacity in the sources and the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import happy_simulator_amd as hs
import hedge_specs as HG
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_arrays import split_parts
from happy_simulator_amd.lowering import UnsupportedTopology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(make, **sim_kw):
    """Source -> make(server, sink) -> ...: a Simulation over whatever `make` returns as (first entity, other entities)."""
    sink = hs.Sink("sink")
    server = hs.Server("srv", service_time=hs.ConstantLatency(0.01), downstream=sink)
    first, others = make(server, sink)
    src = hs.Source.constant(rate=5.0, target=first, name="src")
    return hs.Simulation(sources=[src], entities=[server, sink, first] + list(others), end_time=hs.Instant.from_seconds(1.0), **sim_kw)


def _refused(make, text, **sim_kw):
    with pytest.raises(NotImplementedError, match=re.escape(text)) as err:
        _chain(make, **sim_kw).lowered()
    assert isinstance(err.value, UnsupportedTopology)


def test_constructors_and_the_references_value_errors():
    sink = hs.Sink("sink")
    h = hs.Hedge("hg", sink, 0.05)
    assert (h.name, h.target, h.hedge_delay, h.max_hedges, h.in_flight_count, h.downstream_entities()) == ("hg", sink, 0.05, 1, 0, [sink])
    assert h.stats == hs.HedgeStats(0, 0, 0, 0, 0) and h._in_flight == {} and h._next_request_id == 0
    assert [f for f in hs.HedgeStats.__dataclass_fields__] == ["total_requests", "primary_wins", "hedge_wins", "hedges_sent", "hedges_cancelled"]
    with pytest.raises(Exception):
        h.stats.hedge_wins = 1
    assert hs.Hedge("hg", sink, hedge_delay=1e-9, max_hedges=3).max_hedges == 3
    for delay in (0, -1.0):
        with pytest.raises(ValueError, match=re.escape(f"hedge_delay must be > 0, got {delay}")):
            hs.Hedge("hg", sink, delay)
    for n in (0, -2):
        with pytest.raises(ValueError, match=re.escape(f"max_hedges must be >= 1, got {n}")):
            hs.Hedge("hg", sink, 0.1, n)
    other = hs.Sink("other")
    f = hs.Fallback("fb", sink, other)
    assert (f.name, f.primary, f.fallback, f.timeout, f.downstream_entities()) == ("fb", sink, other, None, [sink, other])
    assert f.stats == hs.FallbackStats(0, 0, 0, 0, 0, 0) and f._in_flight == {} and f._next_request_id == 0
    assert [x for x in hs.FallbackStats.__dataclass_fields__] == ["total_requests", "primary_successes", "primary_failures", "fallback_invocations",
                                                                  "fallback_successes", "fallback_failures"]
    with pytest.raises(Exception):
        f.stats.total_requests = 1
    assert hs.Fallback("fb", sink, other, timeout=0.25).timeout == 0.25
    assert hs.Fallback("fb", sink, lambda event: None).downstream_entities() == [sink]       # (constructed like the reference's; not lowered)
    for timeout in (0, -0.5):
        with pytest.raises(ValueError, match=re.escape(f"timeout must be > 0 or None, got {timeout}")):
            hs.Fallback("fb", sink, other, timeout=timeout)


def test_a_simulation_with_either_wrapper_is_lowered_to_the_single_heap_loop():
    for make in (lambda server, sink: (hs.Hedge("hg", server, 0.05, 2), []),
                 lambda server, sink: (hs.Fallback("fb", server, sink, timeout=0.05), [])):
        sim = _chain(make)
        g = sim.lowered()
        a = g.arrays
        assert "Hedge or Fallback" in sim._station_refusal and a.has_hedges and "hg_params" not in vars(a) and "_hg_params" in vars(a)
        node = int(np.nonzero((a.kind == N.NODE_HEDGE) | (a.kind == N.NODE_FALLBACK))[0][0])
        if a.kind[node] == N.NODE_HEDGE:
            assert a.hg_params[node].tolist() == [50_000_000, 2, -1, 0] and a.target[node] == g.node_of[id(g.nodes[node].target)]
        else:
            assert a.hg_params[node].tolist() == [50_000_000, 0, g.node_of[id(g.nodes[node].fallback)], 0]
            assert a.target[node] == g.node_of[id(g.nodes[node].primary)]
    sim = _chain(lambda server, sink: (hs.Fallback("fb", server, sink), []))               # timeout=None is legal: never a fallback
    assert sim.lowered().arrays.hg_params[-1, 0] == -1
    # the delay is Duration.from_seconds of the mirror, in whole nanoseconds
    sim = _chain(lambda server, sink: (hs.Hedge("hg", server, 0.1 + 0.2), []))
    assert sim.lowered().arrays.hg_params[-1, 0] == hs.Duration.from_seconds(0.1 + 0.2).nanoseconds


def test_probe_on_a_hedge():
    sink = hs.Sink("sink")
    h = hs.Hedge("hg", sink, 0.05)
    probe, data = hs.Probe.on(h, "in_flight_count", interval=0.1)
    src = hs.Source.constant(rate=5.0, target=h, name="src")
    a = hs.Simulation(sources=[src], entities=[sink, h], probes=[probe], end_time=hs.Instant.from_seconds(1.0)).lowered().arrays
    assert a.probe_metric[1] == N.PROBE_HEDGE_METRICS["in_flight_count"] == 17
    with pytest.raises(NotImplementedError):
        hs.Probe.on(hs.Fallback("fb", sink, sink), "in_flight_count")


def test_refusals_by_name():
    lb = lambda server: hs.LoadBalancer("lb", backends=[server])  # noqa: E731
    _refused(lambda server, sink: (hs.Fallback("fb", server, sink, failure_predicate=lambda e: False), []),
             "Fallback 'fb': failure_predicate= is a host callable (not lowered)")
    _refused(lambda server, sink: (hs.Fallback("fb", server, lambda e: None, timeout=0.1), []),
             "Fallback 'fb': fallback= is a host callable, not an Entity (not lowered)")
    _refused(lambda server, sink: (hs.Hedge("hg", server, 0.1, 65_536), []),
             "Hedge 'hg': max_hedges = 65536 is beyond the 65535 hedges a request's entry counts on the engine (Hedge.MAX_HEDGES)")
    # as a LoadBalancer's backend
    _refused(lambda server, sink: (hs.LoadBalancer("lb", backends=[hs.Hedge("hg", server, 0.1)]), []),
             "backend 'hg' of 'lb' is a Hedge: only Server backends are lowered")
    _refused(lambda server, sink: (hs.LoadBalancer("lb", backends=[hs.Fallback("fb", server, sink)]), []),
             "backend 'fb' of 'lb' is a Fallback: only Server backends are lowered")
    # two completion hooks on one Event, directly and through NetworkLinks
    two = " -- two completion hooks on one Event are not lowered (a follow-up)"
    link = lambda name, to: hs.NetworkLink(name, latency=hs.ConstantLatency(0.01), egress=to)  # noqa: E731
    inner = {"LoadBalancer": lambda server, sink: lb(server), "Bulkhead": lambda server, sink: hs.Bulkhead("x", server, 2),
             "TimeoutWrapper": lambda server, sink: hs.TimeoutWrapper("x", server, 0.1), "Client": lambda server, sink: hs.Client("x", server),
             "Hedge": lambda server, sink: hs.Hedge("x", server, 0.1), "Fallback": lambda server, sink: hs.Fallback("x", server, sink)}
    for kind, make_inner in inner.items():
        name = "lb" if kind == "LoadBalancer" else "x"
        _refused(lambda server, sink: (hs.Hedge("hg", make_inner(server, sink), 0.1), []), f"Hedge 'hg': its target is the {kind} '{name}'" + two)
        _refused(lambda server, sink: (hs.Hedge("hg", link("l1", link("l2", make_inner(server, sink))), 0.1), []),
                 f"Hedge 'hg': its target (through its NetworkLinks) is the {kind} '{name}'" + two)
        _refused(lambda server, sink: (hs.Fallback("fb", make_inner(server, sink), sink), []), f"Fallback 'fb': its primary is the {kind} '{name}'" + two)
        _refused(lambda server, sink: (hs.Fallback("fb", server, link("l1", make_inner(server, sink))), []),
                 f"Fallback 'fb': its fallback entity (through its NetworkLinks) is the {kind} '{name}'" + two)
    flow = " -- a completion hook on an item that a BatchProcessor, ConveyorBelt or GateController holds is not lowered (a follow-up)"
    for kind, make_inner in (("BatchProcessor", lambda sink: hs.BatchProcessor("x", sink, batch_size=2)), ("ConveyorBelt", lambda sink: hs.ConveyorBelt("x", sink, 0.1)),
                             ("GateController", lambda sink: hs.GateController("x", sink))):
        _refused(lambda server, sink: (hs.Hedge("hg", make_inner(sink), 0.1), []), f"Hedge 'hg': its target is the {kind} 'x'" + flow)
        _refused(lambda server, sink: (hs.Fallback("fb", server, link("l1", make_inner(sink))), []),
                 f"Fallback 'fb': its fallback entity (through its NetworkLinks) is the {kind} 'x'" + flow)
    # an older wrapper or a Client in front of either
    for what, make_outer in (("Bulkhead 'w'", lambda t: hs.Bulkhead("w", t, 2)), ("TimeoutWrapper 'w'", lambda t: hs.TimeoutWrapper("w", t, 0.1)),
                             ("Client 'w'", lambda t: hs.Client("w", t))):
        _refused(lambda server, sink: (make_outer(hs.Hedge("hg", server, 0.1)), []), f"{what}: its target is the Hedge 'hg'" + two)
        _refused(lambda server, sink: (make_outer(link("l1", hs.Fallback("fb", server, sink))), []),
                 f"{what}: its target (through its NetworkLinks) is the Fallback 'fb'" + two)
    # a target that takes no Requests
    probe_target = hs.Sink("elsewhere")
    _refused(lambda server, sink: (hs.Hedge("hg", hs.Source.constant(rate=1.0, target=sink, name="s2"), 0.1), []), "a Source takes no Requests")
    _refused(lambda server, sink: (hs.Fallback("fb", server, hs.Probe.on(probe_target, "events_received")[0]), []),
             "'fb' forwards to it: Probe 'Probe_elsewhere_events_received' is not lowered to the engine")
    _refused(lambda server, sink: (hs.Hedge("hg", hs.HealthChecker("hc", lb(server)), 0.1), []), "the HealthChecker 'hc' takes no Requests")


def test_refused_in_a_parallel_simulation_partition():
    sink = hs.Sink("sink")
    for ent, kind in ((hs.Hedge("hg", sink, 0.1), "Hedge"), (hs.Fallback("fb", sink, sink, timeout=0.1), "Fallback")):
        src = hs.Source.constant(rate=5.0, target=ent, name="src")
        part = hs.SimulationPartition(name="p0", entities=[sink, ent], sources=[src])
        with pytest.raises(NotImplementedError, match=re.escape(f"partition 'p0': the {kind} '{ent.name}' on a ParallelSimulation partition is not lowered "
                                                                "(Hedge and Fallback run on the single-heap loop: pass it to a Simulation)")):
            hs.ParallelSimulation(partitions=[part], duration=1.0)


def test_faults_may_name_either_wrapper():
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("hg", at=0.2, restart_at=0.5))
    fs.add(hs.PauseNode("fb", start=0.1, end=0.3))
    sink = hs.Sink("sink")
    server = hs.Server("srv", service_time=hs.ConstantLatency(0.01), downstream=sink)
    f = hs.Fallback("fb", server, sink, timeout=0.05)
    h = hs.Hedge("hg", server, 0.05)
    srcs = [hs.Source.constant(rate=5.0, target=h, name="s0"), hs.Source.constant(rate=5.0, target=f, name="s1")]
    sim = hs.Simulation(sources=srcs, entities=[server, sink, h, f], fault_schedule=fs, end_time=hs.Instant.from_seconds(1.0))
    g = sim.lowered()
    assert sorted(n for n, *_ in sim._general_faults(g)) == sorted([g.node_of[id(h)]] * 2 + [g.node_of[id(f)]] * 2)


def test_the_fallback_edge_is_an_edge_of_the_graph():
    """split_parts and the walks over downstream_entities() see a Fallback's second edge: a fallback entity that nothing else reaches
    is a node of the graph, in the part of its wrapper."""
    spec = HG.groups_spec()
    sim, pools = HG.build(spec)
    g = sim.lowered()
    parts = split_parts(g.arrays)
    assert len(parts) == 16
    for f in pools["fallback"]:
        ids = next(ids for ids, _pos, _b in parts if g.node_of[id(f)] in ids)
        assert g.node_of[id(f.fallback)] in ids and g.node_of[id(f.primary)] in ids
    for ids, _pos, b in parts:
        fb = np.nonzero(b.kind == N.NODE_FALLBACK)[0]
        assert b.has_hedges and (b.hg_params[fb, 2] < b.n).all()
        for i in fb:                                           # renumbered into the part: the fallback entity is the Server in front of the group's Sink
            assert b.kind[b.hg_params[i, 2]] == N.NODE_SERVER and b.kind[b.target[b.hg_params[i, 2]]] == N.NODE_SINK
    # a fallback entity listed nowhere else is discovered through the wrapper
    sink, only = hs.Sink("sink"), hs.Sink("only_the_fallback_knows_me")
    f = hs.Fallback("fb", sink, only, timeout=0.1)
    src = hs.Source.constant(rate=5.0, target=f, name="src")
    g = hs.Simulation(sources=[src], entities=[f], end_time=hs.Instant.from_seconds(1.0)).lowered()
    assert id(only) in g.node_of and id(sink) in g.node_of
    # a part without either wrapper drops the family
    plain = hs.Sink("plain_sink")
    src2 = hs.Source.constant(rate=5.0, target=plain, name="src2")
    g = hs.Simulation(sources=[src, src2], entities=[f, plain], end_time=hs.Instant.from_seconds(1.0)).lowered()
    assert sorted(bool(b.has_hedges) for _ids, _pos, b in split_parts(g.arrays)) == [False, True]


def test_every_spec_is_recorded_and_lowers():
    specs = HG.recorded_specs()
    assert len(specs) == len(HG.FIXTURES) + HG.N_RANDOM + 2 and len({s["name"] for s in specs}) == len(specs)
    for spec in specs:
        ref = HG.HEDGE.get("case", spec)                       # (KeyError names the case and the recorder)
        sim, pools = HG.build(spec)
        g = sim.lowered()                                      # refuses nothing
        a = g.arrays
        assert a.has_hedges and int(((a.kind == N.NODE_HEDGE) | (a.kind == N.NODE_FALLBACK)).sum()) == len(pools["hedge"]) + len(pools["fallback"])
        assert len(ref["by_kind"]) == HG.N_KINDS and ref["total_events"] <= 60_000 and spec["end_s"] <= 5.0
        assert len(ref["hg_stats"]) == len(pools["hedge"]) and len(ref["fb_stats"]) == len(pools["fallback"])
        assert ref["hg_params"] == [[h.target.name, h.hedge_delay, h.max_hedges] for h in pools["hedge"]]
        assert ref["fb_params"] == [[f.primary.name, f.fallback.name, f.timeout] for f in pools["fallback"]]
        assert ("trace" in ref) == (spec["name"] in HG.TRACED)
    for path in os.listdir(HG.HEDGE.rec_dir):
        assert os.path.getsize(os.path.join(HG.HEDGE.rec_dir, path)) <= HG.HEDGE.max_part_bytes < (1 << 20)


def test_coverage_of_the_recordings():
    """Computed from the files alone: each of the seven kinds occurs in at least 20 cases; cancelled hedges, winning hedges, a leaked
    entry, a response and a send-hedge on one nanosecond and a late primary response in at least 5 cases each."""
    refs = [HG.HEDGE.get("case", spec) for spec in HG.recorded_specs()]
    per_kind = np.sum([r["by_kind"][HG.EV_HG_FIRST:] > 0 for r in refs], axis=0)
    assert len(per_kind) == 7 and (per_kind >= 20).all(), per_kind
    assert sum(1 for r in refs if (r["hg_stats"][:, 4] > 0).any()) >= 5
    assert sum(1 for r in refs if (r["hg_stats"][:, 2] > 0).any()) >= 5
    assert sum(1 for r in refs if HG.leaked(r)) >= 5
    assert sum(1 for r in refs if r["same_ns_pairs"] > 0) >= 5
    assert sum(1 for r in refs if r["late_primary"] > 0) >= 5
    # the reference never counts a fallback failure; a Hedge's ids are handed out once per Request
    assert all((r["fb_stats"][:, 5] == 0).all() and (r["hg_stats"][:, 0] == r["hg_stats"][:, 5]).all() for r in refs)
    # same-nanosecond pairs in the traces themselves: a `_hg_response` and a `_hg_send_hedge` of one node on one nanosecond
    seen = 0
    for name in HG.TRACED:
        tr = HG.HEDGE.get("case", HG.FIXTURES[name])["trace"]
        resp, send = tr[tr[:, 1] == HG.EV_HG_FIRST + 1], tr[tr[:, 1] == HG.EV_HG_FIRST + 2]
        seen += bool(set(map(tuple, resp[:, [0, 2]].tolist())) & set(map(tuple, send[:, [0, 2]].tolist())))
    assert seen >= 5


def test_default_table_capacity_in_the_sources():
    src = open(os.path.join(ROOT, "happy_simulator_amd", "csrc", "hs_graph.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    assert re.search(r"constexpr int kDefaultHedgeTable = 256;", src)
    assert "table_capacity > 0 ? table_capacity : kDefaultHedgeTable" in src
    assert "the entries the table holds at first (0: 256)" in hdr
    assert re.search(r"#define HS_HEDGE_MAX_IN_FLIGHT \(1 << 20\)", hdr) and N.HEDGE_MAX_IN_FLIGHT == 1 << 20
    assert re.search(r"#define HS_HEDGE_MAX_HEDGES 65535\b", hdr) and N.HEDGE_MAX_HEDGES == hs.Hedge.MAX_HEDGES == 65535
    assert re.search(r"HS_NODE_HEDGE = 18,", hdr) and re.search(r"HS_NODE_FALLBACK = 19\b", hdr) and (N.NODE_HEDGE, N.NODE_FALLBACK) == (18, 19)
    assert re.search(r"HS_PROBE_HG_IN_FLIGHT = 17,", hdr)
    assert re.search(r"#define HS_HEDGE_KINDS 7\b", hdr) and N.HEDGE_KINDS == 7
    # seven internal kinds behind the canary deployer's: 60 of the 64 one drop mask of two words holds
    assert "kEvHgKinds = kEvCnKinds + HS_HEDGE_KINDS" in src and 'static_assert(kEvHgKinds <= 64, "kDropKindsHg is two words' in src
    assert HG.N_KINDS == 60


def test_new_abi_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    for sym in ("hs_graph_set_hedge", "hs_graph_set_fallback", "hs_graph_get_hedge", "hs_graph_get_fallback"):
        assert re.search(rf"\bint {sym}\(hs_graph \*g", hdr) and sym in N.EXPORTED_SYMBOLS
    assert N.ABI_VERSION == 16
    for name in ("Hedge", "HedgeStats", "Fallback", "FallbackStats"):
        assert hasattr(hs, name)
