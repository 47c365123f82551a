"""Host side of Bulkhead and TimeoutWrapper (no GPU): the mirrors against the recorded live reference
(tests/golden/live_resilience/), what the lowering hands to the single-heap loop, and the named refusals."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import graph_family as GF
import resilience_specs as XS
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, split_parts
from recorded import RESILIENCE as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BH_ERRORS = (dict(max_concurrent=0), dict(max_concurrent=-2), dict(max_concurrent=1, max_wait_queue=-1), dict(max_concurrent=1, max_wait_time=0),
              dict(max_concurrent=1, max_wait_time=-0.5), dict(max_concurrent=0, max_wait_queue=-1), dict(max_concurrent=1, max_wait_queue=0, max_wait_time=None))


def test_mirrors_equal_the_recorded_defaults():
    ref = XR.get("defaults")
    k = hs.Sink("k")
    b, t = hs.Bulkhead("b", k, max_concurrent=3), hs.TimeoutWrapper("t", k, timeout=2.5)
    sb, st = b.stats, t.stats
    rb, rt = ref["bulkhead"], ref["timeout"]
    assert [b.max_concurrent, b.max_wait_queue, b.max_wait_time, b.active_count, b.queue_depth, b.available_permits, b._next_request_id,
            len(b._in_flight)] == rb["fields"]
    assert (b.target is k) == rb["target_is"] and [x.name for x in b.downstream_entities()] == rb["downstream"]
    assert type(sb).__name__ == rb["stats_type"] and [f.name for f in dataclasses.fields(sb)] == rb["stats_fields"]
    assert [getattr(sb, f) for f in rb["stats_fields"]] == rb["stats"]
    assert [t.timeout, t.in_flight_count, t._next_request_id] == rt["fields"]
    assert (t.target is k) == rt["target_is"] and [x.name for x in t.downstream_entities()] == rt["downstream"]
    assert type(st).__name__ == rt["stats_type"] and [f.name for f in dataclasses.fields(st)] == rt["stats_fields"]
    assert [getattr(st, f) for f in rt["stats_fields"]] == rt["stats"]
    for stats, r in ((sb, rb), (st, rt)):
        with pytest.raises(dataclasses.FrozenInstanceError) as e:
            stats.total_requests = 1
        assert type(e.value).__name__ == r["stats_frozen"]


def test_value_errors_have_the_reference_texts():
    ref = XR.get("defaults")
    k = hs.Sink("k")
    got = []
    for kw in _BH_ERRORS:
        try:
            hs.Bulkhead("x", k, **kw)
            got.append(None)
        except ValueError as e:
            got.append(str(e))
    assert got == ref["bulkhead"]["errors"] and sum(x is not None for x in got) == 6
    got = []
    for timeout in (0, -1.5, 0.0, 1e-9):
        try:
            hs.TimeoutWrapper("x", k, timeout=timeout)
            got.append(None)
        except ValueError as e:
            got.append(str(e))
    assert got == ref["timeout"]["errors"] and sum(x is not None for x in got) == 3


def test_the_lowering_accepts_every_spec():
    """Every recorded spec is one the product takes; a wrapper sends the Simulation to the single-heap loop whatever its shape."""
    for spec in XS.all_specs():
        XR.get("case", spec)                                   # (recorded: no case is left out)
        sim, pools = GF.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph) and g.arrays.has_wrappers and "Bulkhead or TimeoutWrapper" in sim._station_refusal, spec["name"]
        a = g.arrays
        for w, ws in zip(pools["wrapper"], spec["wrappers"]):
            i = g.node_of[id(w)]
            assert a.kind[i] == (N.NODE_BULKHEAD if ws["kind"] == "bulkhead" else N.NODE_TIMEOUT_WRAPPER)
            assert a.target[i] == g.node_of[id(w.target)]


def test_the_lowered_arrays_of_three_fixtures():
    sim, pools = GF.build(XS.FIXTURES["paused_server_leaks_permits"])      # src, srv0, sink0, bh0
    a = sim.lowered().arrays
    assert a.kind.tolist() == [N.NODE_SOURCE, N.NODE_SERVER, N.NODE_SINK, N.NODE_BULKHEAD] and a.target.tolist() == [3, 2, -1, 1]
    assert a.wrap_params[3].tolist() == [4.0, 3.0, 0.5, 0.0, 0.0] and not a.wrap_params[:3].any()
    assert len(sim._faults) == 2 and sim._general_faults(sim.lowered())[0][:3] == (1, 2 * 10 ** 9, True)
    sim, pools = GF.build(XS.FIXTURES["timeout_two_links"])                # src, srv0, link0, link1, sink0, tw0
    a = sim.lowered().arrays
    assert a.kind.tolist() == [N.NODE_SOURCE, N.NODE_SERVER, N.NODE_LINK, N.NODE_LINK, N.NODE_SINK, N.NODE_TIMEOUT_WRAPPER]
    assert a.target.tolist() == [5, 4, 3, 1, -1, 2] and a.wrap_params[5].tolist() == [0.0, 0.0, 0.0, 0.1, 0.0]
    assert a.rt_cnt.sum() == 0 and len(a.rt_targets) == 0                  # (the in-flight tables are the engine's: no router slots)
    sim, pools = GF.build(XS.FIXTURES["probes_on_the_four_metrics"])       # 2 src, 4 probes, srv0, link0, link1, sink0, bh0, tw1
    a = sim.lowered().arrays
    assert a.kind[2:6].tolist() == [N.NODE_PROBE] * 4 and a.probe_metric[2:6].tolist() == [8, 9, 10, 11] and a.target[2:6].tolist() == [10, 10, 10, 11]
    assert a.probe_interval_s[2:6].tolist() == [0.1, 0.1, 0.25, 0.1]
    assert a.wrap_params[10].tolist() == [2.0, 3.0, 0.5, 0.0, 0.0] and a.wrap_params[11, 3] == 0.1
    b = hs.Bulkhead("b", hs.Sink("k"), max_concurrent=1, max_wait_time=None)
    src = hs.Source.poisson(rate=5, target=b, name="src")
    a = hs.Simulation(sources=[src], entities=[b, b.target], end_time=hs.Instant.from_seconds(1)).lowered().arrays
    assert a.wrap_params[1].tolist() == [1.0, 0.0, -1.0, 0.0, 0.0]        # max_wait_time = None


def test_a_wrapper_only_reachable_from_a_source_sends_the_simulation_to_the_single_heap():
    k = hs.Sink("k")
    srv = hs.Server("s", service_time=hs.ExponentialLatency(0.05), downstream=k)
    t = hs.TimeoutWrapper("t", srv, timeout=0.5)
    sim = hs.Simulation(sources=[hs.Source.poisson(rate=5, target=t, name="src")], entities=[srv, k], end_time=hs.Instant.from_seconds(1))
    g = sim.lowered()
    assert isinstance(g, GeneralGraph) and g.arrays.kind.tolist().count(N.NODE_TIMEOUT_WRAPPER) == 1
    plain = hs.Simulation(sources=[hs.Source.poisson(rate=5, target=srv, name="src")], entities=[srv, k], end_time=hs.Instant.from_seconds(1))
    assert not isinstance(plain.lowered(), GeneralGraph)                   # (without a wrapper: the station engines, as before)


def _sim(first, *entities, **kw):
    return hs.Simulation(sources=[hs.Source.poisson(rate=5, target=first, name="src")], entities=list(entities),
                         end_time=hs.Instant.from_seconds(1), **kw)


def test_the_refusals_by_name():
    k = hs.Sink("k")
    srv = hs.Server("s", service_time=hs.ExponentialLatency(0.05), downstream=k)
    with pytest.raises(hs.UnsupportedTopology, match="TimeoutWrapper 't': on_timeout= is a host callable"):
        t = hs.TimeoutWrapper("t", srv, timeout=0.5, on_timeout=lambda ev: None)
        _sim(t, t, srv, k).lowered()
    # a wrapper as a LoadBalancer backend
    b = hs.Bulkhead("b", srv, max_concurrent=2)
    with pytest.raises(hs.UnsupportedTopology, match="backend 'b' of 'lb' is a Bulkhead: only Server backends are lowered"):
        lb = hs.LoadBalancer("lb", backends=[b])
        _sim(lb, lb, b, srv, k).lowered()
    # a wrapper whose target is a LoadBalancer, a Bulkhead or a TimeoutWrapper -- directly or through NetworkLinks
    lb = hs.LoadBalancer("lb", backends=[srv])
    for make in (lambda to: hs.Bulkhead("w", to, max_concurrent=2), lambda to: hs.TimeoutWrapper("w", to, timeout=0.5)):
        for inner in (lb, hs.Bulkhead("inner", srv, max_concurrent=1), hs.TimeoutWrapper("inner", srv, timeout=0.1)):
            w = make(inner)
            with pytest.raises(hs.UnsupportedTopology, match=f"'w': its target is the {type(inner).__name__} '{inner.name}' -- two completion hooks"):
                _sim(w, w, inner, srv, k).lowered()
            l2 = hs.NetworkLink("l2", latency=hs.ConstantLatency(0.01), egress=inner)
            l1 = hs.NetworkLink("l1", latency=hs.ConstantLatency(0.01), egress=l2)
            w = make(l1)
            with pytest.raises(hs.UnsupportedTopology, match=rf"'w': its target \(through its NetworkLinks\) is the {type(inner).__name__} '{inner.name}'"):
                _sim(w, w, l1, l2, inner, srv, k).lowered()
    # a wrapper whose target takes no Requests
    src2 = hs.Source.poisson(rate=1, target=k, name="other")
    probe, _d = hs.Probe.on(srv, "depth", interval=1.0)
    hc = hs.HealthChecker("hc", lb)
    for bad, text in ((src2, "a Source takes no Requests"), (probe, "Probe 'Probe_s_depth' is not lowered"), (hc, "the HealthChecker 'hc' takes no Requests"),
                      (hs.FaultSchedule(), "FaultSchedule")):
        w = hs.Bulkhead("w", bad, max_concurrent=1)
        with pytest.raises(hs.UnsupportedTopology, match=text):
            _sim(w, w, srv, k, lb).lowered()
    # ParallelSimulation partitions
    for w in (hs.Bulkhead("w", k, max_concurrent=1), hs.TimeoutWrapper("w", k, timeout=1.0)):
        part = hs.SimulationPartition("p0", entities=[w, k], sources=[hs.Source.poisson(rate=5, target=w, name="src")])
        with pytest.raises(hs.UnsupportedTopology, match=f"partition 'p0': the {type(w).__name__} 'w' on a ParallelSimulation partition is not lowered"):
            hs.ParallelSimulation([part], end_time=hs.Instant.from_seconds(1))
    # the table bound: at it and one above it
    at = hs.Bulkhead("w", k, max_concurrent=hs.Bulkhead.MAX_CONCURRENT)
    assert _sim(at, at, k).lowered().arrays.wrap_params[1, 0] == 65536 == N.BULKHEAD_MAX_CONCURRENT
    above = hs.Bulkhead("w", k, max_concurrent=hs.Bulkhead.MAX_CONCURRENT + 1)
    with pytest.raises(hs.UnsupportedTopology, match="Bulkhead 'w': max_concurrent = 65537 is beyond the 65536 request ids"):
        _sim(above, above, k).lowered()


def test_probe_metrics_belong_to_their_wrapper():
    k = hs.Sink("k")
    b, t = hs.Bulkhead("b", k, max_concurrent=1), hs.TimeoutWrapper("t", k, timeout=1.0)
    for target, metric in ((b, "active_count"), (b, "queue_depth"), (b, "available_permits"), (t, "in_flight_count")):
        hs.Probe.on(target, metric, interval=0.5)
    for target, metric in ((t, "active_count"), (t, "queue_depth"), (b, "in_flight_count"), (k, "available_permits")):
        with pytest.raises(NotImplementedError):
            hs.Probe.on(target, metric, interval=0.5)


def test_parts_keep_a_wrapper_with_its_target_and_leave_the_rest_without():
    spec = XS.groups_spec(4)
    spec["servers"].append(XS.srv(0.05, out=None))
    spec["sources"].append(XS.src(4, 9.0))                                  # a fifth component without any wrapper
    sim, pools = GF.build(spec)
    parts = split_parts(sim.lowered().arrays)
    assert len(parts) == 5
    with_w = [b for _ids, _pos, b in parts if b.has_wrappers]
    assert len(with_w) == 4 and all(((b.kind == N.NODE_BULKHEAD) | (b.kind == N.NODE_TIMEOUT_WRAPPER)).sum() == 1 for b in with_w)
    for b in with_w:
        i = int(np.nonzero((b.kind == N.NODE_BULKHEAD) | (b.kind == N.NODE_TIMEOUT_WRAPPER))[0][0])
        assert b.kind[b.target[i]] == N.NODE_LINK and b.wrap_params[i].any()


def test_the_new_symbols_are_in_the_header_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    for sym in ("hs_graph_set_wrapper", "hs_graph_get_wrapper"):
        assert re.search(rf"\bint {sym}\(hs_graph \*g", hdr) and sym in N.EXPORTED_SYMBOLS
    assert re.search(r"HS_NODE_BULKHEAD = 9\b", hdr) and re.search(r"HS_NODE_TIMEOUT_WRAPPER = 10\b", hdr)
    assert (N.NODE_BULKHEAD, N.NODE_TIMEOUT_WRAPPER) == (9, 10)
    assert re.search(r"#define HS_ABI_VERSION 16\b", hdr) and N.ABI_VERSION == 16 and N.EV_KINDS == 15
    assert re.search(rf"#define HS_BULKHEAD_MAX_CONCURRENT {N.BULKHEAD_MAX_CONCURRENT}\b", hdr)
    assert re.search(rf"#define HS_WRAPPER_COUNTERS {N.WRAPPER_COUNTERS}\b", hdr)
    for name, code in N.PROBE_WRAPPER_METRICS.items():
        macro = {"active_count": "BH_ACTIVE", "queue_depth": "BH_QUEUE_DEPTH", "available_permits": "BH_PERMITS", "in_flight_count": "TW_IN_FLIGHT"}[name]
        assert re.search(rf"HS_PROBE_{macro} = {code}\b", hdr)
    if os.path.exists(N.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
        for sym in ("hs_graph_set_wrapper", "hs_graph_get_wrapper"):
            assert re.search(rf" T {sym}$", out, re.M), sym
        lib = N.lib()
        assert lib.hs_abi_version() == 16
        for sym in ("hs_graph_set_wrapper", "hs_graph_get_wrapper"):
            getattr(lib, sym)
