"""Host side of Client and its retry policies (no GPU): the mirrors against the recorded live reference (tests/golden/live_client/),
what the lowering hands to the single-heap loop, send_request() and the named refusals."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import client_specs as CS
import graph_family as GF
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, client_delay_table, split_parts
from recorded import CLIENT as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the grids of tests/golden/make_golden_client.py, which needs the reference to be imported: repeated here)
FIXED_GRID = [(1, 0.0), (3, 0.25), (5, 0), (2, 1), (4, 1e-9)]
EXP_GRID = [(6, 0.1, 1.0, 2.0), (1, 0.1, 0.1, 2.0), (5, 0.05, 0.05, 3.0), (8, 0.001, 10.0, 10.0), (4, 0.3, 0.5, 1.0), (6, 0.1, 0.25, 2.0), (12, 1, 60, 1.5)]
CLIENT_ERRORS = (dict(timeout=-1), dict(timeout=-0.5), dict(timeout=0), dict(timeout=None), dict(timeout=0.0))
POLICY_ERRORS = (("fixed", (0, 0.1)), ("fixed", (1, -0.1)), ("fixed", (-1, -1)), ("fixed", (1, 0)),
                 ("exp", (0, 0.1, 1.0)), ("exp", (1, 0, 1.0)), ("exp", (1, 0.5, 0.1)), ("exp", (1, 0.1, 1.0, 0.5)), ("exp", (1, 0.1, 1.0, 2.0, -0.1)),
                 ("exp", (1, 0.1, 0.1)), ("jitter", (0, 0.1, 1.0)), ("jitter", (1, 0, 1.0)), ("jitter", (1, 0.5, 0.1)), ("jitter", (1, 0.1, 0.1)))


def test_mirrors_equal_the_recorded_defaults():
    ref = CR.get("defaults")
    k = hs.Sink("k")
    c = hs.Client("c", k)
    st = c.stats
    assert [c.timeout, type(c.retry_policy).__name__, c.in_flight_count, c.average_response_time, c._next_request_id,
            c.get_response_time_percentile(0.5), len(c._response_times)] == ref["fields"]
    assert (c.target is k) == ref["target_is"] and [x.name for x in c.downstream_entities()] == ref["downstream"]
    assert type(st).__name__ == ref["stats_type"] and [f.name for f in dataclasses.fields(st)] == ref["stats_fields"]
    assert [getattr(st, f) for f in ref["stats_fields"]] == ref["stats"]
    with pytest.raises(dataclasses.FrozenInstanceError) as e:
        st.timeouts = 1
    assert type(e.value).__name__ == ref["stats_frozen"]
    n, f, x, j = hs.NoRetry(), hs.FixedRetry(3, 0.25), hs.ExponentialBackoff(4, 0.1, 1.0), hs.DecorrelatedJitter(3, 0.1, 1.0)
    p = ref["policies"]
    assert [n.should_retry(1), n.should_retry(100), n.get_delay(1), n.get_delay(7)] == p["no_retry"]
    assert [f.max_attempts, f.delay, [f.should_retry(a) for a in range(1, 5)]] == p["fixed"]
    assert [x.max_attempts, x.initial_delay, x.max_delay, x.multiplier, x.jitter, [x.should_retry(a) for a in range(1, 6)]] == p["exp"]
    assert [j.max_attempts, j.base_delay, j.max_delay, [j.should_retry(a) for a in range(1, 5)], j._previous_delay] == p["jitter"]


def test_value_errors_have_the_reference_texts():
    ref = CR.get("defaults")
    k = hs.Sink("k")
    got = []
    for kw in CLIENT_ERRORS:
        try:
            hs.Client("x", k, **kw)
            got.append(None)
        except ValueError as e:
            got.append(str(e))
    assert got == ref["errors"] and sum(x is not None for x in got) == 2            # timeout = 0 is legal
    cls = {"fixed": hs.FixedRetry, "exp": hs.ExponentialBackoff, "jitter": hs.DecorrelatedJitter}
    got = []
    for kind, args in POLICY_ERRORS:
        try:
            cls[kind](*args)
            got.append(None)
        except ValueError as e:
            got.append(str(e))
    assert got == ref["policy_errors"] and sum(x is not None for x in got) == 11


def test_delay_tables_equal_the_recorded_ones():
    """get_delay(1 .. max_attempts) as floats, and the table of whole nanoseconds the lowering hands to the device against
    Duration.from_seconds of the recorded delays."""
    ref = CR.get("defaults")
    assert [[hs.FixedRetry(m, d).get_delay(a) for a in range(1, m + 1)] for m, d in FIXED_GRID] == ref["fixed_delays"]
    assert [[hs.ExponentialBackoff(*g).get_delay(a) for a in range(1, g[0] + 1)] for g in EXP_GRID] == ref["exp_delays"]
    assert ref["exp_delays"][0] == [0.1, 0.1, 0.2, 0.4, 0.8, 1.0] and ref["exp_delays"][5][-3:] == [0.25, 0.25, 0.25]      # the issue's; the cap
    for (m, d), want in zip(FIXED_GRID, ref["fixed_delays_ns"]):
        table = client_delay_table(hs.FixedRetry(m, d), "Client 'c'")
        assert table.dtype == np.int64 and table.tolist() == want[:m - 1]
        assert want == [hs.Duration.from_seconds(x).nanoseconds for x in [d] * m]
    for g, want in zip(EXP_GRID, ref["exp_delays_ns"]):
        assert client_delay_table(hs.ExponentialBackoff(*g), "Client 'c'").tolist() == want[:g[0] - 1]
    assert client_delay_table(hs.NoRetry(), "c").tolist() == [] and client_delay_table(hs.FixedRetry(1, 5.0), "c").tolist() == []


def test_jittered_policies_work_on_the_host():
    import random

    random.seed(5)
    j = hs.DecorrelatedJitter(5, 0.1, 2.0)
    d = [j.get_delay(a) for a in range(1, 5)]
    assert all(0.1 <= x <= 2.0 for x in d) and j._previous_delay == d[-1] and d[0] <= 0.3
    j.reset()
    assert j._previous_delay == 0.1
    x = hs.ExponentialBackoff(3, 0.1, 1.0, jitter=0.5)
    assert 0.1 <= x.get_delay(2) <= 0.6 and x.jitter == 0.5


def test_send_request_numbering_and_times():
    ref = CR.get("defaults")["send_request"]
    k = hs.Sink("k")
    c = hs.Client("c", k)
    ev1, ev2 = c.send_request(), c.send_request(payload={"a": 1}, event_type="get")
    assert isinstance(ev1, hs.Event)
    got = dict(ids=[ev1.context["metadata"]["request_id"], ev2.context["metadata"]["request_id"]], next_id=c._next_request_id,
               metadata_keys=sorted(ev1.context["metadata"]), attempt=ev1.context["metadata"]["attempt"],
               client_name=ev1.context["metadata"]["client_name"], payload=ev2.context["metadata"]["payload"]["a"],
               types=[ev1.event_type, ev2.event_type], time_ns=ev1.time.nanoseconds, target_is=ev1.target is c)
    assert got == ref and ev1.time == hs.Instant.Epoch                             # outside a Simulation
    c2 = hs.Client("c2", k, timeout=1.0)
    sim = hs.Simulation(start_time=hs.Instant.from_seconds(5), end_time=hs.Instant.from_seconds(9), entities=[c2, k])
    ev = c2.send_request()
    assert ev.time == hs.Instant.from_seconds(5) and ev.context["metadata"]["request_id"] == 1       # the Simulation's start before run()
    ev.time = hs.Instant.from_seconds(6)
    sim.schedule(ev)
    g = sim.lowered()
    _end, _start, sched, cancelled = sim._general_prepare(g, False)
    assert sched == [(g.node_of[id(c2)], 6 * 10 ** 9, 1)] and cancelled == []     # created_at (5 s) need not equal the time
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(7), event_type="Request", target=c2))
    assert sim._general_prepare(g, False)[2][1] == (g.node_of[id(c2)], 7 * 10 ** 9, 0)                # a plain Event: no request_id


def test_the_lowering_accepts_every_spec():
    """Every recorded spec is one the product takes; a Client sends the Simulation to the single-heap loop whatever its shape."""
    for spec in CS.all_specs():
        CR.get("case", spec)                                   # (recorded: no case is left out)
        sim, pools = GF.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph) and g.arrays.has_clients and "do not lower a Client" in sim._station_refusal, spec["name"]
        a = g.arrays
        for c, cs in zip(pools["client"], spec["clients"]):
            i = g.node_of[id(c)]
            assert a.kind[i] == N.NODE_CLIENT and a.target[i] == g.node_of[id(c.target)]
            assert a.cl_params[i, 0] == (-1.0 if cs["timeout"] is None else cs["timeout"])
            assert a.cl_delay_off[i + 1] - a.cl_delay_off[i] == (0 if cs["policy"] is None else cs["policy"][1] - 1)
        sim._general_prepare(g, bool(spec.get("auto")))


def test_the_lowered_arrays_of_two_fixtures():
    sim, pools = GF.build(CS.FIXTURES["exponential_backoff_at_its_cap"])  # srv0, sink0, cl0
    a = sim.lowered().arrays
    assert a.kind.tolist() == [N.NODE_SERVER, N.NODE_SINK, N.NODE_CLIENT] and a.target.tolist() == [1, -1, 0]
    assert a.cl_params[2].tolist() == [0.05, 0.0] and not a.cl_params[:2].any()
    assert a.cl_delay_off.tolist() == [0, 0, 0, 5] and a.cl_delays_ns.tolist() == [100_000_000, 100_000_000, 200_000_000, 250_000_000, 250_000_000]
    sched = sim._general_prepare(sim.lowered(), False)[2]
    assert sched == [(2, 600_000_000, 1), (2, 700_000_000, 2), (2, 1_400_000_000, 3)]
    sim, pools = GF.build(CS.FIXTURES["probe_on_in_flight_count"])        # 2 src, 2 probes, srv0, link0, link1, sink0, cl0, cl1
    a = sim.lowered().arrays
    assert a.kind[2:4].tolist() == [N.NODE_PROBE] * 2 and a.probe_metric[2:4].tolist() == [12, 12] and a.target[2:4].tolist() == [8, 9]
    assert a.cl_params[8:].tolist() == [[0.3, 0.0], [-1.0, 0.0]] and a.cl_delays_ns.tolist() == [100_000_000]
    assert a.rt_cnt.sum() == 0                                             # (the in-flight tables are the engine's: no router slots)


def test_a_client_only_reachable_from_a_source_sends_the_simulation_to_the_single_heap():
    k = hs.Sink("k")
    srv = hs.Server("s", service_time=hs.ExponentialLatency(0.05), downstream=k)
    c = hs.Client("c", srv, timeout=0.5, retry_policy=hs.FixedRetry(2, 0.1))
    sim = hs.Simulation(sources=[hs.Source.poisson(rate=5, target=c, name="src")], entities=[srv, k], end_time=hs.Instant.from_seconds(1))
    g = sim.lowered()
    assert isinstance(g, GeneralGraph) and g.arrays.kind.tolist().count(N.NODE_CLIENT) == 1


def _sim(first, *entities, **kw):
    return hs.Simulation(sources=[hs.Source.poisson(rate=5, target=first, name="src")], entities=list(entities),
                         end_time=hs.Instant.from_seconds(1), **kw)


def test_the_refusals_by_name():
    k = hs.Sink("k")
    srv = hs.Server("s", service_time=hs.ExponentialLatency(0.05), downstream=k)
    # host callables
    for kw in (dict(on_success=lambda a, b: None), dict(on_failure=lambda a, b: None)):
        c = hs.Client("c", srv, timeout=0.5, **kw)
        with pytest.raises(hs.UnsupportedTopology, match="Client 'c': on_success= / on_failure= are host callables"):
            _sim(c, c, srv, k).lowered()
        c = hs.Client("c", srv, timeout=0.5)
        sim = _sim(srv, c, srv, k)
        sim.schedule(c.send_request(**kw))
        with pytest.raises(hs.UnsupportedTopology, match="on_success= / on_failure= are host callables"):
            sim._general_prepare(sim.lowered(), False)
    # the policies that draw from the process-wide generator, and foreign ones
    class Mine:
        def should_retry(self, attempt, error=None):
            return False

        def get_delay(self, attempt):
            return 0.0

    for policy, text in ((hs.ExponentialBackoff(3, 0.1, 1.0, jitter=0.1), r"ExponentialBackoff\(jitter=0.1\) draws from the process-wide random generator"),
                         (hs.DecorrelatedJitter(3, 0.1, 1.0), "DecorrelatedJitter draws from the process-wide random generator"),
                         (Mine(), "retry policy Mine is not lowered"),
                         (hs.FixedRetry(hs.Client.MAX_ATTEMPTS + 1, 0.1), "max_attempts = 65537 is beyond the 65536 attempts"),
                         (hs.FixedRetry(3, float("inf")), r"the delay of attempt 1 cannot be evaluated as a Duration \(OverflowError"),
                         (hs.ExponentialBackoff(4, 1.0, float("inf"), 1e300), r"the delay of attempt 3 cannot be evaluated as a Duration \(OverflowError")):
        c = hs.Client("c", srv, timeout=0.5, retry_policy=policy)
        with pytest.raises(hs.UnsupportedTopology, match="Client 'c': " + text):
            _sim(c, c, srv, k).lowered()
    at = hs.Client("c", srv, timeout=0.5, retry_policy=hs.FixedRetry(hs.Client.MAX_ATTEMPTS, 0.1))      # at the bound: taken
    assert len(_sim(at, at, srv, k).lowered().arrays.cl_delays_ns) == 65535 == N.CLIENT_MAX_ATTEMPTS - 1
    # a Client as a LoadBalancer backend
    c = hs.Client("c", srv, timeout=0.5)
    with pytest.raises(hs.UnsupportedTopology, match="backend 'c' of 'lb' is a Client: only Server backends are lowered"):
        lb = hs.LoadBalancer("lb", backends=[c])
        _sim(lb, lb, c, srv, k).lowered()
    # a Client whose target is a LoadBalancer, a Bulkhead, a TimeoutWrapper or a Client -- directly or through NetworkLinks
    lb = hs.LoadBalancer("lb", backends=[srv])
    for inner in (lb, hs.Bulkhead("inner", srv, max_concurrent=1), hs.TimeoutWrapper("inner", srv, timeout=0.1), hs.Client("inner", srv)):
        w = hs.Client("w", inner, timeout=0.5)
        with pytest.raises(hs.UnsupportedTopology, match=f"Client 'w': its target is the {type(inner).__name__} '{inner.name}' -- two completion hooks"):
            _sim(w, w, inner, srv, k).lowered()
        l2 = hs.NetworkLink("l2", latency=hs.ConstantLatency(0.01), egress=inner)
        l1 = hs.NetworkLink("l1", latency=hs.ConstantLatency(0.01), egress=l2)
        w = hs.Client("w", l1, timeout=0.5)
        with pytest.raises(hs.UnsupportedTopology, match=rf"Client 'w': its target \(through its NetworkLinks\) is the {type(inner).__name__} '{inner.name}'"):
            _sim(w, w, l1, l2, inner, srv, k).lowered()
    # a Bulkhead or a TimeoutWrapper whose target is a Client
    inner = hs.Client("inner", srv, timeout=0.5)
    for w in (hs.Bulkhead("w", inner, max_concurrent=2), hs.TimeoutWrapper("w", inner, timeout=0.5)):
        with pytest.raises(hs.UnsupportedTopology, match=f"{type(w).__name__} 'w': its target is the Client 'inner' -- two completion hooks"):
            _sim(w, w, inner, srv, k).lowered()
    l1 = hs.NetworkLink("l1", latency=hs.ConstantLatency(0.01), egress=inner)
    w = hs.TimeoutWrapper("w", l1, timeout=0.5)
    with pytest.raises(hs.UnsupportedTopology, match=r"TimeoutWrapper 'w': its target \(through its NetworkLinks\) is the Client 'inner'"):
        _sim(w, w, l1, inner, srv, k).lowered()
    # a target that takes no Requests
    src2 = hs.Source.poisson(rate=1, target=k, name="other")
    probe, _d = hs.Probe.on(srv, "depth", interval=1.0)
    hc = hs.HealthChecker("hc", lb)
    for bad, text in ((src2, "a Source takes no Requests"), (probe, "Probe 'Probe_s_depth' is not lowered"), (hc, "the HealthChecker 'hc' takes no Requests"),
                      (hs.FaultSchedule(), "FaultSchedule")):
        w = hs.Client("w", bad, timeout=1.0)
        with pytest.raises(hs.UnsupportedTopology, match=text):
            _sim(w, w, srv, k, lb).lowered()
    # ParallelSimulation partitions
    w = hs.Client("w", k, timeout=1.0)
    part = hs.SimulationPartition("p0", entities=[w, k], sources=[hs.Source.poisson(rate=5, target=w, name="src")])
    with pytest.raises(hs.UnsupportedTopology, match="partition 'p0': the Client 'w' on a ParallelSimulation partition is not lowered"):
        hs.ParallelSimulation([part], end_time=hs.Instant.from_seconds(1))
    # PooledClient / ConnectionPool stay unmirrored
    assert not hasattr(hs, "PooledClient") and not hasattr(hs, "ConnectionPool")


def test_scheduled_events_a_client_does_not_take():
    k = hs.Sink("k")
    c = hs.Client("c", k, timeout=0.5)

    def prepare(ev):
        sim = hs.Simulation(entities=[c, k], end_time=hs.Instant.from_seconds(1))
        sim.schedule(ev)
        return sim._general_prepare(sim.lowered(), False)[2]

    def event(**metadata):
        return hs.Event(time=hs.Instant.from_seconds(0.5), event_type="Request", target=c, context={"metadata": metadata})

    node = 0
    assert prepare(event()) == [(node, 500_000_000, 0)] and prepare(event(request_id=None, attempt=1)) == [(node, 500_000_000, 0)]
    assert prepare(event(request_id=(1 << 30) - 1)) == [(node, 500_000_000, (1 << 30) - 1)]
    for attempt in (2, 0, None, True):
        with pytest.raises(hs.UnsupportedTopology, match=rf"attempt = {attempt!r} is not lowered"):
            prepare(event(request_id=3, attempt=attempt))
    for rid in (0, -1, 1 << 30, 1.0, "a", True):
        with pytest.raises(hs.UnsupportedTopology, match=rf"request_id = {rid!r} is not lowered \(None or a positive int below 2\^30\)"):
            prepare(event(request_id=rid))
    for et in ("_client_timeout", "_client_response"):
        with pytest.raises(hs.UnsupportedTopology, match=f"a Client's own '{et}' Event is not lowered"):
            prepare(hs.Event(time=hs.Instant.from_seconds(0.5), event_type=et, target=c))


def test_probe_metric_belongs_to_a_client():
    k = hs.Sink("k")
    c = hs.Client("c", k)
    hs.Probe.on(c, "in_flight_count", interval=0.5)
    for metric in ("active_count", "queue_depth", "available_permits"):
        with pytest.raises(NotImplementedError):
            hs.Probe.on(c, metric, interval=0.5)
    with pytest.raises(NotImplementedError):
        hs.Probe.on(k, "in_flight_count", interval=0.5)


def test_parts_keep_a_client_with_its_target_and_leave_the_rest_without():
    spec = CS.groups_spec(4)
    spec["servers"].append(CS.srv(0.05, out=None))
    spec["sources"].append(CS.src(4, 9.0))                                  # a fifth component without any Client
    sim, pools = GF.build(spec)
    a = sim.lowered().arrays
    parts = split_parts(a)
    assert len(parts) == 5
    with_c = [b for _ids, _pos, b in parts if b.has_clients]
    assert len(with_c) == 4 and all((b.kind == N.NODE_CLIENT).sum() == 1 for b in with_c)
    for g, b in enumerate(with_c):
        i = int(np.nonzero(b.kind == N.NODE_CLIENT)[0][0])
        assert b.kind[b.target[i]] == N.NODE_LINK and b.cl_params[i, 0] == spec["clients"][g]["timeout"]
        want = client_delay_table(pools["client"][g].retry_policy, "c")
        assert b.cl_delays_ns[b.cl_delay_off[i]:b.cl_delay_off[i + 1]].tolist() == want.tolist() and len(b.cl_delays_ns) == len(want)


def test_what_the_issue_says_holds_in_the_recordings():
    get = lambda name: CR.get("case", CS.FIXTURES[name])  # noqa: E731
    r = get("keyless_ten_plain_events")
    assert r["cl_stats"][0].tolist() == [10, 3, 5, 0, 5, 0, 0] and len(r["cl_keys"]) == 0
    r = get("link_double_response_twenty_requests")
    assert r["cl_stats"][0, :5].tolist() == [40, 0, 40, 20, 20] and r["by_kind"][28:].tolist() == [40, 80, 40] and r["received"][0] == 40
    assert np.array_equal(r["sink_latency_s"], np.full(40, 0.04))
    r = get("timeout_zero_sink")
    assert r["cl_stats"][0, :5].tolist() == [15, 0, 15, 10, 5] and r["received"][0] == 15
    r = get("client_crash_without_restart")
    assert r["cl_stats"][0, 5] == len(r["cl_keys"]) > 0 and r["crashed"].sum() == 1
    r = get("late_response_of_attempt_one")
    trace = r["trace"]
    sends = trace[trace[:, 1] == 28][:, 0].tolist()
    late = [t for t in trace[trace[:, 1] == 29][:, 0].tolist() if t == 300_000_000]
    assert sends[:2] == [0, 250_000_000] and len(late) == 2 and r["cl_stats"][0, 1] == 0      # attempt 1's responses at 0.3 s, attempt 2 in flight until 0.45 s
    assert len(CS.FIXTURES) >= 40 and len(CS.TRACED) == 6 and CS.N_RANDOM >= 120
    assert max(os.path.getsize(os.path.join(CR.rec_dir, f)) for f in os.listdir(CR.rec_dir)) <= 531_061       # the largest live_resilience part


def test_the_new_symbols_are_in_the_header_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    syms = ("hs_graph_set_client", "hs_graph_schedule_client", "hs_graph_get_client")
    for sym in syms:
        assert re.search(rf"\bint {sym}\(hs_graph \*g", hdr) and sym in N.EXPORTED_SYMBOLS
    assert re.search(r"HS_NODE_CLIENT = 11\b", hdr) and N.NODE_CLIENT == 11
    assert re.search(r"#define HS_ABI_VERSION 16\b", hdr) and N.ABI_VERSION == 16 and N.EV_KINDS == 15
    assert re.search(rf"#define HS_CLIENT_MAX_ATTEMPTS {N.CLIENT_MAX_ATTEMPTS}\b", hdr) and hs.Client.MAX_ATTEMPTS == N.CLIENT_MAX_ATTEMPTS
    assert re.search(rf"#define HS_CLIENT_COUNTERS {N.CLIENT_COUNTERS}\b", hdr)
    assert re.search(rf"HS_PROBE_CL_IN_FLIGHT = {N.PROBE_CLIENT_METRICS['in_flight_count']}\b", hdr)
    assert hs.Client.MAX_REQUEST_ID == N.CLIENT_MAX_REQUEST_ID == 1 << 30
    if os.path.exists(N.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
        for sym in syms:
            assert re.search(rf" T {sym}$", out, re.M), sym
        lib = N.lib()
        assert lib.hs_abi_version() == 16
        for sym in syms:
            getattr(lib, sym)
