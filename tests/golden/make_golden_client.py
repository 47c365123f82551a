#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for Client and its retry policies (components/client/client.py, retry.py) -- the
yardstick of tests/test_client_host.py and tests/test_gpu_client.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_client.py          # writes tests/golden/live_client/part_*.npz

Recorded (tests/client_reference.py reads them back):
  * constructor defaults, properties, stats objects and the ValueError texts of Client and the four policies, and
    get_delay(1 .. max_attempts) of FixedRetry and ExponentialBackoff over a parameter grid that includes the max_delay cap;
  * every spec of client_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs of
    make_golden.py choosing the random numbers -- everything make_golden_resilience.run_case records (this run_case is that one with the
    Clients wired in), plus per Client its statistics, its keys in flight and its response times, and the Clients' Events processed
    (kinds 28 / 29 / 30 = a request at a Client, its `_client_response`, its `_client_timeout`, in by_kind and in the trace); the
    fixtures of client_specs.TRACED with their full trace.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed): no case is left out.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))        # (the product: the recorder asserts that it takes every spec)

import client_specs as CS  # noqa: E402
import fault_specs as FS  # noqa: E402
import health_specs as HS  # noqa: E402
import rate_limiter_specs as RS  # noqa: E402
import resilience_specs as XS  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the reference's import path; the stream plugs and the trace classifier)
import make_golden_rate_limiter as MGR  # noqa: E402
import make_golden_faults as MGF  # noqa: E402
import make_golden_health as MGH  # noqa: E402
import make_golden_resilience as MGX  # noqa: E402
import happysimulator.faults as ref_faults  # noqa: E402
import happysimulator.components.client as ref_client  # noqa: E402
from happysimulator import Server, Simulation, Sink  # noqa: E402
from happysimulator.components.client import Client, DecorrelatedJitter, ExponentialBackoff, FixedRetry, NoRetry  # noqa: E402
from happysimulator.components.client.client import ClientStats  # noqa: E402
from happysimulator.components.load_balancer import HealthChecker  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from happysimulator.components.resilience import Bulkhead, TimeoutWrapper  # noqa: E402
from happysimulator.core.event import Event  # noqa: E402
from happysimulator.core.temporal import Duration  # noqa: E402

EV_CL_REQ = MGX.EV_TW_TIMEOUT + 1
EV_CL_RESP, EV_CL_TIMEOUT = EV_CL_REQ + 1, EV_CL_REQ + 2
assert EV_CL_REQ == 28
FIXED_GRID = [(1, 0.0), (3, 0.25), (5, 0), (2, 1), (4, 1e-9)]
EXP_GRID = [(6, 0.1, 1.0, 2.0), (1, 0.1, 0.1, 2.0), (5, 0.05, 0.05, 3.0), (8, 0.001, 10.0, 10.0), (4, 0.3, 0.5, 1.0), (6, 0.1, 0.25, 2.0), (12, 1, 60, 1.5)]
CLIENT_ERRORS = (dict(timeout=-1), dict(timeout=-0.5), dict(timeout=0), dict(timeout=None), dict(timeout=0.0))
POLICY_ERRORS = (("fixed", (0, 0.1)), ("fixed", (1, -0.1)), ("fixed", (-1, -1)), ("fixed", (1, 0)),
                 ("exp", (0, 0.1, 1.0)), ("exp", (1, 0, 1.0)), ("exp", (1, 0.5, 0.1)), ("exp", (1, 0.1, 1.0, 0.5)), ("exp", (1, 0.1, 1.0, 2.0, -0.1)),
                 ("exp", (1, 0.1, 0.1)), ("jitter", (0, 0.1, 1.0)), ("jitter", (1, 0, 1.0)), ("jitter", (1, 0.5, 0.1)), ("jitter", (1, 0.1, 0.1)))


def policy_error(ns, kind, args):
    cls = {"fixed": ns.FixedRetry, "exp": ns.ExponentialBackoff, "jitter": ns.DecorrelatedJitter}[kind]
    try:
        cls(*args)
        return None
    except ValueError as e:
        return str(e)


def defaults():
    """Constructor state, properties, stats objects, error texts and delay tables."""
    k = Sink("k")
    c = Client("c", k)
    st = c.stats
    out = dict(fields=[c.timeout, type(c.retry_policy).__name__, c.in_flight_count, c.average_response_time, c._next_request_id,
                       c.get_response_time_percentile(0.5), len(c._response_times)],
               target_is=c.target is k, downstream=[x.name for x in c.downstream_entities()], stats_type=type(st).__name__,
               stats_fields=[f for f in ClientStats.__dataclass_fields__], stats=[getattr(st, f) for f in ClientStats.__dataclass_fields__])
    try:
        st.timeouts = 1
        out["stats_frozen"] = False
    except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
        out["stats_frozen"] = type(e).__name__
    errors = []
    for kw in CLIENT_ERRORS:
        try:
            Client("x", k, **kw)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["errors"] = errors
    out["policy_errors"] = [policy_error(ref_client, kind, args) for kind, args in POLICY_ERRORS]
    # send_request: the ids, the metadata and the time without a clock
    ev1, ev2 = c.send_request(), c.send_request(payload={"a": 1}, event_type="get")
    out["send_request"] = dict(ids=[ev1.context["metadata"]["request_id"], ev2.context["metadata"]["request_id"]], next_id=c._next_request_id,
                               metadata_keys=sorted(ev1.context["metadata"]), attempt=ev1.context["metadata"]["attempt"],
                               client_name=ev1.context["metadata"]["client_name"], payload=ev2.context["metadata"]["payload"]["a"],
                               types=[ev1.event_type, ev2.event_type], time_ns=ev1.time.nanoseconds, target_is=ev1.target is c)
    n, f, e, j = NoRetry(), FixedRetry(3, 0.25), ExponentialBackoff(4, 0.1, 1.0), DecorrelatedJitter(3, 0.1, 1.0)
    out["policies"] = dict(no_retry=[n.should_retry(1), n.should_retry(100), n.get_delay(1), n.get_delay(7)],
                           fixed=[f.max_attempts, f.delay, [f.should_retry(a) for a in range(1, 5)]],
                           exp=[e.max_attempts, e.initial_delay, e.max_delay, e.multiplier, e.jitter, [e.should_retry(a) for a in range(1, 6)]],
                           jitter=[j.max_attempts, j.base_delay, j.max_delay, [j.should_retry(a) for a in range(1, 5)], j._previous_delay])
    out["fixed_delays"] = [[FixedRetry(m, d).get_delay(a) for a in range(1, m + 1)] for m, d in FIXED_GRID]
    out["exp_delays"] = [[ExponentialBackoff(*g).get_delay(a) for a in range(1, g[0] + 1)] for g in EXP_GRID]
    # Duration.from_seconds of every delay: what the timeout handler adds to `now`
    out["fixed_delays_ns"] = [[Duration.from_seconds(x).nanoseconds for x in row] for row in out["fixed_delays"]]
    out["exp_delays_ns"] = [[Duration.from_seconds(x).nanoseconds for x in row] for row in out["exp_delays"]]
    return out


def run_case(spec, want_trace=False):
    """The reference's run of one spec.  Trace nodes: Sources, Probes, then the entities (servers + lbs + routers + links + limiters
    + sinks + wrappers + clients + checkers); trace kinds: make_golden_resilience's (0 .. 27), then 28 .. 30 = the Clients' three."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    F = MGX._Reference(spec)                                  # (its probe() takes `in_flight_count` by name, of a Client too)
    pools, sources, probes, entities = CS.wire(spec, F, ref_client, Bulkhead, TimeoutWrapper, HealthChecker)
    FS.apply_names(spec, pools)
    servers, sinks, links, routers, lbs, lims = (pools[k] for k in ("server", "sink", "link", "router", "lb", "limiter"))
    fs, handles = FS.make_schedule(ref_faults, spec, pools)
    sim = Simulation(start_time=MG._start(spec), sources=sources, entities=entities, fault_schedule=fs,
                     **({} if spec.get("auto") else {"end_time": MG._at(spec, spec["end_s"])}), **({"probes": probes} if probes else {}))
    FS.cancel_after(spec, handles)
    node_of = {}
    for i, x in enumerate(sources + probes):
        node_of[id(x)] = i
    first = len(sources) + len(probes)
    lim_index = {}
    for i, x in enumerate(entities):
        node_of[id(x)] = first + i
        if isinstance(x, Server):
            for part in (x._queue, x._driver, x._worker):
                node_of[id(part)] = first + i
        if isinstance(x, RateLimitedEntity):
            lim_index[id(x)] = len(lim_index)
    by_name = {x.name: node_of[id(x)] for x in entities + sources + probes}
    cb_probe = {id(p._event_provider.data_sink): len(sources) + j for j, p in enumerate(probes)}
    by_kind = np.zeros(EV_CL_TIMEOUT + 1, np.int64)
    lim_events = np.zeros((len(lims), 2), np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop
    state = dict(cur=sim._start_time, cancelled=0, skipped=0)

    def pop():
        e = orig_pop()
        if by_kind.sum() >= MGR.MAX_EVENTS:
            raise MGR.Livelock(spec["name"])
        if e.cancelled:
            state["cancelled"] += 1
            return e
        if e.time < state["cur"]:
            state["skipped"] += 1
            return e
        state["cur"] = e.time
        et = e.event_type
        if et.startswith(MGF._ON) or et.startswith(MGF._OFF):
            k, nd = (MGF.EV_FAULT_ON if et.startswith(MGF._ON) else MGF.EV_FAULT_OFF), by_name[et.split(":", 1)[1]]
        elif isinstance(e.target, Client):
            k, nd = {"_client_response": EV_CL_RESP, "_client_timeout": EV_CL_TIMEOUT}.get(et, EV_CL_REQ), node_of[id(e.target)]
        elif isinstance(e.target, Bulkhead):
            k, nd = {"_bh_response": MGX.EV_BH_RESP, "_bh_timeout": MGX.EV_BH_TIMEOUT}.get(et, MGX.EV_BH_REQ), node_of[id(e.target)]
        elif isinstance(e.target, TimeoutWrapper):
            k, nd = {"_tw_response": MGX.EV_TW_RESP, "_tw_timeout": MGX.EV_TW_TIMEOUT}.get(et, MGX.EV_TW_REQ), node_of[id(e.target)]
        elif isinstance(e.target, HealthChecker):
            k, nd = MGH._HC_KIND[et], node_of[id(e.target)]
        elif isinstance(e.target, RateLimitedEntity):
            poll = et == f"rate_limit_poll::{e.target.name}"
            k, nd = (MGR.EV_LIM_POLL if poll else MGR.EV_LIM_REQUEST), node_of[id(e.target)]
            if not getattr(e.target, "_crashed", False):
                lim_events[lim_index[id(e.target)], int(poll)] += 1
        else:
            k, nd = MG.classify(e, node_of)
        if k == MG.EV["probe"]:
            fn = e.target._fn if hasattr(e.target, "_fn") else e.target.fn
            cells = {id(cell.cell_contents) for cell in (fn.__closure__ or ())}
            nd = next(c for key, c in cb_probe.items() if key in cells)
        by_kind[k] += 1
        if want_trace:
            trace.append((e.time.nanoseconds, k, nd, e._sort_index))
        return e

    heap.pop = pop
    CS.schedule_all(spec, pools, sim, Event, lambda t_s: MG._at(spec, t_s))
    HS.start_checkers(spec, pools, sim, [[] for _ in pools["checker"]])
    summary = MG.run_sim_windows(sim, spec)
    out = dict(total_events=int(summary.total_events_processed), final_ns=int(sim._current_time.nanoseconds), by_kind=by_kind)
    assert int(by_kind.sum()) == out["total_events"], (spec["name"], int(by_kind.sum()), out["total_events"])
    assert state["cancelled"] == int(sim._events_cancelled)
    out["pending_events"] = int(heap.size())
    out["time_travel"] = int(state["skipped"])
    out["generated"] = np.array([s.generated_count for s in sources], np.int64)
    out["accepted"] = np.array([s.stats_accepted for s in servers], np.int64)
    out["dropped"] = np.array([s.stats_dropped for s in servers], np.int64)
    out["completed"] = np.array([s._requests_completed for s in servers], np.int64)
    out["rejected"] = np.array([s._requests_rejected for s in servers], np.int64)
    out["depth"] = np.array([s.depth for s in servers], np.int64)
    out["active"] = np.array([s.active_requests for s in servers], np.int64)
    out["total_service_s"] = np.array([s._total_service_time for s in servers], np.float64)
    out["received"] = np.array([k.events_received for k in sinks], np.int64)
    out["routed"] = np.array([r.stats_routed for r in routers], np.int64)
    out["packets_sent"] = np.array([l.packets_sent for l in links], np.int64)
    out["packets_dropped"] = np.array([l.packets_dropped for l in links], np.int64)
    out["lb_stats"] = np.array([[lb.stats.requests_received, lb.stats.requests_forwarded, lb.stats.requests_failed,
                                 lb.stats.no_backend_available, len(lb._in_flight)] for lb in lbs], np.int64).reshape(-1, 5)
    tot, toff, index = [], [0], []
    for j, lb in enumerate(lbs):
        tot.extend(lb.get_backend_info(servers[b]).total_requests for b in spec["lbs"][j]["backends"])
        toff.append(len(tot))
        st = lb.strategy
        index.append(st._fallback._index if hasattr(st, "_fallback") else getattr(st, "_index", -1))
    out["lb_backend_total_requests"] = np.asarray(tot, np.int64)
    out["lb_backend_off"] = np.asarray(toff, np.int64)
    out["lb_rr_index"] = np.asarray(index, np.int64)
    sink_t, sink_lat, off = [], [], [0]
    for k in sinks:
        sink_t.extend(t.nanoseconds for t in k.completion_times)
        sink_lat.extend(k.latencies_s)
        off.append(len(sink_t))
    out["sink_t_ns"] = np.asarray(sink_t, np.int64)
    out["sink_latency_s"] = np.asarray(sink_lat, np.float64)
    out["sink_off"] = np.asarray(off, np.int64)
    pt, pv, poff = [], [], [0]
    for d in F.probe_data:
        pt.extend(t for t, _ in d._ns)
        pv.extend(int(v) for _, v in d._ns)
        poff.append(len(pt))
    out["probe_t_ns"], out["probe_v"], out["probe_off"] = np.asarray(pt, np.int64), np.asarray(pv, np.int64), np.asarray(poff, np.int64)
    out.update(RS.limiter_results(lims))
    out["lim_events"] = lim_events
    out.update(FS.fault_results(fs, CS.fault_targets(pools)))
    out.update(HS.health_results(spec, pools))
    out.update(XS.wrapper_results(pools))
    out.update(CS.client_results(pools))
    out["fault_events"] = int(by_kind[MGF.EV_FAULT_ON] + by_kind[MGF.EV_FAULT_OFF])
    out["events_cancelled"] = int(summary.events_cancelled)
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out


def main():
    import client_reference as CR

    cases = {CR.key("defaults"): defaults()}
    for spec in CS.all_specs():
        sim, _pools = CS.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_clients, spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[CR.key("case", spec)] = run_case(spec, want_trace=spec["name"] in CS.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        print(spec["name"], res["total_events"], res["by_kind"][EV_CL_REQ:].tolist(), res["cl_stats"].tolist(), res["crashed"].sum(), flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[CR.key("case", CS.FIXTURES[name])]  # noqa: E731
    d = cases[CR.key("defaults")]
    assert d["exp_delays"][0] == [0.1, 0.1, 0.2, 0.4, 0.8, 1.0], d["exp_delays"][0]
    assert d["errors"] == ["timeout must be >= 0, got -1", "timeout must be >= 0, got -0.5", None, None, None]      # timeout = 0 is legal
    r = get("keyless_ten_plain_events")                    # 10 plain Events at 0.0 .. 0.9 s, timeout 0.5, the Server paused over [0.25, 0.55)
    assert r["cl_stats"][0].tolist() == [10, 3, 5, 0, 5, 0, 0], r["cl_stats"]
    r = get("link_double_response_twenty_requests")        # Client(0.02, FixedRetry(2, 0.05)) -> NetworkLink(0.03) -> Server(0.01) -> Sink
    assert r["cl_stats"][0, :5].tolist() == [40, 0, 40, 20, 20] and r["by_kind"][EV_CL_RESP] == 80 and r["received"][0] == 40, (r["cl_stats"], r["by_kind"])
    assert np.array_equal(r["sink_latency_s"], np.full(40, 0.04)), r["sink_latency_s"]       # created_at is the send time of the attempt
    r = get("timeout_zero_sink")                           # the timeout was constructed before the response and pops first
    assert r["cl_stats"][0, :5].tolist() == [15, 0, 15, 10, 5] and r["received"][0] == 15, r["cl_stats"]
    r = get("retry_lands_after_the_restart")
    assert r["cl_stats"][0, :5].tolist() == [3, 1, 2, 2, 0], r["cl_stats"]
    r = get("late_response_of_attempt_one")
    assert r["cl_stats"][0, :5].tolist() == [6, 0, 6, 3, 3] and r["by_kind"][EV_CL_RESP] == 12, (r["cl_stats"], r["by_kind"])    # every response (two per attempt: link and Sink) is late: a no-op
    r = get("client_crash_without_restart")
    assert r["cl_stats"][0, 5] > 0                         # entries stay in flight for ever
    r = get("source_plain_and_send_request_mixed")
    assert r["cl_stats"][0, 6] == 4
    assert len(CS.FIXTURES) >= 40 and len(CS.TRACED) == 6 and CS.N_RANDOM >= 120
    CR.write(cases)


if __name__ == "__main__":
    main()
