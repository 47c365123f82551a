#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for Bulkhead and TimeoutWrapper (components/resilience/bulkhead.py, timeout.py)
-- the yardstick of tests/test_resilience_host.py and tests/test_gpu_resilience.py.  Run by hand where the reference is installed
(refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_resilience.py          # writes tests/golden/live_resilience/part_*.npz

Recorded (tests/resilience_reference.py reads them back):
  * constructor defaults, properties, stats objects and the ValueError texts of both classes;
  * every spec of resilience_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs
    of make_golden.py choosing the random numbers -- everything make_golden_faults.run_case records (this run_case is that one with the
    wrappers wired in), plus what make_golden_health.run_case records about checkers, plus per wrapper its statistics, its ids in flight
    and the ids of its wait queue, and the wrappers' Events processed (kinds 22 / 23 / 24 = a Request at a Bulkhead, its `_bh_response`,
    its `_bh_timeout`; 25 / 26 / 27 = the same of a TimeoutWrapper, in by_kind and in the trace); the fixtures of
    resilience_specs.TRACED with their full trace.
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

import fault_specs as FS  # noqa: E402
import health_specs as HS  # noqa: E402
import rate_limiter_specs as RS  # noqa: E402
import resilience_specs as XS  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the reference's import path; the stream plugs and the trace classifier)
import make_golden_rate_limiter as MGR  # noqa: E402
import make_golden_faults as MGF  # noqa: E402
import make_golden_health as MGH  # noqa: E402
import happysimulator.faults as ref_faults  # noqa: E402
from happysimulator import Server, Simulation, Sink  # noqa: E402
from happysimulator.components.load_balancer import HealthChecker  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from happysimulator.components.resilience import Bulkhead, TimeoutWrapper  # noqa: E402
from happysimulator.components.resilience.bulkhead import BulkheadStats  # noqa: E402
from happysimulator.components.resilience.timeout import TimeoutStats  # noqa: E402
from happysimulator.core.event import Event  # noqa: E402
from happysimulator.instrumentation.probe import Probe  # noqa: E402

EV_BH_REQ = MGH.EV_HC_TIMEOUT + 1
EV_BH_RESP, EV_BH_TIMEOUT, EV_TW_REQ, EV_TW_RESP, EV_TW_TIMEOUT = (EV_BH_REQ + k for k in range(1, 6))
WRAPPER_METRICS = ("active_count", "queue_depth", "available_permits", "in_flight_count")


def defaults():
    """Constructor state, properties, stats objects and error texts."""
    k = Sink("k")
    b, t = Bulkhead("b", k, max_concurrent=3), TimeoutWrapper("t", k, timeout=2.5)
    out = {}
    sb, st = b.stats, t.stats
    out["bulkhead"] = dict(fields=[b.max_concurrent, b.max_wait_queue, b.max_wait_time, b.active_count, b.queue_depth, b.available_permits,
                                   b._next_request_id, len(b._in_flight)], target_is=b.target is k,
                           downstream=[x.name for x in b.downstream_entities()], stats_type=type(sb).__name__,
                           stats_fields=[f for f in BulkheadStats.__dataclass_fields__],
                           stats=[getattr(sb, f) for f in BulkheadStats.__dataclass_fields__])
    out["timeout"] = dict(fields=[t.timeout, t.in_flight_count, t._next_request_id], target_is=t.target is k,
                          downstream=[x.name for x in t.downstream_entities()], stats_type=type(st).__name__,
                          stats_fields=[f for f in TimeoutStats.__dataclass_fields__], stats=[getattr(st, f) for f in TimeoutStats.__dataclass_fields__])
    for key, obj, attr in (("bulkhead", sb, "total_requests"), ("timeout", st, "total_requests")):
        try:
            setattr(obj, attr, 1)
            out[key]["stats_frozen"] = False
        except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
            out[key]["stats_frozen"] = type(e).__name__
    errors = []
    for kw in (dict(max_concurrent=0), dict(max_concurrent=-2), dict(max_concurrent=1, max_wait_queue=-1), dict(max_concurrent=1, max_wait_time=0),
               dict(max_concurrent=1, max_wait_time=-0.5), dict(max_concurrent=0, max_wait_queue=-1), dict(max_concurrent=1, max_wait_queue=0, max_wait_time=None)):
        try:
            Bulkhead("x", k, **kw)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["bulkhead"]["errors"] = errors
    errors = []
    for timeout in (0, -1.5, 0.0, 1e-9):
        try:
            TimeoutWrapper("x", k, timeout=timeout)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["timeout"]["errors"] = errors
    return out


class _Reference(MGR._Reference):
    def probe(self, target, metric, interval):
        if metric not in WRAPPER_METRICS:
            return super().probe(target, metric, interval)
        probe, data = Probe.on(target, metric, interval=interval)
        data._ns = []

        def add_stat(value, time, _orig=data.add_stat, _d=data):
            _d._ns.append((time.nanoseconds, value))
            _orig(value, time)

        data.add_stat = add_stat
        self.probe_data.append(data)
        return probe


def run_case(spec, want_trace=False):
    """The reference's run of one spec.  Trace nodes: Sources, Probes, then the entities (servers + lbs + routers + links + limiters
    + sinks + wrappers + checkers); trace kinds: make_golden_health's (0 .. 21), then 22 .. 27 = the wrappers' six."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    F = _Reference(spec)
    pools, sources, probes, entities = XS.wire(spec, F, Bulkhead, TimeoutWrapper, HealthChecker)
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
    by_kind = np.zeros(EV_TW_TIMEOUT + 1, np.int64)
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
        elif isinstance(e.target, Bulkhead):
            k, nd = {"_bh_response": EV_BH_RESP, "_bh_timeout": EV_BH_TIMEOUT}.get(et, EV_BH_REQ), node_of[id(e.target)]
        elif isinstance(e.target, TimeoutWrapper):
            k, nd = {"_tw_response": EV_TW_RESP, "_tw_timeout": EV_TW_TIMEOUT}.get(et, EV_TW_REQ), node_of[id(e.target)]
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
    for on, t_s in spec.get("schedule") or []:
        sim.schedule(Event(time=MG._at(spec, t_s), event_type="Request", target=pools[on[0]][on[1]]))
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
    out.update(FS.fault_results(fs, XS.fault_targets(pools)))
    out.update(HS.health_results(spec, pools))
    out.update(XS.wrapper_results(pools))
    out["fault_events"] = int(by_kind[MGF.EV_FAULT_ON] + by_kind[MGF.EV_FAULT_OFF])
    out["events_cancelled"] = int(summary.events_cancelled)
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out


def main():
    import resilience_reference as XR

    cases = {XR.key("defaults"): defaults()}
    for spec in XS.all_specs():
        sim, _pools = XS.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_wrappers, spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[XR.key("case", spec)] = run_case(spec, want_trace=spec["name"] in XS.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        print(spec["name"], res["total_events"], res["by_kind"][EV_BH_REQ:].tolist(), res["wrap_stats"][:, :5].tolist(), res["crashed"].sum(), flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[XR.key("case", XS.FIXTURES[name])]  # noqa: E731
    r = get("bulkhead_link_twenty_requests")              # 20 Requests through Bulkhead -> NetworkLink -> Server: 38 `_bh_response` Events
    assert r["by_kind"][EV_BH_REQ] == 20 and r["by_kind"][EV_BH_RESP] == 38, r["by_kind"][EV_BH_REQ:]
    r = get("paused_server_leaks_permits")                # every permit leaked during the pause: active_count == 4 and 3 queued at 10 s,
    assert r["wrap_stats"][0, 7] == 4 and r["wrap_stats"][0, 8] == 3 and r["wrap_stats"][0, 2] > 200, r["wrap_stats"]     # the rest rejected
    r = get("bulkhead_server_burst")
    assert r["wrap_stats"][0, 5] > 1                      # peak_concurrent above 1 in front of a Server
    r = get("timeout_response_after_the_wrappers_restart")
    assert r["wrap_stats"][0, 1] > 0 and r["wrap_stats"][0, 2] > 0
    r = get("timeout_wrapper_crash_without_restart")
    assert r["wrap_stats"][0, 3] > 0                      # entries stay in flight for ever
    r = get("expired_entries_skipped_after_a_wrapper_crash")
    assert r["wrap_stats"][0, 3] > 0
    assert len(XS.FIXTURES) >= 40 and len(XS.TRACED) == 6 and XS.N_RANDOM >= 120
    XR.write(cases)


if __name__ == "__main__":
    main()
