#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for HealthChecker and LoadBalancer.mark_unhealthy / mark_healthy
(components/load_balancer/health_check.py, load_balancer.py:244-297) -- the yardstick of tests/test_health_host.py and
tests/test_gpu_health.py.  Run by hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_health.py          # writes tests/golden/live_health/part_*.npz

Recorded (tests/health_reference.py reads them back):
  * constructor defaults, properties, stats and state objects and the ValueError texts of HealthChecker;
  * every spec of health_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs of
    make_golden.py choosing the random numbers -- everything make_golden_faults.run_case records, plus per LoadBalancer the health
    flag of every backend, its mark counts and WeightedRoundRobin's current weights, per checker its stats and per-backend states
    and pending check ids, and the checkers' Events processed (kinds 19 = a cycle, 20 = a response, 21 = a timeout in by_kind and in
    the trace); the fixtures of health_specs.TRACED with their full trace.
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
import make_golden as MG  # noqa: E402  (installs the reference's import path; the stream plugs and the trace classifier)
import make_golden_rate_limiter as MGR  # noqa: E402
import make_golden_faults as MGF  # noqa: E402
import happysimulator.faults as ref_faults  # noqa: E402
from happysimulator import Instant, Server, Simulation, Sink  # noqa: E402
from happysimulator.components.load_balancer import HealthChecker, LoadBalancer  # noqa: E402
from happysimulator.components.load_balancer.health_check import BackendHealthState, HealthCheckStats  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402

EV_HC_CYCLE, EV_HC_RESP, EV_HC_TIMEOUT = MGF.EV_FAULT_OFF + 1, MGF.EV_FAULT_OFF + 2, MGF.EV_FAULT_OFF + 3
_HC_KIND = {"_health_check_cycle": EV_HC_CYCLE, "_health_check_response": EV_HC_RESP, "_health_check_timeout": EV_HC_TIMEOUT}


def defaults():
    """Constructor state, properties, stats / state objects and error texts."""
    lb = LoadBalancer("lb", backends=[Server("a"), Server("b")])
    hc = HealthChecker("hc", lb)
    st, bs = hc.stats, hc.get_backend_state(lb.all_backends[0])
    out = dict(fields=[hc.interval, hc.timeout, hc.healthy_threshold, hc.unhealthy_threshold, hc._check_event_type, hc.is_running],
               lb_is=hc.load_balancer is lb, downstream=[x.name for x in hc.downstream_entities()],
               stats_type=type(st).__name__, stats_fields=[f for f in HealthCheckStats.__dataclass_fields__],
               stats=[st.checks_performed, st.checks_passed, st.checks_failed, st.checks_timed_out, st.backends_marked_healthy,
                      st.backends_marked_unhealthy],
               state_type=type(bs).__name__, state_fields=[f for f in BackendHealthState.__dataclass_fields__],
               state=[bs.consecutive_successes, bs.consecutive_failures, bs.last_check_time is None, bs.last_check_passed is None, bs.is_checking],
               state_by_unknown_name=hc.get_backend_state_by_name("nobody") is None)
    try:
        st.checks_performed = 1
        out["stats_frozen"] = False
    except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
        out["stats_frozen"] = type(e).__name__
    ev = hc.start()
    out["start"] = dict(event_type=ev.event_type, time_ns=ev.time.nanoseconds, target_is=ev.target is hc, daemon=ev.daemon,
                        running=hc.is_running)
    hc.stop()
    out["stopped"] = hc.is_running
    errors = []
    for kw in (dict(interval=0), dict(interval=-1.5), dict(timeout=0), dict(timeout=-2), dict(interval=1.0, timeout=1.0),
               dict(interval=1.0, timeout=2.5), dict(healthy_threshold=0), dict(unhealthy_threshold=0), dict(interval=0, timeout=0)):
        try:
            HealthChecker("x", lb, **kw)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["errors"] = errors
    # the LoadBalancer's marks (load_balancer.py:244-297)
    a, b = lb.all_backends
    lb.mark_unhealthy(a)
    lb.mark_unhealthy(a)
    lb.mark_unhealthy(Server("stranger"))
    s1 = lb.stats
    out["marks"] = dict(after_unhealthy=[s1.backends_marked_unhealthy, s1.backends_marked_healthy, lb.healthy_count],
                        healthy=[x.name for x in lb.healthy_backends], unhealthy=[x.name for x in lb.unhealthy_backends],
                        info=[lb.get_backend_info(a).is_healthy, lb.get_backend_info(b).is_healthy])
    lb.mark_healthy(a)
    lb.mark_healthy(b)
    s2 = lb.stats
    out["marks"]["after_healthy"] = [s2.backends_marked_unhealthy, s2.backends_marked_healthy, lb.healthy_count]
    return out


def run_case(spec, want_trace=False):
    """The reference's run of one spec.  Trace nodes: Sources, Probes, then the entities (servers + lbs + routers + links + limiters
    + sinks + checkers); trace kinds: make_golden_faults' (0 .. 18), then 19 / 20 / 21 = a checker's cycle / response / timeout."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    F = MGR._Reference(spec)
    pools, sources, probes, entities = HS.wire(spec, F, HealthChecker)
    FS.apply_names(spec, pools)
    servers, sinks, links, routers, lbs, lims = (pools[k] for k in ("server", "sink", "link", "router", "lb", "limiter"))
    fs, handles = FS.make_schedule(ref_faults, spec, pools)
    early = HS.early_starts(spec, pools)
    sim = Simulation(start_time=MG._start(spec), sources=sources, entities=entities, fault_schedule=fs, end_time=MG._at(spec, spec["end_s"]),
                     **({"probes": probes} if probes else {}))
    FS.cancel_after(spec, handles)
    HS.start_checkers(spec, pools, sim, early)
    node_of = {}
    for i, x in enumerate(sources + probes):
        node_of[id(x)] = i
    first = len(sources) + len(probes)
    for i, x in enumerate(entities):
        node_of[id(x)] = first + i
        if isinstance(x, Server):
            for part in (x._queue, x._driver, x._worker):
                node_of[id(part)] = first + i
    by_name = {x.name: node_of[id(x)] for x in entities + sources + probes}
    by_kind = np.zeros(EV_HC_TIMEOUT + 1, np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop
    state = dict(cur=sim._start_time, cancelled=0, skipped=0, probe=None, probe_drops=0)

    def settle_probe():
        # the Event handled since the last pop was a probe at a live Server: did its queue refuse it?
        if state["probe"] is not None:
            srv, before = state["probe"]
            state["probe_drops"] += int(srv.stats_dropped > before)
            state["probe"] = None

    def pop():
        settle_probe()
        e = orig_pop()
        if by_kind.sum() >= MGR.MAX_EVENTS:
            raise MGR.Livelock(spec["name"])
        if e.cancelled:
            state["cancelled"] += 1
            return e
        if e.time < state["cur"]:                         # time travel: skipped, not counted (core/simulation.py:480-489)
            state["skipped"] += 1
            return e
        state["cur"] = e.time
        et = e.event_type
        if et.startswith(MGF._ON) or et.startswith(MGF._OFF):
            k, nd = (MGF.EV_FAULT_ON if et.startswith(MGF._ON) else MGF.EV_FAULT_OFF), by_name[et.split(":", 1)[1]]
        elif isinstance(e.target, HealthChecker):
            k, nd = _HC_KIND[et], node_of[id(e.target)]
        elif isinstance(e.target, RateLimitedEntity):
            k, nd = (MGR.EV_LIM_POLL if et == f"rate_limit_poll::{e.target.name}" else MGR.EV_LIM_REQUEST), node_of[id(e.target)]
        else:
            k, nd = MG.classify(e, node_of)
        by_kind[k] += 1
        if et == "health_check" and isinstance(e.target, Server) and not getattr(e.target, "_crashed", False):
            state["probe"] = (e.target, e.target.stats_dropped)
        if want_trace:
            trace.append((e.time.nanoseconds, k, nd, e._sort_index))
        return e

    heap.pop = pop
    summary = sim.run()
    settle_probe()
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
    out.update(FS.fault_results(fs, HS.fault_targets(pools)))
    out.update(HS.health_results(spec, pools))
    out["health_events"] = by_kind[EV_HC_CYCLE:].copy()
    out["probe_drops"] = int(state["probe_drops"])                # probes a full bounded queue refused (their checks pass all the same)
    out["events_cancelled"] = int(summary.events_cancelled)
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out


def main():
    import health_reference as HR

    cases = {HR.key("defaults"): defaults()}
    for spec in HS.all_specs():
        sim, _pools = HS.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_health, spec["name"]
        sim._general_prepare(sim._graph, False)            # ... and every scheduled Event of it
        res = cases[HR.key("case", spec)] = run_case(spec, want_trace=spec["name"] in HS.TRACED)
        assert res["total_events"] <= 20_000, (spec["name"], res["total_events"])
        print(spec["name"], res["total_events"], res["health_events"].tolist(), res["lb_marks"].tolist(), res["checker_stats"].tolist()[:1],
              res["crashed"].sum(), res["probe_drops"], flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[HR.key("case", HS.FIXTURES[name])]  # noqa: E731
    r = get("crash_then_restart_of_one_backend")
    assert r["checker_stats"][0, 0] == 63 and r["checker_stats"][0, 3] == 6 and r["lb_marks"][0, :2].tolist() == [1, 1], r["checker_stats"]
    r = get("all_backends_down_then_one_back")
    assert r["lb_stats"][0, 3] > 0 and r["lb_marks"][0, 1] >= 1
    r = get("probe_meets_a_full_bounded_queue")
    assert r["probe_drops"] >= 1 and r["checker_stats"][0, 2] == 0 and r["checker_stats"][0, 1] >= r["checker_stats"][0, 0] - 2, r["probe_drops"]
    for name in HS.WIDE:                                   # the slots marked unhealthy before the run return mid-run, not at once
        r, sp = get(name), HS.FIXTURES[name]
        nb = len(sp["servers"])
        back = HS.wide_returning(sp)
        assert len(back) >= len(sp["unhealthy"]) - 1 and r["lb_marks"][0, 0] >= len(sp["unhealthy"]) + 1 and r["lb_marks"][0, 1] == len(back), (name, r["lb_marks"])
        assert all(r["checker_states"][q, 0] >= 4 and r["lb_healthy"][q] for q in back), name
        assert sum(r["lb_backend_total_requests"][q] for q in back) > 0, name
    r = get("checker_crash_with_restart")
    assert r["checker_states"][:, 4].sum() > 0                                        # backends stay is_checking
    r = get("stop_before_run")
    assert r["checker_stats"][0, 0] == 0 and r["health_events"].tolist() == [1, 0, 0]
    r = get("start_scheduled_twice")
    assert r["health_events"][0] > get("crash_then_restart_of_one_backend")["health_events"][0]
    r = get("early_start_before_a_later_start_time")
    assert r["time_travel"] == 1 and r["health_events"].sum() == 0
    HR.write(cases)


if __name__ == "__main__":
    main()
