#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for FaultSchedule with CrashNode / PauseNode (happysimulator/faults/) -- the
yardstick of tests/test_faults_host.py and tests/test_gpu_faults.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_faults.py          # writes tests/golden/live_faults/part_*.npz

Recorded (tests/fault_reference.py reads them back):
  * constructor defaults, properties, the stats quirks and the KeyError texts of the classes;
  * every spec of fault_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs of
    make_golden.py choosing the random numbers -- everything make_golden_rate_limiter.run_case records, plus the final `_crashed`
    flag of every Source, Probe and entity, FaultSchedule.stats, events_cancelled and the fault Events processed (kinds 17 = a
    crash / pause, 18 = a restart / resume in by_kind and in the trace); the fixtures of fault_specs.TRACED with their full trace.
    by_kind counts every processed Event, one dropped at a crashed target included; lim_events counts per limiter the Events its
    handlers actually ran for.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed).
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
import rate_limiter_specs as RS  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the reference's import path; the stream plugs and the trace classifier)
import make_golden_rate_limiter as MGR  # noqa: E402
import happysimulator.faults as ref_faults  # noqa: E402
from happysimulator import Instant, Server, Simulation, Sink, Source  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from happysimulator.core.event import Event  # noqa: E402

EV_FAULT_ON, EV_FAULT_OFF = MGR.EV_LIM_POLL + 1, MGR.EV_LIM_POLL + 2
_ON = ("fault.crash:", "fault.pause:")
_OFF = ("fault.restart:", "fault.resume:")


def defaults():
    """Constructor state, properties, stats quirks and error texts."""
    out = {}
    c, p = ref_faults.CrashNode("a", at=1.0), ref_faults.PauseNode("b", start=1.0, end=2.0)
    out["crash"] = dict(fields=[c.entity_name, c.at, c.restart_at], repr=repr(c), eq=c == ref_faults.CrashNode("a", 1.0, None))
    out["pause"] = dict(fields=[p.entity_name, p.start, p.end], repr=repr(p))
    for key, obj, attr in (("crash", c, "at"), ("pause", p, "start")):
        try:
            setattr(obj, attr, 5.0)
            out[key]["frozen"] = False
        except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
            out[key]["frozen"] = type(e).__name__
    fs = ref_faults.FaultSchedule()
    h = fs.add(c)
    fs.add(p)
    st0 = fs.stats
    out["schedule"] = dict(name=fs.name, named=ref_faults.FaultSchedule("chaos").name, stats_type=type(st0).__name__,
                           stats=[st0.faults_scheduled, st0.faults_activated, st0.faults_deactivated, st0.faults_cancelled],
                           handle_fault_is=h.fault is c, handle_cancelled=h.cancelled, handle_events=len(h._events))
    h.cancel()
    h.cancel()
    st1 = fs.stats
    out["schedule"]["stats_after_cancel"] = [st1.faults_scheduled, st1.faults_activated, st1.faults_deactivated, st1.faults_cancelled]
    out["schedule"]["handle_cancelled_after"] = h.cancelled
    try:
        st1.faults_scheduled = 3
        out["schedule"]["stats_frozen"] = False
    except Exception as e:  # noqa: BLE001
        out["schedule"]["stats_frozen"] = type(e).__name__
    # names: an unknown one, and an entity that is reachable but not listed (faults/schedule.py:112-135)
    sink, hidden = Sink("sink"), Sink("hidden")
    srv = Server("srv", downstream=hidden)
    errors = {}
    for label, name in (("unknown", "nobody"), ("unlisted", "hidden")):
        fs2 = ref_faults.FaultSchedule()
        fs2.add(ref_faults.CrashNode(name, at=1.0))
        try:
            Simulation(end_time=Instant.from_seconds(1), sources=[Source.constant(rate=1, target=srv, name="src")], entities=[srv, sink],
                       fault_schedule=fs2)
            errors[label] = None
        except KeyError as e:
            errors[label] = [type(e).__name__, str(e)]
    out["key_errors"] = errors
    # the Events come into being in Simulation.__init__: two per restartable fault, crash before restart, daemons
    fs3 = ref_faults.FaultSchedule()
    h3 = fs3.add(ref_faults.CrashNode("srv", at=1.0, restart_at=2.0))
    h4 = fs3.add(ref_faults.CrashNode("sink", at=1.5))
    Simulation(end_time=Instant.from_seconds(1), sources=[Source.constant(rate=1, target=srv, name="src")], entities=[srv, sink, hidden],
               fault_schedule=fs3)
    out["events"] = dict(types=[e.event_type for e in h3._events + h4._events], daemon=[e.daemon for e in h3._events + h4._events],
                         times_ns=[e.time.nanoseconds for e in h3._events + h4._events],
                         sort_index=[e._sort_index for e in h3._events + h4._events])
    return out


def run_case(spec, want_trace=False):
    """The reference's run of one spec.  Trace nodes: Sources, Probes, then the entities (servers + lbs + routers + links + limiters
    + sinks); trace kinds: make_golden.EV, 15 / 16 = a limiter's two handlers, 17 / 18 = a fault Event that sets / clears the flag
    (node: the entity it names)."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    F = MGR._Reference(spec)
    pools, sources, probes, entities = RS.wire(spec, F)
    pools["probe"] = probes
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
    by_name = {x.name: node_of[id(x)] for x in entities + sources + probes}        # (the schedule's own dict order: the last wins)
    cb_probe = {id(p._event_provider.data_sink): len(sources) + j for j, p in enumerate(probes)}
    by_kind = np.zeros(EV_FAULT_OFF + 1, np.int64)
    lim_events = np.zeros((len(lims), 2), np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop
    state = dict(cur=sim._start_time, cancelled=0, skipped=0)

    def pop():
        e = orig_pop()
        if by_kind.sum() >= MGR.MAX_EVENTS:
            raise MGR.Livelock(spec["name"])
        if e.cancelled:                                   # skipped, counted in events_cancelled (core/simulation.py:475-477)
            state["cancelled"] += 1
            return e
        if e.time < state["cur"]:                         # time travel: skipped, not counted (:480-489)
            state["skipped"] += 1
            return e
        state["cur"] = e.time
        et = e.event_type
        if et.startswith(_ON) or et.startswith(_OFF):
            k, nd = (EV_FAULT_ON if et.startswith(_ON) else EV_FAULT_OFF), by_name[et.split(":", 1)[1]]
        elif isinstance(e.target, RateLimitedEntity):
            poll = et == f"rate_limit_poll::{e.target.name}"
            k, nd = (MGR.EV_LIM_POLL if poll else MGR.EV_LIM_REQUEST), node_of[id(e.target)]
            if not getattr(e.target, "_crashed", False):       # (popped and counted, but its handler never ran: core/event.py:261)
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
    for (kind, idx), t_s in spec.get("schedule") or []:
        sim.schedule(Event(time=MG._at(spec, t_s), event_type="Request", target=pools[kind][idx]))
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
    out.update(FS.fault_results(fs, FS.fault_targets(pools)))
    out["fault_events"] = int(by_kind[EV_FAULT_ON] + by_kind[EV_FAULT_OFF])
    out["events_cancelled"] = int(summary.events_cancelled)
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out


def main():
    import fault_reference as FR

    cases = {FR.key("defaults"): defaults()}
    kinds_hit, grid_hit = set(), 0
    for spec in FS.all_specs():
        sim, _pools = FS.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._faults, spec["name"]
        res = cases[FR.key("case", spec)] = run_case(spec, want_trace=spec["name"] in FS.TRACED)
        for ft in spec["faults"]:
            if not isinstance(ft["on"], str):
                kinds_hit.add(ft["on"][0])
        grid_hit += spec["name"].startswith("fault_graph_") and int(spec["name"].rsplit("_", 1)[1]) % FS.GRID_SHARE == 0
        print(spec["name"], res["total_events"], res["fault_events"], res["crashed"].tolist(), res["events_cancelled"], res["time_travel"],
              flush=True)
    missing = [p for p in FS.POOLS if p not in kinds_hit]
    assert not missing, f"no fault on these entity kinds: {missing}"
    assert grid_hit == len(range(0, FS.N_RANDOM, FS.GRID_SHARE))
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[FR.key("case", FS.FIXTURES[name])]  # noqa: E731
    r = get("fault_is_the_event_beyond_the_end")
    assert r["final_ns"] == 3_000_010_000 and r["crashed"].sum() == 1 and r["fault_events"] == 1, r["final_ns"]
    r = get("fault_later_than_the_event_beyond_the_end")
    assert r["fault_events"] == 0 and r["crashed"].sum() == 0
    r = get("cancelled_before_construction")
    assert r["fault_stats"].tolist() == [1, 0, 0, 1] and r["fault_events"] == 2 and r["events_cancelled"] == 0
    r = get("cancelled_after_construction")
    assert r["fault_stats"].tolist() == [2, 0, 0, 1] and r["fault_events"] == 2 and r["events_cancelled"] == 2
    r = get("fault_before_start")
    assert r["time_travel"] == 1 and r["fault_events"] == 3
    r = get("auto_terminate_pending_restart")
    assert r["pending_events"] == 1 and r["crashed"].sum() == 1 and r["fault_events"] == 1
    r = get("source_crash_restart")
    assert r["crashed"].sum() == 0 and r["sink_t_ns"].max() < 4 * 10 ** 9        # restarted, and generates nothing any more
    r = get("overlapping_crash_and_pause")
    assert r["crashed"].sum() == 0 and r["fault_events"] == 4
    for k in RS.POLICIES:
        r = get(f"limiter_{k}_crash")
        assert r["lim_stats"][0, 5] == 1 and r["lim_stats"][0, 4] > 0, (k, r["lim_stats"])     # _poll_scheduled stays set, the queue never drains
    FR.write(cases)


if __name__ == "__main__":
    main()
