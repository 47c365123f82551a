#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for FaultSchedule with CrashNode / PauseNode (happysimulator/faults/) -- the
yardstick of tests/test_faults_host.py and tests/test_gpu_faults.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_faults.py          # writes tests/golden/live_faults/part_*.npz

Recorded (tests/recorded.py FAULTS reads them back; record_family.run_case is the run):
  * constructor defaults, properties, the stats quirks and the KeyError texts of the classes;
  * every spec of fault_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs of
    make_golden.py choosing the random numbers -- everything the rate_limiter family records, plus the final `_crashed`
    flag of every Source, Probe and entity, FaultSchedule.stats, events_cancelled and the fault Events processed (kinds 17 = a
    crash / pause, 18 = a restart / resume in by_kind and in the trace); the fixtures of fault_specs.TRACED with their full trace.
    by_kind counts every processed Event, one dropped at a crashed target included; lim_events counts per limiter the Events its
    handlers actually ran for.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed).
"""
from __future__ import annotations

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import fault_specs as FS  # noqa: E402
import graph_family as GF  # noqa: E402
import rate_limiter_specs as RS  # noqa: E402
import happysimulator.faults as ref_faults  # noqa: E402
from happysimulator import Instant, Server, Simulation, Sink, Source  # noqa: E402
from recorded import FAULTS as FR  # noqa: E402


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


def main():
    cases = {FR.key("defaults"): defaults()}
    kinds_hit, grid_hit = set(), 0
    for spec in FS.all_specs():
        sim, _pools = GF.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._faults, spec["name"]
        res = cases[FR.key("case", spec)] = RF.run_case(spec, "faults", want_trace=spec["name"] in FS.TRACED)
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
