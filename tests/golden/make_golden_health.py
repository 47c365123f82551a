#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for HealthChecker and LoadBalancer.mark_unhealthy / mark_healthy
(components/load_balancer/health_check.py, load_balancer.py:244-297) -- the yardstick of tests/test_health_host.py and
tests/test_gpu_health.py.  Run by hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_health.py          # writes tests/golden/live_health/part_*.npz

Recorded (tests/recorded.py HEALTH reads them back; record_family.run_case is the run):
  * constructor defaults, properties, stats and state objects and the ValueError texts of HealthChecker;
  * every spec of health_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs of
    make_golden.py choosing the random numbers -- everything the faults family records but the probe samples and the limiters, plus per LoadBalancer the health
    flag of every backend, its mark counts and WeightedRoundRobin's current weights, per checker its stats and per-backend states
    and pending check ids, and the checkers' Events processed (kinds 19 = a cycle, 20 = a response, 21 = a timeout in by_kind and in
    the trace); the fixtures of health_specs.TRACED with their full trace.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed): no case is left out.
"""
from __future__ import annotations

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import health_specs as HS  # noqa: E402
from happysimulator import Server  # noqa: E402
from happysimulator.components.load_balancer import HealthChecker, LoadBalancer  # noqa: E402
from happysimulator.components.load_balancer.health_check import BackendHealthState, HealthCheckStats  # noqa: E402
from recorded import HEALTH as HR  # noqa: E402


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


def main():
    cases = {HR.key("defaults"): defaults()}
    for spec in HS.all_specs():
        sim, _pools = GF.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_health, spec["name"]
        sim._general_prepare(sim._graph, False)            # ... and every scheduled Event of it
        res = cases[HR.key("case", spec)] = RF.run_case(spec, "health", want_trace=spec["name"] in HS.TRACED)
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
