"""ON THE GPU BOX: LoadBalancer groups in ONE Simulation -- Source -> LoadBalancer -> three Servers -> Sink, a HealthChecker on the
LoadBalancer (interval 1 s, timeout 0.25 s) and one backend crashed and restarted per group at a per-group offset off the checkers'
grid -- the single-heap loop's health kinds (csrc/hs_graph.hip kEvHcCycle / kEvHcResp / kEvHcTimeout, the selection over the healthy
list) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps side by side).  Prints one
JSON line: events/s of the device and the device time; `wall_s` is Simulation.run() as a whole.  A demonstration: nothing exists to
compare the number with.

    python tools/health_profile.py [groups] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402

STRATEGIES = (hs.RoundRobin, hs.LeastConnections, hs.WeightedRoundRobin, hs.WeightedLeastConnections)


def build(n, end_s):
    sources, entities, lbs, checkers = [], [], [], []
    fs = hs.FaultSchedule()
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        servers = [hs.Server(f"srv{g}_{j}", service_time=hs.ExponentialLatency(0.05), downstream=sink) for j in range(3)]
        lb = hs.LoadBalancer(f"lb{g}", strategy=STRATEGIES[g % 4]())
        for j, s in enumerate(servers):
            lb.add_backend(s, weight=1 + (g + j) % 3)
        hc = hs.HealthChecker(f"hc{g}", lb, interval=1.0, timeout=0.25, healthy_threshold=2, unhealthy_threshold=3)
        sources.append(hs.Source.poisson(rate=20, target=lb, name=f"src{g}"))
        entities += servers + [lb, sink, hc]
        lbs.append(lb)
        checkers.append(hc)
        at = 1.0 + (g % 1999) * 0.000977 + 0.0000003               # (1 s .. 2.95 s, never on a cycle's or a timeout's nanosecond)
        fs.add(hs.CrashNode(f"srv{g}_{g % 3}", at, restart_at=at + 4.4))
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7, fault_schedule=fs)
    for hc in checkers:
        sim.schedule(hc.start())
    return sim, lbs, checkers


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 1.0)[0].run()                                         # (first touch of the library)
    sim, lbs, checkers = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    print(json.dumps(dict(what="Source.poisson(20) -> LoadBalancer -> 3 x Server(Exp(0.05)) -> Sink, a HealthChecker(1.0, 0.25, 2, 3) per "
                               "LoadBalancer, one backend crashed for 4.4 s per group; RoundRobin / LeastConnections / WeightedRoundRobin / "
                               "WeightedLeastConnections in turn",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, health_events=[int(v) for v in sim._health_by_kind],
                          fault_events=int(sim._fault_events_processed), device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), wall_s=round(wall, 3),
                          checks_performed=sum(c.stats.checks_performed for c in checkers),
                          checks_timed_out=sum(c.stats.checks_timed_out for c in checkers),
                          marked_unhealthy=sum(lb.stats.backends_marked_unhealthy for lb in lbs),
                          marked_healthy=sum(lb.stats.backends_marked_healthy for lb in lbs),
                          no_backend_available=sum(lb.stats.no_backend_available for lb in lbs))), flush=True)


if __name__ == "__main__":
    main()
