"""ON THE GPU BOX: Client groups in ONE Simulation -- Source.poisson(40) -> Client(timeout, ExponentialBackoff) -> NetworkLink -> Server
-> Sink, the Server crashed for a second at a per-group offset: a retry storm against a dead backend and the recovery after its restart
-- the single-heap loop's client kinds (csrc/hs_graph.hip kEvClReq .. kEvClTimeout, the completion hook at the end of a link's transit
and at the Server's enqueue) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps side
by side).  Prints one JSON line: events/s of the device and the device time; `wall_s` is Simulation.run() as a whole.  A
demonstration: nothing exists to compare the number with.

    python tools/client_profile.py [groups] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    sources, entities, clients = [], [], []
    fs = hs.FaultSchedule()
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        server = hs.Server(f"srv{g}", service_time=hs.ExponentialLatency(0.02), downstream=sink)
        link = hs.NetworkLink(f"link{g}", latency=hs.ConstantLatency(0.03), jitter=hs.ExponentialLatency(0.02), egress=server)
        c = hs.Client(f"cl{g}", link, timeout=0.15, retry_policy=hs.ExponentialBackoff(max_attempts=5, initial_delay=0.05, max_delay=0.8))
        sources.append(hs.Source.poisson(rate=40, target=c, name=f"src{g}"))
        entities += [c, link, server, sink]
        clients.append(c)
        at = 2.0 + (g % 1999) * 0.000977 + 0.0000003
        fs.add(hs.CrashNode(f"srv{g}", at=at, restart_at=at + 1.0))      # Requests dropped at the crashed Server: no hook, the timeout fires
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7, fault_schedule=fs)
    return sim, clients


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 1.0)[0].run()                                         # (first touch of the library)
    sim, clients = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    print(json.dumps(dict(what="Source.poisson(40) -> Client(0.15, ExponentialBackoff(5, 0.05, 0.8)) -> NetworkLink(0.03 + Exp(0.02)) -> "
                               "Server(Exp(0.02)) -> Sink, the Server crashed for 1 s per group; a demonstration: nothing exists to compare "
                               "the number with",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, client_events=[int(v) for v in sim._client_by_kind],
                          fault_events=int(sim._fault_events_processed), device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), wall_s=round(wall, 3),
                          requests_sent=sum(c.stats.requests_sent for c in clients),
                          responses=sum(c.stats.responses_received for c in clients),
                          timeouts=sum(c.stats.timeouts for c in clients), retries=sum(c.stats.retries for c in clients),
                          failures=sum(c.stats.failures for c in clients), in_flight_at_the_end=sum(c.in_flight_count for c in clients))), flush=True)


if __name__ == "__main__":
    main()
