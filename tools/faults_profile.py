"""ON THE GPU BOX: 65 536 disconnected Source -> Server -> Sink chains in ONE Simulation, 10 s, every Server paused for one second
(PauseNode) at a per-chain offset off the tick grid -- the single-heap loop's fault kinds and its drop at dispatch
(csrc/hs_graph.hip kEvFaultOn / kEvFaultOff) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to
2 048 heaps side by side).  Prints two JSON lines: the run with faults, and the same chains without a fault schedule on the same
loop (without one a Simulation of plain chains goes to the station engine, so that run is lowered to the single heap by hand).
`wall_s` is Simulation.run() as a whole; `device_ms` is the launch alone.

    python tools/faults_profile.py [chains] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402
from happy_simulator_amd.graph_engine import lower_general  # noqa: E402


def build(n, end_s, faults=True):
    sources, entities, servers = [], [], []
    fs = hs.FaultSchedule()
    for i in range(n):
        sink = hs.Sink(f"sink{i}")
        srv = hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink)
        sources.append(hs.Source.poisson(rate=10, target=srv, name=f"src{i}"))
        entities += [srv, sink]
        servers.append(srv)
        start = 1.0 + (i % 7919) * 0.000977 + 0.0000003             # (1 s .. 8.74 s, never a multiple of a round interval)
        fs.add(hs.PauseNode(f"srv{i}", start, start + 1.0))
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7,
                        fault_schedule=fs if faults else None)
    if not faults:
        sim._graph = lower_general(sim._sources, sim._entities, sim._probes)
        sim._station_refusal = "forced onto the single-heap loop (tools/faults_profile.py)"
    return sim, servers


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(64, 1.0)[0].run()                                        # (first touch of the library)
    for faults in (True, False):
        sim, servers = build(n, end_s, faults)
        t0 = time.monotonic()
        summary = sim.run()
        wall = time.monotonic() - t0
        dev_ms = sim._engine_summary.last_run_ms
        ev = summary.total_events_processed
        print(json.dumps(dict(what="Source.poisson(10) -> Server(Exp(0.05)) -> Sink" + (", every Server paused for 1 s" if faults else ", no fault schedule"),
                              faults=faults, chains=n, end_s=end_s, parts=sim._graph_parts, events=ev,
                              fault_events=int(getattr(sim, "_fault_events_processed", 0)), device_ms=round(dev_ms, 3),
                              device_events_per_s=round(ev / (dev_ms / 1e3), 1), wall_s=round(wall, 3),
                              accepted=sum(s.stats_accepted for s in servers), completed=sum(s._requests_completed for s in servers))), flush=True)


if __name__ == "__main__":
    main()
