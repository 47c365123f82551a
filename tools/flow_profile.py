"""ON THE GPU BOX: flow groups in ONE Simulation -- Source.poisson(40) -> GateController(closed for half of every second, queue 32) ->
ConveyorBelt(0.05, capacity 8) -> BatchProcessor(8, 0.02, timeout 0.1) -> Server -> Sink -- the single-heap loop's flow kinds
(csrc/hs_graph.hip kEvBpItem .. kEvGtClose: a gate that forwards its whole queue in one handler, a batch that leaves in one handler,
a timeout its processor cancels) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps
side by side).  Prints one JSON line: events/s of the device and the device time; `wall_s` is Simulation.run() as a whole.  A
demonstration: the loop's ~2.5 us per event and heap is the only figure it can be set against.

    python tools/flow_profile.py [groups] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    sources, entities, flows = [], [], []
    gates, sinks = [], []
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        server = hs.Server(f"srv{g}", service_time=hs.ExponentialLatency(0.01), downstream=sink)
        batch = hs.BatchProcessor(f"bp{g}", server, batch_size=8, process_time=0.02, timeout_s=0.1)
        belt = hs.ConveyorBelt(f"cv{g}", batch, 0.05, capacity=8)
        off = g * 0.000211 + 0.0000003              # (no two gates share a nanosecond: two parts' Events on one would be left to one heap)
        gate = hs.GateController(f"gt{g}", belt, schedule=[(k + 0.5 + off, k + 1.0 + off) for k in range(int(end_s))], initially_open=False,
                                 queue_capacity=32)
        sources.append(hs.Source.poisson(rate=40, target=gate, name=f"src{g}"))
        entities += [gate, belt, batch, server, sink]
        flows.append((gate, belt, batch))
        sinks.append(sink)
        gates.append(gate)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7)
    for gate in gates:
        for ev in gate.start_events():
            sim.schedule(ev)
    return sim, flows, sinks


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 1.0)[0].run()                                         # (first touch of the library)
    sim, flows, sinks = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    heaps = max(sim._graph_parts, 1)
    print(json.dumps(dict(what="Source.poisson(40) -> GateController(closed half of every second, queue 32) -> ConveyorBelt(0.05, 8) -> "
                               "BatchProcessor(8, 0.02, timeout 0.1) -> Server(Exp(0.01)) -> Sink per group; a demonstration: the loop's "
                               "~2.5 us per event and heap is the only figure to set it against",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, flow_events=[int(v) for v in sim._flow_by_kind],
                          events_cancelled=int(summary.events_cancelled), device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), us_per_event_and_heap=round(dev_ms * 1e3 / (ev / heaps), 3),
                          wall_s=round(wall, 3),
                          passed_through=sum(g.stats.passed_through for g, _c, _b in flows), gate_rejected=sum(g.stats.rejected for g, _c, _b in flows),
                          conveyor_rejected=sum(c.stats.items_rejected for _g, c, _b in flows),
                          batches=sum(b.stats.batches_processed for _g, _c, b in flows), batch_timeouts=sum(b.stats.timeouts for _g, _c, b in flows),
                          received=sum(k.events_received for k in sinks))), flush=True)


if __name__ == "__main__":
    main()
