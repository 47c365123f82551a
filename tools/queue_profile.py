"""ON THE GPU BOX: chains with queue policies in ONE Simulation -- Source.poisson(60) -> Server(c = 2, Exp(0.02), CoDelQueue(0.005, 0.02))
-> Server(Exp(0.012), AdaptiveLIFO(4, capacity 32)) -> Server(Exp(0.01), LIFOQueue(16)) -> Sink -- the single-heap loop's queue-policy
instantiation (csrc/hs_graph.hip hs_graph_run_batch_level<kLvQueues>: a pop that takes the newest item, a pop that drops the items behind the one
it delivers) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps side by side).  Prints
one JSON line: events/s of the device and the device time; `wall_s` is Simulation.run() as a whole.  A demonstration: nothing else
runs these policies, so the loop's ~2.5 us per event and heap is the only figure it can be set against.

    python tools/queue_profile.py [groups] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    sources, entities, chains = [], [], []
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        last = hs.Server(f"lifo{g}", service_time=hs.ExponentialLatency(0.01), queue_policy=hs.LIFOQueue(16), downstream=sink)
        mid = hs.Server(f"alifo{g}", service_time=hs.ExponentialLatency(0.012), queue_policy=hs.AdaptiveLIFO(4, capacity=32), downstream=last)
        first = hs.Server(f"codel{g}", concurrency=2, service_time=hs.ExponentialLatency(0.02), queue_policy=hs.CoDelQueue(0.005, 0.02), downstream=mid)
        sources.append(hs.Source.poisson(rate=60, target=first, name=f"src{g}"))
        entities += [first, mid, last, sink]
        chains.append((first, mid, last, sink))
    return hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7), chains


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 1.0)[0].run()                                         # (first touch of the library)
    sim, chains = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    heaps = max(sim._graph_parts, 1)
    codel = [c.queue_policy.stats for c, _a, _l, _s in chains]
    alifo = [a.queue_policy.stats for _c, a, _l, _s in chains]
    print(json.dumps(dict(what="Source.poisson(60) -> Server(c=2, Exp(0.02), CoDelQueue(0.005, 0.02)) -> Server(Exp(0.012), AdaptiveLIFO(4, 32)) -> "
                               "Server(Exp(0.01), LIFOQueue(16)) -> Sink per group; a demonstration: nothing else runs these policies, the loop's "
                               "~2.5 us per event and heap is the only figure to set it against",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), us_per_event_and_heap=round(dev_ms * 1e3 / (ev / heaps), 3),
                          wall_s=round(wall, 3), codel_dropped=sum(s.dropped for s in codel), codel_drop_intervals=sum(s.drop_intervals for s in codel),
                          alifo_mode_switches=sum(s.mode_switches for s in alifo), alifo_dequeued_lifo=sum(s.dequeued_lifo for s in alifo),
                          lifo_dropped=sum(l.stats_dropped for _c, _a, l, _s in chains), received=sum(k.events_received for _c, _a, _l, k in chains))),
          flush=True)


if __name__ == "__main__":
    main()
