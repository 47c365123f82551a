"""ON THE GPU BOX: the degraded-network experiment in ONE Simulation -- Source.poisson(60) -> Client(timeout 80 ms, FixedRetry(3, 50 ms)) ->
NetworkLink(20 ms + Exp(10 ms)) -> Server(c = 2, Exp(0.01)) -> Sink per group, every link registered in one Network, with
InjectLatency(+100 ms) from 2 s to 4 s and InjectPacketLoss(0.3) from 5 s to 7 s on every link -- the single-heap loop's link-fault
instantiation (csrc/hs_graph.hip hs_graph_run_batch_level<kLvLinkFaults>) with the data-parallel dimension a Simulation has: its parts
(hs_graph_run_parts, up to 2 048 heaps side by side).  Prints one JSON line: events/s of the device and the device time; `wall_s` is
Simulation.run() as a whole.  A demonstration: nothing else runs these faults, so the loop's ~2.5 us per event and heap is the only
figure it can be set against.

    python tools/link_fault_profile.py [groups] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    sources, entities, chains = [], [], []
    net = hs.Network("net")
    fs = hs.FaultSchedule()
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        server = hs.Server(f"srv{g}", concurrency=2, service_time=hs.ExponentialLatency(0.01), downstream=sink)
        link = hs.NetworkLink(f"link{g}", latency=hs.ConstantLatency(0.02), jitter=hs.ExponentialLatency(0.01))
        client = hs.Client(f"cl{g}", link, timeout=0.08, retry_policy=hs.FixedRetry(3, 0.05))
        net.add_link(client, server, link)
        fs.add(hs.InjectLatency(client.name, server.name, 100.0, 2.0, 4.0))
        fs.add(hs.InjectPacketLoss(client.name, server.name, 0.3, 5.0, 7.0))
        sources.append(hs.Source.poisson(rate=60, target=client, name=f"src{g}"))
        entities += [client, link, server, sink]
        chains.append((client, link, server, sink))
    return hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities + [net], fault_schedule=fs, seed=7), chains


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
    print(json.dumps(dict(what="Source.poisson(60) -> Client(0.08, FixedRetry(3, 0.05)) -> NetworkLink(0.02 + Exp(0.01)) -> Server(c=2, Exp(0.01)) -> Sink "
                               "per group, InjectLatency(+100 ms, 2 s .. 4 s) and InjectPacketLoss(0.3, 5 s .. 7 s) on every link; a demonstration: "
                               "nothing else runs these faults, the loop's ~2.5 us per event and heap is the only figure to set it against",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), us_per_event_and_heap=round(dev_ms * 1e3 / (ev / heaps), 3),
                          wall_s=round(wall, 3), packets_dropped=sum(l.packets_dropped for _c, l, _s, _k in chains),
                          loss_draws=sum(l._loss_draws for _c, l, _s, _k in chains), client_timeouts=sum(c.stats.timeouts for c, _l, _s, _k in chains),
                          client_retries=sum(c.stats.retries for c, _l, _s, _k in chains), received=sum(k.events_received for _c, _l, _s, k in chains))),
          flush=True)


if __name__ == "__main__":
    main()
