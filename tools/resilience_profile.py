"""ON THE GPU BOX: wrapper groups in ONE Simulation -- Source -> Bulkhead -> NetworkLink -> Server -> Sink, every other group with a
TimeoutWrapper in the Bulkhead's place, and the wrapper's target -- the link -- paused for a second at a per-group offset -- the single-heap loop's
resilience kinds (csrc/hs_graph.hip kEvBhReq .. kEvTwTimeout, the completion hook at the end of a link's transit and at the Server's
enqueue) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps side by side).  Prints
one JSON line: events/s of the device and the device time; `wall_s` is Simulation.run() as a whole.  A demonstration: nothing exists
to compare the number with.

    python tools/resilience_profile.py [groups] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    sources, entities, wrappers = [], [], []
    fs = hs.FaultSchedule()
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        server = hs.Server(f"srv{g}", service_time=hs.ExponentialLatency(0.02), downstream=sink)
        link = hs.NetworkLink(f"link{g}", latency=hs.ConstantLatency(0.03), jitter=hs.ExponentialLatency(0.02), egress=server)
        w = (hs.TimeoutWrapper(f"tw{g}", link, timeout=0.08) if g % 2 else
             hs.Bulkhead(f"bh{g}", link, max_concurrent=4, max_wait_queue=3, max_wait_time=0.5))
        sources.append(hs.Source.poisson(rate=40, target=w, name=f"src{g}"))
        entities += [w, link, server, sink]
        wrappers.append(w)
        at = 2.0 + (g % 1999) * 0.000977 + 0.0000003
        fs.add(hs.PauseNode(f"link{g}", at, at + 1.0))               # Requests dropped at the paused link: permits leak, ids time out
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7, fault_schedule=fs)
    return sim, wrappers


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 1.0)[0].run()                                         # (first touch of the library)
    sim, wrappers = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    bulkheads, timeouts = wrappers[0::2], wrappers[1::2]
    print(json.dumps(dict(what="Source.poisson(40) -> Bulkhead(4, 3, 0.5) | TimeoutWrapper(0.08) -> NetworkLink(0.03 + Exp(0.02)) -> "
                               "Server(Exp(0.02)) -> Sink, the link paused for 1 s per group",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, resilience_events=[int(v) for v in sim._resilience_by_kind],
                          fault_events=int(sim._fault_events_processed), device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), wall_s=round(wall, 3),
                          bulkhead_rejected=sum(b.stats.rejected_requests for b in bulkheads),
                          bulkhead_timed_out=sum(b.stats.timed_out_requests for b in bulkheads),
                          active_at_the_end=sum(b.active_count for b in bulkheads), bulkheads_without_a_permit=sum(b.available_permits == 0 for b in bulkheads),
                          timeouts=sum(t.stats.timed_out_requests for t in timeouts),
                          successful=sum(t.stats.successful_requests for t in timeouts))), flush=True)


if __name__ == "__main__":
    main()
