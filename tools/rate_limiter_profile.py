"""ON THE GPU BOX: 65 536 disconnected Source -> RateLimitedEntity -> Server -> Sink chains in ONE Simulation, 10 s -- the
single-heap loop's limiter handlers (csrc/hs_graph.hip kEvLimRequest / kEvLimPoll) with the data-parallel dimension a Simulation has:
its parts (hs_graph_run_parts, up to 2 048 heaps side by side).  Prints one JSON line: device time, events and events/s.
`wall_s` is Simulation.run() as a whole: lowering, splitting into parts, the launch, and reading back every limiter's state (one
copy of the nodes' state and of the sliding-window rings per part, then host calls); `device_ms` is the launch alone.

    python tools/rate_limiter_profile.py [chains] [end_s]
"""
import json
import sys
import time

import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    policies = (lambda: hs.TokenBucketPolicy(3, 5.0), lambda: hs.LeakyBucketPolicy(4.0), lambda: hs.SlidingWindowPolicy(0.5, 3),
                lambda: hs.FixedWindowPolicy(3, 0.5))
    sources, entities, limiters = [], [], []
    for i in range(n):
        sink = hs.Sink(f"sink{i}")
        srv = hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink)
        lim = hs.RateLimitedEntity(f"lim{i}", srv, policies[i % 4](), queue_capacity=4)
        sources.append(hs.Source.poisson(rate=10, target=lim, name=f"src{i}"))
        entities += [lim, srv, sink]
        limiters.append(lim)
    return hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7), limiters


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(64, 1.0)[0].run()                                        # (first touch of the library)
    sim, limiters = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    print(json.dumps(dict(what="Source.poisson(10) -> RateLimitedEntity(queue_capacity=4, the four policies in turn) -> Server(Exp(0.05)) -> Sink",
                          chains=n, end_s=end_s, parts=sim._graph_parts, events=ev, device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), wall_s=round(wall, 3),
                          received=sum(x.stats.received for x in limiters), forwarded=sum(x.stats.forwarded for x in limiters),
                          dropped=sum(x.stats.dropped for x in limiters))))


if __name__ == "__main__":
    main()
