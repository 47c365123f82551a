"""ON THE GPU BOX: the capacity experiment in ONE Simulation -- Source.poisson(40) -> LoadBalancer(LeastConnections) over one
Server(Exp(0.05)), scaled by an AutoScaler(TargetUtilization(0.6), 1 .. 4 instances, evaluated every 0.5 s, cooldowns of 1 s and 2 s)
-> Sink per group -- the single-heap loop's scaler instantiation (csrc/hs_graph.hip hs_graph_run_batch_level<kLvScaler>) with the data-parallel
dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps side by side).  Prints one JSON line: events/s of the
device and the device time; `wall_s` is Simulation.run() as a whole.  A demonstration: nothing else runs a scaler, so the loop's
~2.5 us per event and heap is the only figure it can be set against.

    python tools/autoscaler_profile.py [groups] [end_s]
    python tools/autoscaler_profile.py --replicas [n]      # the standing replica workload WITHOUT a scaler (tools/graph_replicas.py's
                                                           # graph x 60 s): device_ms of one hs_graph_run_many over n replicas, the
                                                           # figure that is set against the parent commit's
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import happy_simulator_amd as hs  # noqa: E402


def build(n, end_s):
    sources, entities, groups = [], [], []
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        server = hs.Server(f"srv{g}", service_time=hs.ExponentialLatency(0.05), downstream=sink)
        lb = hs.LoadBalancer(f"lb{g}", backends=[server], strategy=hs.LeastConnections())
        scaler = hs.AutoScaler(f"as{g}", lb, lambda name, sink=sink: hs.Server(name, service_time=hs.ExponentialLatency(0.05), downstream=sink),
                               hs.TargetUtilization(0.6), min_instances=1, max_instances=4, evaluation_interval=0.5, scale_out_cooldown=1.0,
                               scale_in_cooldown=2.0)
        sources.append(hs.Source.poisson(rate=40, target=lb, name=f"src{g}"))
        entities += [server, lb, sink, scaler]
        groups.append((scaler, lb, sink))
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7)
    for scaler, _lb, _sink in groups:
        sim.schedule(scaler.start())
    return sim, groups


def replicas(n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import graph_specs as GS
    import helpers as H

    spec = dict(H.Golden("graph_three_load_balancers").spec)
    spec["end_s"] = 60.0
    GS.build(spec)[0].run()                                        # (first touch of the library)
    sims = []

    def build_fn():
        sims.append(GS.build(spec)[0])
        return sims[-1]

    res = hs.ParallelRunner().run_replicas(build_fn, n, base_seed=7)
    print(json.dumps(dict(replicas=n, device_ms=round(sims[0]._engine_summary.last_run_ms, 3),
                          events=sum(r.summary.total_events_processed for r in res))), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--replicas":
        return replicas(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 1.0)[0].run()                                         # (first touch of the library)
    sim, groups = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    heaps = max(sim._graph_parts, 1)
    print(json.dumps(dict(what="Source.poisson(40) -> LoadBalancer(LeastConnections) over Server(Exp(0.05)), AutoScaler(TargetUtilization(0.6), 1 .. 4, "
                               "every 0.5 s, cooldowns 1 s / 2 s) -> Sink per group; a demonstration: nothing else runs a scaler, the loop's "
                               "~2.5 us per event and heap is the only figure to set it against",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), us_per_event_and_heap=round(dev_ms * 1e3 / (ev / heaps), 3),
                          wall_s=round(wall, 3), evaluations=sum(s.stats.evaluations for s, _l, _k in groups),
                          scale_outs=sum(s.stats.scale_out_count for s, _l, _k in groups), scale_ins=sum(s.stats.scale_in_count for s, _l, _k in groups),
                          instances_added=sum(s.stats.instances_added for s, _l, _k in groups),
                          cooldown_blocks=sum(s.stats.cooldown_blocks for s, _l, _k in groups),
                          pool_nodes=sum(len(s._pool) for s, _l, _k in groups), received=sum(k.events_received for _s, _l, k in groups))),
          flush=True)


if __name__ == "__main__":
    main()
