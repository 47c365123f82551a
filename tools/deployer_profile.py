"""ON THE GPU BOX: rolling deployments in ONE Simulation -- Source.poisson(40) -> LoadBalancer(LeastConnections) over three
Server(Exp(0.05)), replaced by a RollingDeployer(batch_size=1, health_check_interval=0.5, healthy_threshold=2, max_failures=3) whose
deploy() is scheduled at 1 s -> Sink per group -- the single-heap loop's deployer instantiation (csrc/hs_graph.hip
hs_graph_run_batch_level<kLvDeploy>) with the data-parallel dimension a Simulation has: its parts (hs_graph_run_parts, up to 2 048 heaps side by
side).  Prints one JSON line: events/s of the device and the device time; `wall_s` is Simulation.run() as a whole.  A demonstration:
nothing else runs a deployer, so the loop's ~2.5 us per event and heap is the only figure it can be set against.

    python tools/deployer_profile.py [groups] [end_s]
    python tools/deployer_profile.py --replicas [n]       # the standing replica workload WITHOUT a deployer (tools/graph_replicas.py's
                                                          # graph x 60 s): device_ms of one hs_graph_run_many over n replicas, the
                                                          # figure that is set against the parent commit's
    python tools/deployer_profile.py --verdict new.jsonl parent.jsonl out.json
                                                          # five `--replicas` lines of this build and of the parent commit, run in
                                                          # turns on one device: the new median may exceed the parent's by no more than
                                                          # the parent's own max - min
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(n, end_s):
    import happy_simulator_amd as hs

    sources, entities, groups = [], [], []
    for g in range(n):
        sink = hs.Sink(f"sink{g}")
        servers = [hs.Server(f"srv{g}_{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink) for i in range(3)]
        lb = hs.LoadBalancer(f"lb{g}", backends=servers, strategy=hs.LeastConnections())
        deployer = hs.RollingDeployer(f"rd{g}", lb, lambda name, sink=sink: hs.Server(name, service_time=hs.ExponentialLatency(0.05), downstream=sink),
                                      batch_size=1, health_check_interval=0.5, healthy_threshold=2, max_failures=3)
        sources.append(hs.Source.poisson(rate=40, target=lb, name=f"src{g}"))
        entities += servers + [lb, sink, deployer]
        groups.append((deployer, lb, sink))
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=sources, entities=entities, seed=7)
    for deployer, _lb, _sink in groups:
        ev = deployer.deploy()
        ev.time = hs.Instant.from_seconds(1.0)
        sim.schedule(ev)
    return sim, groups


def replicas(n):
    import happy_simulator_amd as hs

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


def verdict(new_path, parent_path, out_path):
    read = lambda path: [json.loads(line) for line in open(path) if line.strip().startswith("{")]  # noqa: E731
    new, parent = read(new_path), read(parent_path)
    assert len(new) == len(parent) == 5 and len({r["events"] for r in new + parent}) == 1, (new, parent)
    a, b = [r["device_ms"] for r in new], [r["device_ms"] for r in parent]
    spread = round(max(b) - min(b), 3)
    out = dict(what="1 024 replicas of tools/graph_replicas.py's graph x 60 s WITHOUT a deployer, hs_graph_run_many device time; five runs of "
                    "this build and of the parent commit in turns on one MI355X",
               replicas=new[0]["replicas"], events=new[0]["events"], new_ms=a, parent_ms=b, new_median_ms=statistics.median(a),
               parent_median_ms=statistics.median(b), parent_max_minus_min_ms=spread,
               within_the_parents_spread=bool(statistics.median(a) <= statistics.median(b) + spread))
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    return 0 if out["within_the_parents_spread"] else 1


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--verdict":
        return verdict(*sys.argv[2:5])
    if len(sys.argv) > 1 and sys.argv[1] == "--replicas":
        return replicas(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    build(8, 2.0)[0].run()                                         # (first touch of the library)
    sim, groups = build(n, end_s)
    t0 = time.monotonic()
    summary = sim.run()
    wall = time.monotonic() - t0
    dev_ms = sim._engine_summary.last_run_ms
    ev = summary.total_events_processed
    heaps = max(sim._graph_parts, 1)
    print(json.dumps(dict(what="Source.poisson(40) -> LoadBalancer(LeastConnections) over 3 x Server(Exp(0.05)), RollingDeployer(batch_size=1, "
                               "health_check_interval=0.5, healthy_threshold=2, max_failures=3), deploy() at 1 s -> Sink per group; a "
                               "demonstration: nothing else runs a deployer, the loop's ~2.5 us per event and heap is the only figure to set "
                               "it against",
                          groups=n, end_s=end_s, parts=sim._graph_parts, events=ev, device_ms=round(dev_ms, 3),
                          device_events_per_s=round(ev / (dev_ms / 1e3), 1), us_per_event_and_heap=round(dev_ms * 1e3 / (ev / heaps), 3),
                          wall_s=round(wall, 3), deployments_completed=sum(d.stats.deployments_completed for d, _l, _k in groups),
                          deployments_rolled_back=sum(d.stats.deployments_rolled_back for d, _l, _k in groups),
                          instances_replaced=sum(d.stats.instances_replaced for d, _l, _k in groups),
                          health_checks_performed=sum(d.stats.health_checks_performed for d, _l, _k in groups),
                          pool_nodes=sum(len(d._pool) for d, _l, _k in groups), received=sum(k.events_received for _d, _l, k in groups))),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
