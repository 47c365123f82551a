#!/usr/bin/env python3
"""Device times of the WeightedRoundRobin / IPHash / LeastConnections strategies -> profiles/lb_strategies.json (DESIGN.md
sections 5 and 6 quote it).  HIP events on the engines' own streams, warm-up runs first, medians over repeats.

  pipeline     RoundRobin, WeightedRoundRobin (unit and skewed weights), ConsistentHash and IPHash at the benchmarked size
               (32 768 Sources -> 32 768 backends x 60 s): device ms per run (hs_lb_bench_runs).
  single_heap  one LeastConnections LoadBalancer over 8 .. 32 768 backends: device time per event with the selection on all 64
               lanes and on the lone lane (hs_debug_graph_flags) -- the crossover is csrc/hs_graph.hip kCoopMinBackends.
  loop         a graph WITHOUT a least-loaded strategy (RoundRobin over 8 backends): the time per event of the restructured loop.

  regression   the restructured loop against the parent commit on the same device: `--loop-only --tree <checkout of the parent,
               built>` measures the `loop` graph with that checkout's package (it needs nothing this change added) and
               `--merge` folds such results and bench.py lines (`--full`: other_workloads.graph_replicas / graph_parts;
               `--workload lb`) of both builds into the JSON.

    python tools/lb_strategies_profile.py [--out profiles/lb_strategies.json] [--quick]
    python tools/lb_strategies_profile.py --loop-only [--tree DIR] --out loop.json
    python tools/lb_strategies_profile.py --merge KEY=FILE ... --out profiles/lb_strategies.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if "--tree" in sys.argv:                               # the package of another checkout (the parent commit's) instead of this one
    sys.path[0] = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])

import happy_simulator_amd as hs  # noqa: E402
from happy_simulator_amd import _native as N  # noqa: E402
from happy_simulator_amd.graph_engine import GraphEngine, lower_general  # noqa: E402
from happy_simulator_amd.lb_engine import LbBackendArrays, LbSourceArrays, LoadBalancerEngine  # noqa: E402


def pipeline(strategy, weights, S, B, end_s, warmup, steps):
    end_ns = int(end_s * 1e9)
    keyed = strategy in (N.LB_CONSISTENT_HASH, N.LB_IP_HASH)
    src = LbSourceArrays(n=S, src_rate=np.full(S, 6.0), n_clients=np.full(S, (1 << 20) if keyed else 1, np.int64),
                         src_kind=np.full(S, N.SRC_POISSON, np.uint8))
    be = LbBackendArrays(n=B, names=[f"srv{j}" for j in range(B)], concurrency=np.full(B, 1, np.int32),
                         svc_kind=np.full(B, N.LAT_EXPONENTIAL, np.uint8), svc_mean_s=np.full(B, 0.1))
    with LoadBalancerEngine(src, be, virtual_nodes=150, horizon_ns=end_ns, shared_sink=True, seed=42, strategy=strategy) as eng:
        if weights is not None:
            eng.set_weights(weights)
        eng.bench_runs(end_ns, warmup)
        run_ms, sort_ms = eng.bench_runs(end_ns, steps)
        s = eng.summary()
        return dict(device_ms=float(np.median(run_ms)), device_ms_min=float(run_ms.min()), device_ms_max=float(run_ms.max()),
                    sort_ms=float(np.median(sort_ms)), events=int(s.events_processed), launches=int(s.launches),
                    max_backend_requests=int(eng.stats()["total_requests"].max()))


def graph_arrays(strategy, B, requests, end_s):
    sink = hs.Sink("k")
    servers = [hs.Server(f"srv{j}", concurrency=2, service_time=hs.ExponentialLatency(0.5), downstream=sink) for j in range(B)]
    lb = hs.LoadBalancer("lb", backends=servers, strategy=strategy)
    srcs = [hs.Source.poisson(rate=requests / end_s / 4, target=lb, name=f"s{i}") for i in range(4)]
    return lower_general(srcs, [lb, *servers, sink]).arrays


def single_heap(arrays, flags, end_s, repeats):
    end_ns = int(end_s * 1e9)
    out = []
    for r in range(repeats + 1):                       # (the first run warms the device up: not counted)
        with GraphEngine(arrays, seed=42) as eng:
            if flags:
                eng.set_debug_flags(flags)
            eng.run_until(end_ns)
            s = eng.summary()
            if r:
                out.append((s.last_run_ms, int(s.events_processed), int(s.events_by_kind[11]), eng.coop_selects() if flags else 0,
                            int(s.launches)))
    ms = statistics.median(o[0] for o in out)
    _, events, selections, coop, launches = out[0]
    return dict(device_ms=ms, events=events, selections=selections, cooperative_selections=coop, launches=launches,
                us_per_event=1e3 * ms / events)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lb_strategies.json"))
    ap.add_argument("--quick", action="store_true", help="a small pipeline and few repeats (a functional check of this script)")
    ap.add_argument("--loop-only", action="store_true", help="only the graph without a least-loaded strategy")
    ap.add_argument("--tree", default=None, help="import the package of this checkout (see the module docstring)")
    ap.add_argument("--merge", nargs="*", default=None, metavar="KEY=FILE",
                    help="fold JSON files (a --loop-only result, or the last line of a bench.py log) into --out under regression.KEY")
    args = ap.parse_args()
    if args.merge is not None:
        with open(args.out) as f:
            res = json.load(f)
        reg = res.setdefault("regression", {})
        for item in args.merge:
            key, path = item.split("=", 1)
            with open(path) as f:
                d = json.loads(f.read().strip().splitlines()[-1])
            if "loop" in d:
                reg[key] = d["loop"]
            else:
                ow = d.get("config", {}).get("other_workloads", {})
                reg[key] = {"ms_per_step": d.get("ms_per_step"), "value": d.get("value"),
                            "device_ms_per_step": d.get("config", {}).get("device_ms_per_step"),
                            **{k: {q: ow[k][q] for q in ("device_ms", "events", "events_per_s_device") if q in ow[k]}
                               for k in ("graph_replicas", "graph_parts") if k in ow}}
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if args.loop_only:
        res = dict(loop=dict(round_robin_8=single_heap(graph_arrays(hs.RoundRobin(), 8, 20000, 4.0), 0, 4.0, 5)))
        print(res, flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f)
            f.write("\n")
        return
    S = B = 2048 if args.quick else 32768
    end_s, warmup, steps = (5.0, 1, 2) if args.quick else (60.0, 3, 10)
    res = dict(device=N.lib().hs_device_count(), pipeline={}, single_heap={}, loop={})
    skew = (1 + 3 * (np.arange(B) % 4 == 0)).astype(np.int32)
    heavy = np.ones(B, np.int32)                       # one backend with 64 mean shares: beyond the [k][backend] rows (dense layout)
    heavy[B // 3] = 64
    for name, strategy, weights in (("round_robin", N.LB_ROUND_ROBIN, None), ("weighted_round_robin_unit", N.LB_WEIGHTED_ROUND_ROBIN, np.ones(B, np.int32)),
                                    ("weighted_round_robin_skewed", N.LB_WEIGHTED_ROUND_ROBIN, skew),
                                    ("weighted_round_robin_one_heavy", N.LB_WEIGHTED_ROUND_ROBIN, heavy), ("consistent_hash", N.LB_CONSISTENT_HASH, None),
                                    ("ip_hash", N.LB_IP_HASH, None)):
        res["pipeline"][name] = pipeline(strategy, weights, S, B, end_s, warmup, steps)
        print(name, res["pipeline"][name], flush=True)
    res["pipeline"]["config"] = dict(sources=S, backends=B, rate=6.0, mean=0.1, end_s=end_s, warmup=warmup, steps=steps)
    repeats = 1 if args.quick else 3
    for nb in (8, 16, 32, 64, 512, 4096, 32768):
        requests = 4000 if nb <= 4096 else 200             # (the lone lane needs ~B loads per selection)
        arrays = graph_arrays(hs.LeastConnections(), nb, requests, 2.0)
        row = dict(cooperative=single_heap(arrays, N.GRAPH_DEBUG_COOPERATIVE, 2.0, repeats),
                   lane_serial=single_heap(arrays, N.GRAPH_DEBUG_LANE_SERIAL, 2.0, repeats))
        sel = row["cooperative"]["selections"]
        row["us_per_selection_saved"] = 1e3 * (row["lane_serial"]["device_ms"] - row["cooperative"]["device_ms"]) / sel
        res["single_heap"][str(nb)] = row
        print(nb, row, flush=True)
    res["loop"]["round_robin_8"] = single_heap(graph_arrays(hs.RoundRobin(), 8, 20000, 4.0), 0, 4.0, repeats)
    print(res["loop"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
