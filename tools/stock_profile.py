"""ON THE GPU BOX: replicas of Source.poisson(40) -> InventoryBuffer(20, reorder at 5, 20 items, lead time 1/3 s, stock-outs to a Sink of
their own) -> PooledCycleResource(3 units, 0.05 s, a line of 8) -> Sink through ParallelRunner.run_replicas -- hs_graph_run_many, one
workgroup and one heap per replica -- on the single-heap loop's last level (csrc/hs_graph.hip kLvStock: kEvPcItem .. kEvIbReplenish).
Prints one JSON line: the events, the device time, events/s of the device and the microseconds per event and heap; `wall_s` is
run_replicas as a whole.  A demonstration of what the level costs as measured, not a bound.

    python tools/stock_profile.py [replicas] [end_s]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import happy_simulator_amd as hs  # noqa: E402


def build(end_s, made):
    sink, lost = hs.Sink("sink"), hs.Sink("stockouts")
    pool = hs.PooledCycleResource("pool", 3, 0.05, downstream=sink, queue_capacity=8)
    buffer = hs.InventoryBuffer("buffer", 20, 5, 20, 1.0 / 3.0, downstream=pool, stockout_target=lost)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(end_s), sources=[hs.Source.poisson(rate=40, target=buffer, name="src")],
                        entities=[buffer, pool, sink, lost], seed=7)
    made.append((sim, buffer, pool, sink))
    return sim


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    end_s = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    build(1.0, []).run()                                           # (first touch of the library)
    made = []
    t0 = time.monotonic()
    res = hs.ParallelRunner().run_replicas(lambda: build(end_s, made), n, base_seed=7)
    wall = time.monotonic() - t0
    dev_ms = made[0][0]._engine_summary.last_run_ms                # the batch's device time (hs_graph_run_many)
    ev = sum(r.summary.total_events_processed for r in res)
    print(json.dumps(dict(what="Source.poisson(40) -> InventoryBuffer(20, reorder_point 5, order_quantity 20, lead_time 1/3, stockout_target a Sink) -> "
                               "PooledCycleResource(3, 0.05, queue_capacity 8) -> Sink per replica; a demonstration, as measured",
                          replicas=n, end_s=end_s, events=ev, stock_events=[int(sum(s._stock_by_kind[k] for s, *_ in made)) for k in range(4)],
                          device_ms=round(dev_ms, 3), device_events_per_s=round(ev / (dev_ms / 1e3), 1),
                          us_per_event_and_heap=round(dev_ms * 1e3 / (ev / n), 3), wall_s=round(wall, 3),
                          consumed=sum(b.stats.items_consumed for _s, b, _p, _k in made), stockouts=sum(b.stats.stockouts for _s, b, _p, _k in made),
                          reorders=sum(b.stats.reorders for _s, b, _p, _k in made), completed=sum(p.completed for _s, _b, p, _k in made),
                          rejected=sum(p.rejected for _s, _b, p, _k in made), received=sum(k.events_received for _s, _b, _p, k in made))), flush=True)


if __name__ == "__main__":
    main()
