#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for BatchProcessor, ConveyorBelt and GateController
(components/industrial/batch_processor.py, conveyor.py, gate_controller.py) -- the yardstick of tests/test_flow_host.py and
tests/test_gpu_flow.py.  Run by hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_flow.py          # writes tests/golden/live_flow/part_*.npz

Recorded (tests/flow_specs.py FLOW reads them back):
  * constructor defaults, properties, stats objects and the ValueError texts of the three classes, start_events() and the host-side
    open() / close();
  * every spec of flow_specs.all_specs() and the two growth cases: the reference's own event loop over its own components, with the
    Philox stream plugs of make_golden.py choosing the random numbers -- everything the faults family records, plus per entity its
    statistics and what it still holds, and the Events processed of the eight new kinds (31 .. 38 in by_kind and in the trace: a
    Request at a BatchProcessor, its `_BatchTimeout`, the continuation of a batch; a Request at a ConveyorBelt, the continuation of
    its transit; a Request at a GateController, its `_GateOpen`, its `_GateClose`); the fixtures of flow_specs.TRACED with their
    full trace.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed): no case is left out.
Running it again rewrites the parts byte for byte.
"""
from __future__ import annotations

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import flow_specs as FL  # noqa: E402
from happysimulator import Sink  # noqa: E402

BatchProcessor, ConveyorBelt, GateController = RF.BatchProcessor, RF.ConveyorBelt, RF.GateController
EV, REF_NS = RF.EV, RF.REF_NS
CTOR_ERRORS = (("batch", dict(batch_size=0)), ("batch", dict(batch_size=-3)), ("batch", dict(process_time=-0.5)), ("batch", dict(batch_size=1, process_time=0)),
               ("batch", dict(timeout_s=-1.0)), ("conveyor", dict(transit_time=-0.1)), ("conveyor", dict(transit_time=0)),
               ("conveyor", dict(transit_time=1.0, capacity=-2)), ("gate", dict(queue_capacity=-1)), ("gate", dict(schedule=[])))


def ctor_error(ns, kind, kw):
    k = ns.Sink("k") if hasattr(ns, "Sink") else Sink("k")
    try:
        if kind == "batch":
            ns.BatchProcessor("x", k, **kw)
        elif kind == "conveyor":
            ns.ConveyorBelt("x", k, **kw)
        else:
            ns.GateController("x", k, **kw)
        return None
    except ValueError as e:
        return str(e)


def defaults(ns=REF_NS, sink=Sink):
    """Constructor state, properties, stats objects and error texts; start_events() and open() / close() on the host."""
    k = sink("k")
    b, c, g = ns.BatchProcessor("b", k), ns.ConveyorBelt("c", k, 0.5), ns.GateController("g", k)
    out = dict(batch=[b.batch_size, b.process_time, b.timeout_s, b.batches_processed, b.items_processed, b.timeouts, b.buffer_depth],
               conveyor=[c.transit_time, c.items_in_transit, c.items_transported, c.items_rejected, c.has_capacity()],
               gate=[list(g.schedule), g.is_open, g.queue_depth],
               downstream=[x.downstream is k and [d.name for d in x.downstream_entities()] for x in (b, c, g)],
               stats_types=[type(x.stats).__name__ for x in (b, c, g)],
               stats_fields=[list(type(x.stats).__dataclass_fields__) for x in (b, c, g)],
               stats=[[getattr(x.stats, f) for f in type(x.stats).__dataclass_fields__] for x in (b, c, g)])
    frozen = []
    for x in (b, c, g):
        try:
            setattr(x.stats, next(iter(type(x.stats).__dataclass_fields__)), 1)
            frozen.append(False)
        except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
            frozen.append(type(e).__name__)
    out["stats_frozen"] = frozen
    out["errors"] = [ctor_error(ns, kind, kw) for kind, kw in CTOR_ERRORS]
    g2 = ns.GateController("g2", k, schedule=[(1.0, 2.5), (3, 4)], initially_open=False, queue_capacity=2)
    evs = g2.start_events()
    out["start_events"] = [[e.time.nanoseconds, e.event_type, bool(e.daemon), e.target is g2] for e in evs]
    steps = []
    for what in ("open", "open", "close", "close", "open"):
        r = getattr(g2, what)()
        steps.append([what, r, g2.is_open, g2.stats.open_cycles, g2.queue_depth])
    out["host_open_close"] = steps
    out["conveyor_capacity"] = [ns.ConveyorBelt("c", k, 0.1, capacity=cap).has_capacity() for cap in (0, -1, 1)]
    return out


def run_case(spec, want_trace=False):
    """The reference's run of one spec: record_family.run_case as the family "flow", which holds no Event of a checker, a wrapper or a
    Client."""
    out = RF.run_case(spec, "flow", want_trace)
    assert out["by_kind"][EV["hc_cycle"]:EV["bp_item"]].sum() == 0
    return out


def main():
    cases = {FL.FLOW.key("defaults"): defaults()}
    for spec in FL.all_specs() + [make() for make in FL.GROWTH]:
        sim, _pools = FL.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_flows, spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[FL.FLOW.key("case", spec)] = run_case(spec, want_trace=spec["name"] in FL.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        print(spec["name"], res["total_events"], res["by_kind"][EV["bp_item"]:].tolist(), res["flow_stats"].tolist(), res["events_cancelled"],
              res["crashed"].sum(), flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[FL.FLOW.key("case", FL.FIXTURES[name])]  # noqa: E731
    r = get("gate_conveyor_processor_chain")
    assert r["flow_stats"][0, :5].tolist() == [25, 15, 20, 2, 0], r["flow_stats"]          # GateStats(25, 15, 20, 2, False)
    assert r["flow_stats"][1, :3].tolist() == [15, 0, 10], r["flow_stats"]                # ConveyorStats(15, 0, 10)
    assert r["flow_stats"][2, :3].tolist() == [6, 15, 6], r["flow_stats"]                 # BatchProcessorStats(6, 15, 6)
    assert r["total_events"] == 274 and r["received"][0] == 15, (r["total_events"], r["received"])
    r = get("batch_size_one_with_timeout")                  # the four items of a constant Source of rate 4 that stops after 1 s, over 3 s
    assert r["flow_stats"][0, :3].tolist() == [2, 4, 0] and r["events_cancelled"] == 2 and r["total_events"] == 23, (r["flow_stats"], r["events_cancelled"], r["total_events"])
    r = get("gate_flushes_five_into_a_conveyor_at_capacity")
    assert r["flow_stats"][1, 2] >= 3, r["flow_stats"]
    r = get("two_batches_in_process")
    assert r["by_kind"][EV["bp_cont"]] >= 2
    assert get("processor_paused_timeout_dropped")["crashed"].sum() == 0
    assert len(FL.FIXTURES) >= 30 and len(FL.TRACED) >= 6 and FL.N_RANDOM >= 100
    FL.FLOW.write(cases)


if __name__ == "__main__":
    main()
