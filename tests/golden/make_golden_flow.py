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

import types

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import flow_specs as FL  # noqa: E402
import graph_family as GF  # noqa: E402
import fault_specs as FS  # noqa: E402
import make_golden as MG  # noqa: E402
import happysimulator.components.industrial.batch_processor as ref_bp  # noqa: E402
import happysimulator.components.industrial.conveyor as ref_cv  # noqa: E402
import happysimulator.components.industrial.gate_controller as ref_gt  # noqa: E402
from happysimulator import Instant, Simulation, Sink, Source  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from happysimulator.components.server.server import Server  # noqa: E402
from happysimulator.core.event import Event, ProcessContinuation  # noqa: E402
from happysimulator.load.profile import ConstantRateProfile  # noqa: E402
from happysimulator.load.providers.constant_arrival import ConstantArrivalTimeProvider  # noqa: E402
from happysimulator.load.source import SimpleEventProvider  # noqa: E402

BatchProcessor, ConveyorBelt, GateController = ref_bp.BatchProcessor, ref_cv.ConveyorBelt, ref_gt.GateController
EV = dict(RF.EV)
for _name in FL.EV_FLOW:
    EV[_name] = len(EV)
assert EV["bp_item"] == FL.EV_FLOW_FIRST and len(EV) == 39
REF_NS = types.SimpleNamespace(**vars(RF.REF_NS), BatchProcessor=BatchProcessor, ConveyorBelt=ConveyorBelt, GateController=GateController)
REF_METRIC = dict(RF.REF_METRIC, buffer_depth="buffer_depth", items_in_transit="items_in_transit")
SECTIONS = ("time_travel", "stats", "probes", "limiters", "faults", "flows", "fault_events", "cancelled")
CTOR_ERRORS = (("batch", dict(batch_size=0)), ("batch", dict(batch_size=-3)), ("batch", dict(process_time=-0.5)), ("batch", dict(batch_size=1, process_time=0)),
               ("batch", dict(timeout_s=-1.0)), ("conveyor", dict(transit_time=-0.1)), ("conveyor", dict(transit_time=0)),
               ("conveyor", dict(transit_time=1.0, capacity=-2)), ("gate", dict(queue_capacity=-1)), ("gate", dict(schedule=[])))


class _Reference(RF._Reference):
    """record_family's factory; a Source may stop handing out Requests (`stop_s`), a Probe may read the three new metrics."""

    def source(self, k, sc, to):
        if sc.get("stop_s") is None:
            return super().source(k, sc, to)
        assert sc["kind"] == "constant"
        prov = ConstantArrivalTimeProvider(ConstantRateProfile(rate=sc["rate"]), start_time=Instant.Epoch)
        return Source(f"src{k}", SimpleEventProvider(to, "Request", MG._at(self.spec, sc["stop_s"])), prov)

    def probe(self, target, metric, interval):
        probe, data = RF.recording_probe(target, REF_METRIC[metric], interval)
        self.probe_data.append(data)
        return probe


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


def classify(e, node_of, by_name):
    """(kind, node) of a popped Event: the three entities' own kinds, else record_family's."""
    t = e.target
    if isinstance(t, BatchProcessor):
        return (EV["bp_cont"] if isinstance(e, ProcessContinuation) else EV["bp_timeout"] if e.event_type == "_BatchTimeout" else EV["bp_item"]), node_of[id(t)]
    if isinstance(t, ConveyorBelt):
        return (EV["cv_cont"] if isinstance(e, ProcessContinuation) else EV["cv_item"]), node_of[id(t)]
    if isinstance(t, GateController):
        return (EV["gt_open"] if e.event_type == "_GateOpen" else EV["gt_close"] if e.event_type == "_GateClose" else EV["gt_item"]), node_of[id(t)]
    return RF.classify(e, node_of, by_name)


_SECTION = dict(RF._SECTION, faults=lambda c: FS.fault_results(c.fs, FL.fault_targets(c.pools)), flows=lambda c: FL.flow_results(c.pools))


def run_case(spec, want_trace=False):
    """The reference's run of one spec (record_family.run_case with this family's wiring, kinds and sections)."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    c = types.SimpleNamespace(spec=spec, F=_Reference(spec), skipped=0, probe_drops=0)
    c.pools, c.sources, probes, entities = FL.wire(spec, c.F, REF_NS)
    c.fs, handles = GF.make_schedule(REF_NS, spec, c.pools)
    sim = Simulation(start_time=MG._start(spec), sources=c.sources, entities=entities, fault_schedule=c.fs,
                     **({} if spec.get("auto") else {"end_time": MG._at(spec, spec["end_s"])}), **({"probes": probes} if probes else {}))
    GF.cancel_after(spec, handles)
    node_of = {}
    for i, x in enumerate(c.sources + probes):
        node_of[id(x)] = i
    first = len(c.sources) + len(probes)
    lim_index = {}
    for i, x in enumerate(entities):
        node_of[id(x)] = first + i
        if isinstance(x, Server):
            for part in (x._queue, x._driver, x._worker):
                node_of[id(part)] = first + i
        if isinstance(x, RateLimitedEntity):
            lim_index[id(x)] = len(lim_index)
    by_name = {x.name: node_of[id(x)] for x in entities + c.sources + probes}
    cb_probe = {id(p._event_provider.data_sink): len(c.sources) + j for j, p in enumerate(probes)}
    c.by_kind = by_kind = np.zeros(len(EV), np.int64)
    c.lim_events = np.zeros((len(lim_index), 2), np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop
    state = dict(cur=sim._start_time, cancelled=0)

    def pop():
        e = orig_pop()
        assert by_kind.sum() < RF.MAX_EVENTS, spec["name"]
        if e.cancelled:                                   # skipped, counted in events_cancelled (core/simulation.py:326-329)
            state["cancelled"] += 1
            return e
        if e.time < state["cur"]:                         # time travel: skipped, not counted
            c.skipped += 1
            return e
        state["cur"] = e.time
        k, nd = classify(e, node_of, by_name)
        live = not getattr(e.target, "_crashed", False)
        if isinstance(e.target, RateLimitedEntity) and live:
            c.lim_events[lim_index[id(e.target)], k - EV["lim_request"]] += 1
        if k == EV["probe"]:
            fn = e.target._fn if hasattr(e.target, "_fn") else e.target.fn
            cells = {id(cell.cell_contents) for cell in (fn.__closure__ or ())}
            nd = next(node for key, node in cb_probe.items() if key in cells)
        by_kind[k] += 1
        if want_trace:
            trace.append((e.time.nanoseconds, k, nd, e._sort_index))
        return e

    heap.pop = pop
    FL.schedule_all(spec, c.pools, sim, Event, lambda t_s: MG._at(spec, t_s))
    c.summary = MG.run_sim_windows(sim, spec)
    out = dict(total_events=int(c.summary.total_events_processed), final_ns=int(sim._current_time.nanoseconds), by_kind=by_kind)
    assert int(by_kind.sum()) == out["total_events"], (spec["name"], int(by_kind.sum()), out["total_events"])
    assert state["cancelled"] == int(sim._events_cancelled)
    assert by_kind[EV["hc_cycle"]:EV["bp_item"]].sum() == 0
    out["pending_events"] = int(heap.size())
    for name in SECTIONS:
        out.update(_SECTION[name](c))
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
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
