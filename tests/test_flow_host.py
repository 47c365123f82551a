"""Host side of BatchProcessor, ConveyorBelt and GateController (no GPU): the mirrors against the recorded live reference
(tests/golden/live_flow/), what the lowering hands to the single-heap loop, the named refusals, and family_checks.compare on one of
this family's recordings."""
import copy
import os
import re
import subprocess

import ctypes as C
import numpy as np
import pytest

import family_checks as FC
import flow_specs as FL
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, flow_delay_ns, split_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = FL.FLOW
# (the grid of tests/golden/make_golden_flow.py, which needs the reference to be imported: repeated here)
CTOR_ERRORS = (("batch", dict(batch_size=0)), ("batch", dict(batch_size=-3)), ("batch", dict(process_time=-0.5)), ("batch", dict(batch_size=1, process_time=0)),
               ("batch", dict(timeout_s=-1.0)), ("conveyor", dict(transit_time=-0.1)), ("conveyor", dict(transit_time=0)),
               ("conveyor", dict(transit_time=1.0, capacity=-2)), ("gate", dict(queue_capacity=-1)), ("gate", dict(schedule=[])))
UT = hs.UnsupportedTopology


def _product_defaults():
    """tests/golden/make_golden_flow.py `defaults()` over the product's classes (that module imports the reference: its few lines
    are repeated here)."""
    k = hs.Sink("k")
    b, c, g = hs.BatchProcessor("b", k), hs.ConveyorBelt("c", k, 0.5), hs.GateController("g", k)
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
    errors = []
    for kind, kw in CTOR_ERRORS:
        try:
            (hs.BatchProcessor("x", k, **kw) if kind == "batch" else hs.ConveyorBelt("x", k, **kw) if kind == "conveyor" else hs.GateController("x", k, **kw))
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["errors"] = errors
    g2 = hs.GateController("g2", k, schedule=[(1.0, 2.5), (3, 4)], initially_open=False, queue_capacity=2)
    out["start_events"] = [[e.time.nanoseconds, e.event_type, bool(e.daemon), e.target is g2] for e in g2.start_events()]
    steps = []
    for what in ("open", "open", "close", "close", "open"):
        r = getattr(g2, what)()
        steps.append([what, r, g2.is_open, g2.stats.open_cycles, g2.queue_depth])
    out["host_open_close"] = steps
    out["conveyor_capacity"] = [hs.ConveyorBelt("c", k, 0.1, capacity=cap).has_capacity() for cap in (0, -1, 1)]
    return out


def test_mirrors_equal_the_recorded_defaults_and_errors():
    ref = FR.get("defaults")
    got = _product_defaults()
    assert set(got) == set(ref)
    for key in ref:
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert ref["errors"][:3] == ["batch_size must be > 0, got 0", "batch_size must be > 0, got -3", "process_time must be >= 0, got -0.5"]
    assert ref["errors"][5] == "transit_time must be >= 0, got -0.1" and ref["errors"][3:5] == [None, None] and ref["errors"][6:] == [None] * 4
    assert ref["stats_types"] == ["BatchProcessorStats", "ConveyorStats", "GateStats"] and ref["stats_frozen"] == ["FrozenInstanceError"] * 3
    assert hs.GateStats() == hs.GateStats(0, 0, 0, 0, True) and hs.BatchProcessorStats() == hs.BatchProcessorStats(0, 0, 0) and hs.ConveyorStats(1, 2, 3).items_rejected == 3


def test_what_the_issue_says_holds_in_the_recordings():
    get = lambda name: FR.get("case", FL.FIXTURES[name])  # noqa: E731
    r = get("gate_conveyor_processor_chain")
    assert r["flow_stats"].tolist() == [[25, 15, 20, 2, 0, 5], [15, 0, 10, 1, 0, 0], [6, 15, 6, 0, 0, 0]]
    assert r["total_events"] == 274 and r["received"].tolist() == [15] and len(r["by_kind"]) == 39
    r = get("batch_size_one_with_timeout")
    assert r["flow_stats"][0].tolist() == [2, 4, 0, 0, 0, 0] and r["events_cancelled"] == 2 and r["total_events"] == 23
    r = get("gate_flushes_five_into_a_conveyor_at_capacity")          # 5 on one nanosecond into a capacity of 2
    open_t = r["trace"][r["trace"][:, 1] == FL.EV_FLOW_FIRST + 6][0, 0]
    assert int(((r["trace"][:, 1] == FL.EV_FLOW_FIRST + 3) & (r["trace"][:, 0] == open_t)).sum()) == 5 and r["flow_stats"][1, 2] == 5
    r = get("gate_paused_open_event_dropped")
    assert r["flow_stats"][0, 3] == 1 and r["by_kind"][FL.EV_FLOW_FIRST + 6] == 2          # two `_GateOpen` popped, one handled
    r = get("processor_paused_timeout_dropped")
    assert r["by_kind"][FL.EV_FLOW_FIRST + 1] > r["flow_stats"][0, 2]                        # a timeout popped at the paused processor flushed nothing
    for make in FL.GROWTH:
        assert FR.get("case", make())["total_events"] > 2000


def test_the_lowering_accepts_every_spec_with_the_new_node_kinds():
    """Every recorded spec is one the product takes; one of the three sends the Simulation to the single-heap loop whatever its shape."""
    kinds = {"batch": N.NODE_BATCH_PROCESSOR, "conveyor": N.NODE_CONVEYOR, "gate": N.NODE_GATE}
    names = [s["name"] for s in FL.all_specs()]
    assert len(names) == len(set(names)) == len(FL.FIXTURES) + FL.N_RANDOM and FL.N_RANDOM >= 100 and len(FL.FIXTURES) >= 30
    for spec in FL.all_specs() + [make() for make in FL.GROWTH]:
        assert FR.get("case", spec)["total_events"] <= 40_000              # (recorded: no case is left out)
        sim, pools = FL.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph) and g.arrays.has_flows and "BatchProcessor, ConveyorBelt or GateController" in sim._station_refusal
        for fl, ent in zip(spec["flows"], pools["flow"]):
            assert g.arrays.kind[g.node_of[id(ent)]] == kinds[fl["kind"]]
        _end, _start, sched, _c = sim._general_prepare(g, bool(spec.get("auto")))
        n_gate = sum(2 * len(spec["flows"][on[1]]["sched"]) for on, _t, *mode in spec.get("schedule") or [] if mode)
        assert sum(1 for e in sched if len(e) == 4) == n_gate


def test_the_lowered_arrays_of_the_issues_chain():
    spec = FL.FIXTURES["gate_conveyor_processor_chain"]           # src0 | srv0, sink0, flow0 (gate), flow1 (conveyor), flow2 (processor)
    sim, pools = FL.build(spec)
    g = sim.lowered()
    a = g.arrays
    assert a.kind.tolist() == [N.NODE_SOURCE, N.NODE_SERVER, N.NODE_SINK, N.NODE_GATE, N.NODE_CONVEYOR, N.NODE_BATCH_PROCESSOR]
    assert a.target.tolist() == [3, 2, -1, 4, 5, 1]
    assert a.flow_params[3].tolist() == [5, 0, 0, 0] and a.flow_params[4].tolist() == [2, 200_000_000, 0, 0]
    assert a.flow_params[5].tolist() == [4, 50_000_000, 300_000_000, 0]
    _end, _start, sched, _c = sim._general_prepare(g, False)
    assert sched == [(3, 10 ** 9, None, True), (3, 2 * 10 ** 9, None, False), (3, 3 * 10 ** 9, None, True), (3, 3_500_000_000, None, False)]
    # whole nanoseconds as `Instant + seconds` makes them (core/temporal.py): int(seconds * 1e9), truncated
    assert flow_delay_ns(0.3, "x", "t") == int(0.3 * 1_000_000_000) == 300_000_000 and flow_delay_ns(4.188, "x", "t") == 4_187_999_999
    assert flow_delay_ns(2, "x", "t") == 2 * 10 ** 9
    for bad in (float("nan"), float("inf"), 1e30):
        with pytest.raises(UT, match="process_time"):
            hs.Simulation(sources=[], entities=[hs.BatchProcessor("b", hs.Sink("k"), process_time=bad)], end_time=hs.Instant.from_seconds(1)).lowered()


def test_host_open_and_close_set_the_state_the_run_starts_from():
    k = hs.Sink("k")
    g = hs.GateController("g", k, initially_open=False)
    assert g.open() == [] and g.open() == [] and g.close() == [] and g.open() == []
    a = hs.Simulation(sources=[], entities=[g, k], end_time=hs.Instant.from_seconds(1)).lowered().arrays
    assert a.flow_params[0].tolist() == [0, 0, 2, 1]             # unbounded, open_cycles = 2 so far, open


def _sim(entities, sources=(), **kw):
    return hs.Simulation(sources=list(sources), entities=list(entities), end_time=hs.Instant.from_seconds(1), **kw)


def test_the_refusals_by_name():
    k = hs.Sink("k")
    srv = hs.Server("s", service_time=hs.ExponentialLatency(0.05), downstream=k)
    three = lambda to: (hs.BatchProcessor("b", to), hs.ConveyorBelt("c", to, 0.1), hs.GateController("g", to))  # noqa: E731
    # a LoadBalancer backend
    for ent in three(k):
        lb = hs.LoadBalancer("lb", backends=[srv, ent], strategy=hs.RoundRobin())
        with pytest.raises(UT, match=rf"backend '{ent.name}' of 'lb' is a {type(ent).__name__}: only Server backends are lowered"):
            _sim([lb, srv, ent, k]).lowered()
    # the target of a Bulkhead, a TimeoutWrapper or a Client, directly or through NetworkLinks
    for ent in three(k):
        link = hs.NetworkLink("l", latency=hs.ConstantLatency(0.01), egress=ent)
        for to, via in ((ent, ""), (link, r" \(through its NetworkLinks\)")):
            for wrap in (hs.Bulkhead("w", to, max_concurrent=2), hs.TimeoutWrapper("w", to, timeout=0.5), hs.Client("w", to, timeout=0.5)):
                with pytest.raises(UT, match=rf"{type(wrap).__name__} 'w': its target{via} is the {type(ent).__name__} '{ent.name}' -- a completion hook "
                                             "on an item that a BatchProcessor, ConveyorBelt or GateController holds is not lowered"):
                    _sim([wrap, link, ent, k]).lowered()
    # a ParallelSimulation partition
    for ent in three(k):
        part = hs.SimulationPartition("p0", entities=[ent, k], sources=[hs.Source.poisson(rate=5, target=ent, name="src")])
        with pytest.raises(UT, match=rf"partition 'p0': the {type(ent).__name__} '{ent.name}' on a ParallelSimulation partition is not lowered"):
            hs.ParallelSimulation([part], end_time=hs.Instant.from_seconds(1))
    # the bounds, named as constants
    assert hs.BatchProcessor.MAX_BATCH_SIZE == hs.GateController.MAX_QUEUE_CAPACITY == N.FLOW_MAX_ITEMS == 1 << 20
    _sim([hs.BatchProcessor("b", k, batch_size=1 << 20), k]).lowered()
    with pytest.raises(UT, match=r"batch_size = 1048577 is beyond the 1048576 items of one batch on the engine \(BatchProcessor.MAX_BATCH_SIZE\)"):
        _sim([hs.BatchProcessor("b", k, batch_size=(1 << 20) + 1), k]).lowered()
    _sim([hs.GateController("g", k, queue_capacity=1 << 20), k]).lowered()
    with pytest.raises(UT, match=r"queue_capacity = 1048577 is beyond the 1048576 items of a bounded queue on the engine \(GateController.MAX_QUEUE_CAPACITY"):
        _sim([hs.GateController("g", k, queue_capacity=(1 << 20) + 1), k]).lowered()
    with pytest.raises(UT, match="batch_size must be an int"):
        _sim([hs.BatchProcessor("b", k, batch_size=2.5), k]).lowered()
    # a downstream that takes no Requests
    with pytest.raises(UT, match="takes no Requests|is not lowered"):
        _sim([hs.ConveyorBelt("c", None, 0.1)]).lowered()


def test_scheduled_events_the_three_take_and_refuse():
    k = hs.Sink("k")
    g, b = hs.GateController("g", k, schedule=[(0.2, 0.4)]), hs.BatchProcessor("b", k, timeout_s=0.5)
    sim = _sim([g, b, k])
    for ev in g.start_events():
        sim.schedule(ev)
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(0.3), event_type="Request", target=g))
    graph = sim.lowered()
    _end, _start, sched, _c = sim._general_prepare(graph, False)
    assert sched == [(0, 200_000_000, None, True), (0, 400_000_000, None, False), (0, 300_000_000)]
    sim = _sim([g, b, k])
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(0.3), event_type="_GateOpen", target=g))          # not a daemon: not start_events()'s
    with pytest.raises(UT, match="only the daemon Events start_events\\(\\) returns are lowered for a GateController"):
        sim._general_prepare(sim.lowered(), False)
    sim = _sim([g, b, k])
    sim.schedule(hs.Event(time=hs.Instant.from_seconds(0.3), event_type="_BatchTimeout", target=b))
    with pytest.raises(UT, match="a BatchProcessor's own '_BatchTimeout' Event is not lowered"):
        sim._general_prepare(sim.lowered(), False)


def test_gate_events_under_an_infinite_end_are_daemons_and_keep_one_heap():
    """The reference's gate Events are daemons: an auto-terminating run ends once only they are pending (recorded:
    auto_terminating_run stops with the second interval's two Events still in the heap)."""
    spec = FL.FIXTURES["auto_terminating_run"]
    ref = FR.get("case", spec)
    assert ref["pending_events"] == 2 and ref["by_kind"][FL.EV_FLOW_FIRST + 6:].tolist() == [1, 1] and ref["final_ns"] < 3 * 10 ** 9
    sim, _pools = FL.build(spec)
    end_ns, _start, sched, _c = sim._general_prepare(sim.lowered(), True)
    assert end_ns == 1 << 61 and sum(1 for e in sched if len(e) == 4) == 4


def test_probe_metrics_belong_to_their_entity():
    k = hs.Sink("k")
    b, c, g = hs.BatchProcessor("b", k), hs.ConveyorBelt("c", k, 0.1), hs.GateController("g", k)
    for ent, metric in ((b, "buffer_depth"), (c, "items_in_transit"), (g, "queue_depth")):
        probe, _data = hs.Probe.on(ent, metric, interval=0.5)
        a = _sim([b, c, g, k], probes=[probe]).lowered().arrays
        assert a.kind[0] == N.NODE_PROBE and a.probe_metric[0] == N.PROBE_FLOW_METRICS[metric]
    for ent, metric in ((c, "buffer_depth"), (g, "items_in_transit"), (b, "queue_depth"), (k, "queue_depth")):
        with pytest.raises(NotImplementedError, match="probe metric"):
            hs.Probe.on(ent, metric, interval=0.5)


def test_parts_keep_a_group_together_and_leave_the_rest_without():
    spec = FL.groups_spec(4)
    spec["servers"].append(FL.srv(0.05, out=None))
    spec["sources"].append(FL.src(4, 9.0))                                  # a fifth component without any of the three
    sim, _pools = FL.build(spec)
    parts = split_parts(sim.lowered().arrays)
    assert len(parts) == 5
    with_flows = [b for _ids, _pos, b in parts if b.flow_params is not None]
    assert len(with_flows) == 4 and all(sorted(b.kind[b.kind >= N.NODE_BATCH_PROCESSOR].tolist()) == [12, 13, 14] for b in with_flows)
    assert all((b.flow_params[b.kind < N.NODE_BATCH_PROCESSOR] == 0).all() for b in with_flows)


# ---- family_checks.compare on one of this family's recordings, as tests/test_family_checks_host.py does for the others -------------
def _case():
    spec = FL.FIXTURES["gate_conveyor_processor_chain"]
    ref = FR.get("case", spec)
    got = copy.deepcopy(ref)
    got["by_kind"] = ref["by_kind"][:N.EV_KINDS].copy()
    for key, (lo, hi) in {"internal_by_kind": (15, 19), "other_by_kind": (19, 31), "flow_by_kind": (31, 39)}.items():
        got[key] = ref["by_kind"][lo:hi].copy()
    return spec["name"], got, ref


def test_compare_passes_an_unaltered_copy_and_the_set_is_the_literal():
    name, got, ref = _case()
    assert FL.NOT_COMPARED == {"trace", "by_kind", "pending_events", "time_travel"} and FL.BY_KIND_SLICES[-1][1] == len(ref["by_kind"]) == 39
    FL.compare(name, got, ref)


def test_compare_raises_on_every_kind_of_difference():
    name, got, ref = _case()
    arrays = [k for k, v in ref.items() if k not in FL.NOT_COMPARED and isinstance(v, np.ndarray) and v.size]
    assert len(arrays) >= 8 and "flow_stats" in arrays
    for key in arrays:
        altered = dict(got, **{key: got[key].copy()})
        altered[key].flat[-1] += 1
        with pytest.raises(AssertionError, match=key):
            FL.compare(name, altered, ref)
    zeros = np.flatnonzero((ref["sink_latency_s"] == 0.0) & ~np.signbit(ref["sink_latency_s"]))
    for key in (k for k in arrays if ref[k].dtype == np.float64):
        with pytest.raises(AssertionError, match=key):
            FL.compare(name, dict(got, **{key: got[key].astype(np.float32)}), ref)
    assert len(zeros) == 0                                         # (a Request spends time at the conveyor: no latency is 0.0 here)
    for key in ("final_ns", "total_events", "events_cancelled", "fault_events"):
        with pytest.raises(AssertionError, match=key):
            FL.compare(name, dict(got, **{key: got[key] + 1}), ref)
    first = 0
    for part, end in FL.BY_KIND_SLICES:
        altered = dict(got, **{part: got[part].copy()})
        altered[part].flat[0] += 1
        with pytest.raises(AssertionError, match=rf"by_kind\[{first}:{end}\]"):
            FL.compare(name, altered, ref)
        first = end
    with pytest.raises(AssertionError):
        FC.compare(name, got, ref, FL.NOT_COMPARED, FL.BY_KIND_SLICES[:-1])
    for key in (k for k in ref if k not in FL.NOT_COMPARED):
        with pytest.raises(AssertionError, match=key):
            FL.compare(name, {k: v for k, v in got.items() if k != key}, ref)
    for key in FL.NOT_COMPARED - {"by_kind"}:
        FL.compare(name, dict(got, **{key: "something else"}), ref)


def test_the_new_symbols_are_in_the_header_and_the_library_and_no_struct_changed():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    syms = ("hs_graph_set_flow", "hs_graph_schedule_gate", "hs_graph_get_flow")
    for sym in syms:
        assert re.search(rf"\bint {sym}\(hs_graph \*g", hdr) and sym in N.EXPORTED_SYMBOLS
    assert re.search(r"HS_NODE_CLIENT = 11,", hdr) and re.search(r"HS_NODE_BATCH_PROCESSOR = 12,", hdr) and re.search(r"HS_NODE_CONVEYOR = 13,", hdr)
    assert re.search(r"HS_NODE_GATE = 14\b", hdr) and (N.NODE_BATCH_PROCESSOR, N.NODE_CONVEYOR, N.NODE_GATE) == (12, 13, 14)
    assert re.search(r"#define HS_ABI_VERSION 16\b", hdr) and N.ABI_VERSION == 16 and N.EV_KINDS == 15
    assert re.search(r"#define HS_FLOW_MAX_ITEMS \(1 << 20\)", hdr) and re.search(rf"#define HS_FLOW_COUNTERS {N.FLOW_COUNTERS}\b", hdr)
    assert re.search(rf"#define HS_FLOW_KINDS {N.FLOW_KINDS}\b", hdr) and N.FLOW_KINDS == len(FL.EV_FLOW)
    for name, code in N.PROBE_FLOW_METRICS.items():
        tag = {"buffer_depth": "BP_BUFFER_DEPTH", "items_in_transit": "CV_IN_TRANSIT", "queue_depth": "GT_QUEUE_DEPTH"}[name]
        assert re.search(rf"HS_PROBE_{tag} = {code}\b", hdr)
    # the struct sizes tests/test_abi.py pins: additive only
    assert C.sizeof(N.GraphConfig) == 64 and C.sizeof(N.GraphNodes) == 208 and C.sizeof(N.GraphStats) == 128
    assert C.sizeof(N.Config) == 56 and C.sizeof(N.Summary) == 8 * (1 + 15 + 1 + 1 + 1 + 1) + 8 + 8 + 8 + 8 + 8
    if os.path.exists(N.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
        for sym in syms:
            assert re.search(rf" T {sym}$", out, re.M), sym
        lib = N.lib()
        assert lib.hs_abi_version() == 16
        for sym in syms:
            getattr(lib, sym)
