"""Host side of PooledCycleResource and InventoryBuffer (no GPU): the constructors and the reference's ValueError texts, the properties
before a run, every refusal by its text, the lowered arrays, the lowering of every recorded spec, the coverage of the recordings under
tests/golden/live_stock/ (computed from the files alone), the new macros, probe codes and symbols of the C ABI (still version 16) and
the fact that a Simulation without the two entities lowers exactly as before."""
import os
import re

import numpy as np
import pytest

import happy_simulator_amd as hs
import stock_specs as ST
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_arrays import split_parts
from happy_simulator_amd.lowering import UnsupportedTopology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EV = {name: ST.EV_ST_FIRST + k for k, name in enumerate(ST.ST_EVENTS)}


def _chain(make, **sim_kw):
    """Source -> make(server, sink) -> ...: a Simulation over whatever `make` returns as (first entity, other entities)."""
    sink = hs.Sink("sink")
    server = hs.Server("srv", service_time=hs.ConstantLatency(0.01), downstream=sink)
    first, others = make(server, sink)
    src = hs.Source.constant(rate=5.0, target=first, name="src")
    return hs.Simulation(sources=[src], entities=[server, sink, first] + list(others), end_time=hs.Instant.from_seconds(1.0), **sim_kw)


def _refused(make, text, **sim_kw):
    with pytest.raises(NotImplementedError, match=re.escape(text)) as err:
        _chain(make, **sim_kw).lowered()
    assert isinstance(err.value, UnsupportedTopology)


def test_constructors_properties_and_the_references_value_errors():
    sink, other = hs.Sink("sink"), hs.Sink("other")
    p = hs.PooledCycleResource("pool", 3, 0.25, downstream=sink, queue_capacity=4)
    assert (p.name, p.pool_size, p.cycle_time, p.downstream, p._queue_capacity, p.downstream_entities()) == ("pool", 3, 0.25, sink, 4, [sink])
    assert (p.available, p.active, p.queued, p.completed, p.rejected, p.utilization) == (3, 0, 0, 0, 0, 0.0) and len(p._queue) == 0
    assert p.stats == hs.PooledCycleStats(pool_size=3, available=3, active=0, queued=0, completed=0, rejected=0, utilization=0.0)
    assert list(hs.PooledCycleStats.__dataclass_fields__) == ["pool_size", "available", "active", "queued", "completed", "rejected", "utilization"]
    assert hs.PooledCycleStats() == hs.PooledCycleStats(0, 0, 0, 0, 0, 0, 0.0)
    with pytest.raises(Exception):
        p.stats.completed = 1
    q = hs.PooledCycleResource("pool", 1, 0)
    assert q.downstream is None and q.downstream_entities() == [] and q._queue_capacity == 0 and q.cycle_time == 0
    for size in (0, -2):
        with pytest.raises(ValueError, match=re.escape(f"pool_size must be > 0, got {size}")):
            hs.PooledCycleResource("pool", size, 1.0)
    with pytest.raises(ValueError, match=re.escape("cycle_time must be >= 0, got -0.5")):
        hs.PooledCycleResource("pool", 1, -0.5)
    b = hs.InventoryBuffer("buf")
    assert (b.stock, b.reorder_point, b.order_quantity, b.lead_time, b.supplier, b.downstream, b.stockout_target) == (100, 20, 50, 5.0, None, None, None)
    assert b.downstream_entities() == [] and b._order_pending is False
    assert b.stats == hs.InventoryStats(current_stock=100, stockouts=0, reorders=0, items_consumed=0, items_replenished=0) and b.stats.fill_rate == 1.0
    assert list(hs.InventoryStats.__dataclass_fields__) == ["current_stock", "stockouts", "reorders", "items_consumed", "items_replenished"]
    assert hs.InventoryStats(items_consumed=3, stockouts=1).fill_rate == 0.75 and hs.InventoryStats().current_stock == 0
    with pytest.raises(Exception):
        b.stats.stockouts = 1
    sup = hs.Sink("sup")
    b = hs.InventoryBuffer("buf", 0, 0, 1, 0.0, supplier=sup, downstream=sink, stockout_target=other)
    assert b.downstream_entities() == [sink, sup, other] and b.stock == 0
    for kw, text in ((dict(initial_stock=-1), "initial_stock must be >= 0, got -1"), (dict(reorder_point=-3), "reorder_point must be >= 0, got -3"),
                     (dict(order_quantity=0), "order_quantity must be > 0, got 0"), (dict(order_quantity=-4), "order_quantity must be > 0, got -4")):
        with pytest.raises(ValueError, match=re.escape(text)):
            hs.InventoryBuffer("buf", **kw)


def test_a_simulation_with_either_entity_is_lowered_to_the_single_heap_loop():
    sim = _chain(lambda server, sink: (hs.PooledCycleResource("pool", 2, 0.1 + 0.2, downstream=server, queue_capacity=5), []))
    g = sim.lowered()
    a = g.arrays
    assert "PooledCycleResource or InventoryBuffer" in sim._station_refusal and a.has_stock and "st_params" not in vars(a) and "_st_params" in vars(a)
    node = int(np.nonzero(a.kind == N.NODE_POOLED_CYCLE)[0][0])
    assert a.st_params.dtype == np.int64 and a.st_params[node].tolist() == [2, int((0.1 + 0.2) * 1_000_000_000), 5, 0, -1]
    assert a.target[node] == g.node_of[id(g.nodes[node].downstream)]
    sim = _chain(lambda server, sink: (hs.PooledCycleResource("pool", 1, 0.5), []))        # no downstream: target -1; the line unbounded
    a = sim.lowered().arrays
    assert a.target[-1] == -1 and a.st_params[-1].tolist() == [1, 500_000_000, 0, 0, -1]
    other = hs.Sink("other")
    sim = _chain(lambda server, sink: (hs.InventoryBuffer("buf", 7, 3, (1 << 62), 1.0 / 3.0, supplier=sink, downstream=server, stockout_target=other), [other]))
    g = sim.lowered()
    a = g.arrays
    node = int(np.nonzero(a.kind == N.NODE_INVENTORY)[0][0])
    row = a.st_params[node]
    assert row[:3].tolist() == [7, 3, 1 << 62] and row[3:4].view(np.float64)[0] == 1.0 / 3.0 and row[4] == g.node_of[id(other)]
    assert a.target[node] == g.node_of[id(g.nodes[node].downstream)] and "PooledCycleResource or InventoryBuffer" in sim._station_refusal
    # a Source's target counts: a pool that `entities` does not list is found downstream and forces the single heap all the same
    sink = hs.Sink("sink")
    pool = hs.PooledCycleResource("pool", 1, 0.1, downstream=sink)
    sim = hs.Simulation(sources=[hs.Source.constant(rate=5.0, target=pool, name="src")], entities=[sink], end_time=hs.Instant.from_seconds(1.0))
    assert sim.lowered().arrays.has_stock and "PooledCycleResource" in sim._station_refusal


def test_split_parts_and_the_walks_see_every_edge_of_a_buffer():
    """The stock-out edge joins two groups into one part and is renumbered inside it; the supplier and the stock-out target are among
    the entities a walk over downstream_entities() reaches -- a Random LoadBalancer behind either is found."""
    spec = ST.groups_spec()
    sim, pools = ST.build(spec)
    g = sim.lowered()
    parts = split_parts(g.arrays)
    assert len(parts) == 6
    for ids, _pos, b in parts:
        assert b.has_stock and (b.kind == N.NODE_INVENTORY).sum() == 1 == (b.kind == N.NODE_POOLED_CYCLE).sum()
        at = int(np.nonzero(b.kind == N.NODE_INVENTORY)[0][0])
        so = int(b.st_params[at, 4])
        want = g.nodes[ids[at]].stockout_target
        assert (so == -1 and want is None) or g.nodes[ids[so]] is want
    sinks = [hs.Sink("a"), hs.Sink("b")]
    buf = hs.InventoryBuffer("buf", 1, 0, 1, 0.1, downstream=sinks[0], stockout_target=sinks[1])
    srcs = [hs.Source.constant(rate=5.0, target=buf, name="s0"), hs.Source.constant(rate=5.0, target=sinks[1], name="s1")]
    a = hs.Simulation(sources=srcs, entities=sinks + [buf], end_time=hs.Instant.from_seconds(1.0)).lowered().arrays
    assert split_parts(a) is None                                                          # one component through the stock-out edge
    srv = hs.Server("srv", service_time=hs.ConstantLatency(0.01), downstream=sinks[0])
    lb = hs.LoadBalancer("lb", backends=[srv], strategy=hs.Random())
    for kw in (dict(stockout_target=lb), dict(supplier=lb)):
        buf = hs.InventoryBuffer("buf", 1, 0, 1, 0.1, downstream=sinks[0], **kw)
        sim = hs.Simulation(sources=[hs.Source.constant(rate=5.0, target=buf, name="s0")], entities=sinks + [buf, lb, srv], end_time=hs.Instant.from_seconds(1.0))
        with pytest.raises(UnsupportedTopology, match="reaches the Random LoadBalancer 'lb' through other entities"):
            sim.lowered()


def test_probes_on_the_four_metrics():
    sink = hs.Sink("sink")
    pool = hs.PooledCycleResource("pool", 2, 0.1, downstream=sink)
    buf = hs.InventoryBuffer("buf", 5, 1, 5, 0.2, downstream=pool)
    probes = [hs.Probe.on(pool, m, interval=0.1)[0] for m in ("available", "active", "queued")] + [hs.Probe.on(buf, "stock", interval=0.1)[0]]
    src = hs.Source.constant(rate=5.0, target=buf, name="src")
    a = hs.Simulation(sources=[src], entities=[sink, pool, buf], probes=probes, end_time=hs.Instant.from_seconds(1.0)).lowered().arrays
    assert a.probe_metric[1:5].tolist() == [18, 19, 20, 21] == [N.PROBE_STOCK_METRICS[m] for m in ("available", "active", "queued", "stock")]
    for target, metric in ((buf, "available"), (pool, "stock"), (sink, "queued"), (hs.Server("s"), "active")):
        with pytest.raises(NotImplementedError):
            hs.Probe.on(target, metric)


def test_refusals_by_name():
    pool = lambda to, **kw: hs.PooledCycleResource("pool", 1, 0.1, downstream=to, **kw)  # noqa: E731
    buf = lambda to, **kw: hs.InventoryBuffer("buf", 1, 0, 1, 0.1, downstream=to, **kw)  # noqa: E731
    link = lambda name, to: hs.NetworkLink(name, latency=hs.ConstantLatency(0.01), egress=to)  # noqa: E731
    # as a LoadBalancer's backend
    _refused(lambda server, sink: (hs.LoadBalancer("lb", backends=[pool(server)]), []), "backend 'pool' of 'lb' is a PooledCycleResource: only Server backends are lowered")
    _refused(lambda server, sink: (hs.LoadBalancer("lb", backends=[buf(server)]), []), "backend 'buf' of 'lb' is a InventoryBuffer: only Server backends are lowered")
    # as the target, primary or fallback entity of what hangs a completion hook on the Event, directly and through NetworkLinks
    hook = " -- a completion hook on an item that a PooledCycleResource or an InventoryBuffer holds or forwards is not lowered (a follow-up)"
    for kind, name, make in (("PooledCycleResource", "pool", pool), ("InventoryBuffer", "buf", buf)):
        for what, wrap, role in (("Bulkhead 'w'", lambda to, sink: hs.Bulkhead("w", to, 2), "target"),
                                 ("TimeoutWrapper 'w'", lambda to, sink: hs.TimeoutWrapper("w", to, 0.1), "target"),
                                 ("Client 'w'", lambda to, sink: hs.Client("w", to), "target"),
                                 ("Hedge 'w'", lambda to, sink: hs.Hedge("w", to, 0.1), "target"),
                                 ("Fallback 'w'", lambda to, sink: hs.Fallback("w", to, sink), "primary"),
                                 ("Fallback 'w'", lambda to, sink: hs.Fallback("w", sink, to), "fallback entity")):
            _refused(lambda server, sink: (wrap(make(server), sink), []), f"{what}: its {role} is the {kind} '{name}'" + hook)
            _refused(lambda server, sink: (wrap(link("l1", link("l2", make(server))), sink), []),
                     f"{what}: its {role} (through its NetworkLinks) is the {kind} '{name}'" + hook)
    # sizes and times the engine does not hold
    big = (1 << 20) + 1
    _refused(lambda server, sink: (hs.PooledCycleResource("pool", big, 0.1, downstream=server), []),
             f"PooledCycleResource 'pool': pool_size = {big} is beyond the 1048576 the engine holds (PooledCycleResource.MAX_POOL_SIZE)")
    _refused(lambda server, sink: (pool(server, queue_capacity=big), []),
             f"PooledCycleResource 'pool': queue_capacity = {big} is beyond the 1048576 the engine holds (PooledCycleResource.MAX_POOL_SIZE); 0 is unbounded")
    _refused(lambda server, sink: (hs.PooledCycleResource("pool", 1.5, 0.1, downstream=server), []), "PooledCycleResource 'pool': pool_size must be an int, got 1.5")
    for bad in (float("inf"), float("nan")):
        _refused(lambda server, sink: (hs.PooledCycleResource("pool", 1, bad, downstream=server), []),
                 f"PooledCycleResource 'pool': cycle_time = {bad!r} is not a finite number >= 0")
        _refused(lambda server, sink: (hs.InventoryBuffer("buf", 1, 0, 1, bad, downstream=server), []),
                 f"InventoryBuffer 'buf': lead_time = {bad!r} is not a finite number >= 0")
    _refused(lambda server, sink: (hs.InventoryBuffer("buf", 1, 0, 1, -0.5, downstream=server), []), "InventoryBuffer 'buf': lead_time = -0.5 is not a finite number >= 0")
    beyond = (1 << 62) + 1
    for kw, nm in ((dict(initial_stock=beyond), "initial_stock"), (dict(reorder_point=beyond), "reorder_point"), (dict(order_quantity=beyond), "order_quantity")):
        _refused(lambda server, sink: (hs.InventoryBuffer("buf", downstream=server, **kw), []),
                 f"InventoryBuffer 'buf': {nm} = {beyond} is beyond 2^62 (InventoryBuffer.MAX_STOCK)")
    _refused(lambda server, sink: (hs.InventoryBuffer("buf", 1, 0, 2.5, 0.1, downstream=server), []), "InventoryBuffer 'buf': order_quantity must be an int, got 2.5")
    # each at most 2^62, and together no more than the level a 64-bit stock holds: at 2^62 + 2^62 the second replenish would reach 2^63
    _refused(lambda server, sink: (hs.InventoryBuffer("buf", 0, 1 << 62, 1 << 62, 0.1, downstream=server), []),
             f"InventoryBuffer 'buf': reorder_point + order_quantity = {1 << 63} is beyond 2^63 - 2^48, the level a 64-bit stock holds")
    ok = _chain(lambda server, sink: (hs.InventoryBuffer("buf", 1 << 62, (1 << 62) - (1 << 48), 1 << 62, 0.1, downstream=server), []))
    assert ok.lowered().arrays.has_stock and hs.InventoryBuffer.MAX_LEVEL == N.INVENTORY_MAX_LEVEL == (1 << 63) - (1 << 48)
    # a receiver that takes no Requests
    _refused(lambda server, sink: (buf(server, stockout_target=hs.Source.constant(rate=1.0, target=sink, name="other")), []), "a Source takes no Requests")
    # a scheduled Event that carries a quantity, or a hand-made replenish: next to a buffer they are refused wherever they are aimed
    for ev_kw, aim in ((dict(event_type="Request", context={"quantity": 3}), "buffer"), (dict(event_type="_InventoryReplenish"), "buffer"),
                       (dict(event_type="_InventoryReplenish"), "server"), (dict(event_type="Request", context={"quantity": 1}), "server")):
        sim = _chain(lambda server, sink: (buf(server), []))
        target = sim._entities[2] if aim == "buffer" else sim._entities[0]
        sim.schedule(hs.Event(time=hs.Instant.from_seconds(0.5), target=target, **ev_kw))
        g = sim.lowered()
        with pytest.raises(UnsupportedTopology, match="a hand-made '_InventoryReplenish' Event and a 'quantity' in an Event's context are not lowered"):
            sim._general_prepare(g, False)
    # in a ParallelSimulation partition
    for make in (pool, buf):
        sink = hs.Sink("sink")
        ent = make(sink)
        part = hs.SimulationPartition("p0", sources=[hs.Source.constant(rate=5.0, target=ent, name="src")], entities=[ent, sink])
        with pytest.raises(UnsupportedTopology, match=f"partition 'p0': the {type(ent).__name__} '{ent.name}' on a ParallelSimulation partition is not lowered"):
            hs.ParallelSimulation(partitions=[part], end_time=hs.Instant.from_seconds(1.0)).run()


def test_every_recorded_spec_is_lowered_and_recorded():
    specs = ST.recorded_specs()
    assert len(specs) == 160 and len(ST.FIXTURES) == 58 and len(ST.TRACED) == 33 and ST.N_RANDOM == 100
    for spec in specs:
        sim, pools = ST.build(spec)
        g = sim.lowered()
        sim._general_prepare(g, bool(spec.get("auto")))
        a = g.arrays
        assert a.has_stock and ((a.kind == N.NODE_POOLED_CYCLE).sum(), (a.kind == N.NODE_INVENTORY).sum()) == (len(pools["pool"]), len(pools["buffer"]))
        ref = ST.STOCK.get("case", spec)
        assert len(ref["by_kind"]) == ST.N_KINDS == 64 and not ref["by_kind"][39:ST.EV_ST_FIRST].any() and ref["total_events"] == ref["by_kind"].sum()
        assert ref["pc_state"].shape == (len(pools["pool"]), 6) and ref["ib_state"].shape == (len(pools["buffer"]), 7)
        assert ("trace" in ref) == (spec["name"] in ST.TRACED)
    sizes = sorted(ST.group_sizes(ST.groups_spec()))
    assert len(sizes) == 6 and 48 in sizes and 49 in sizes
    src = open(os.path.join(N.CSRC, "hs_graph.hip")).read()
    assert "kLdsNodesBatch = 48" in src


def _rounded(spec, ref):
    trace, lead_ns = ref["trace"], int(spec["buffers"][0]["lt"] * 1_000_000_000)
    consumes = set(trace[trace[:, 1] == EV["ib_item"]][:, 0].tolist())
    return sum(1 for t in trace[trace[:, 1] == EV["ib_replenish"]][:, 0].tolist() if t - lead_ns not in consumes)


def test_the_recordings_cover_what_the_handlers_can_get_wrong():
    """From the files alone: every kind in many cases, re-sent Requests that lose their unit and queue again, re-sent Requests lost at a
    crashed pool, rejections, stock-outs, an order that stays pending at a live buffer, replenishments that an integer addition of
    nanoseconds would put elsewhere."""
    refs = {spec["name"]: ST.STOCK.get("case", spec) for spec in ST.recorded_specs()}
    kinds = np.sum([r["by_kind"][ST.EV_ST_FIRST:] > 0 for r in refs.values()], axis=0)
    assert kinds.min() >= 40, kinds
    count = lambda pred: sum(1 for r in refs.values() if pred(r))  # noqa: E731
    assert count(lambda r: r["requeued"] > 0) >= 5 and count(lambda r: r["lost"] > 0) >= 5
    assert count(lambda r: (r["pc_state"][:, 4] > 0).any()) >= 5 and count(lambda r: (r["ib_state"][:, 1] > 0).any()) >= 5
    assert count(lambda r: (r["pc_state"][:, 2] > 0).any()) >= 10                          # a line at the end of the run
    r = refs["crash_over_a_replenish_leaves_the_order_pending"]
    assert r["ib_state"][0].tolist()[2:] == [1, r["ib_state"][0, 3], 0, 1, 0] and r["ib_state"][0, 1] > 3      # one reorder, nothing came, pending, live
    assert refs["resent_request_loses_the_unit_to_an_arrival_of_its_nanosecond"]["requeued"] > 3
    assert refs["crashed_pool_restarts_with_a_line"]["lost"] >= 1 and refs["paused_pool_across_a_cycle_end"]["lost"] >= 1
    for name in ST.ROUNDED:
        assert _rounded(ST.FIXTURES[name], refs[name]) >= 3, name
    assert refs["large_order_quantity"]["ib_state"][0, 0] > (1 << 60)
    assert refs["line_of_400_requests_at_one_pool"]["pc_state"][0, 2] > 300
    for name in ST.FIXTURES:
        if name.endswith("_in_windows"):
            a, b = refs[name[:-len("_in_windows")]], refs[name]
            assert ST.WINDOW_KEYS <= set(b) and len(b["window_pc_state"]) == 6
            assert all(a[k].tobytes() == b[k].tobytes() for k in a if k != "trace" and isinstance(a[k], np.ndarray))


def test_compare_sees_a_difference_in_a_stock_case():
    spec = ST.FIXTURES["buffer_pool_server_sink"]
    ref = ST.STOCK.get("case", spec)
    got = dict(ref, by_kind=ref["by_kind"][:15].copy())
    first = 15
    for key, end in ST.BY_KIND_SLICES[1:]:
        got[key] = ref["by_kind"][first:end].copy()
        first = end
    ST.compare(spec["name"], got, ref)
    for key in ("pc_state", "ib_state", "stock_by_kind"):
        with pytest.raises(AssertionError):
            ST.compare(spec["name"], dict(got, **{key: got[key] + 1}), ref)


def test_the_c_abi_gains_symbols_macros_and_probe_codes_at_version_16():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    assert "#define HS_ABI_VERSION 16" in hdr
    assert re.search(r"HS_NODE_POOLED_CYCLE = 20,", hdr) and re.search(r"HS_NODE_INVENTORY = 21\b", hdr) and (N.NODE_POOLED_CYCLE, N.NODE_INVENTORY) == (20, 21)
    for macro, value in (("HS_PROBE_PC_AVAILABLE", 18), ("HS_PROBE_PC_ACTIVE", 19), ("HS_PROBE_PC_QUEUED", 20), ("HS_PROBE_IB_STOCK", 21)):
        assert re.search(rf"\b{macro} = {value},", hdr), macro
    assert re.search(r"#define HS_STOCK_KINDS 4\b", hdr) and N.STOCK_KINDS == 4 and re.search(r"#define HS_POOL_MAX_UNITS \(1 << 20\)", hdr)
    assert re.search(r"#define HS_POOL_COUNTERS 5\b", hdr) and re.search(r"#define HS_INVENTORY_COUNTERS 6\b", hdr) and re.search(r"#define HS_INVENTORY_MAX \(1ll << 62\)", hdr)
    assert (N.POOL_MAX_UNITS, N.INVENTORY_MAX, N.POOL_COUNTERS, N.INVENTORY_COUNTERS) == (1 << 20, 1 << 62, 5, 6)
    assert re.search(r"#define HS_INVENTORY_MAX_LEVEL 0x7fff000000000000ll", hdr) and N.INVENTORY_MAX_LEVEL == 0x7fff000000000000
    assert hs.PooledCycleResource.MAX_POOL_SIZE == N.POOL_MAX_UNITS and hs.InventoryBuffer.MAX_STOCK == N.INVENTORY_MAX
    for sym in ("hs_graph_set_pool", "hs_graph_set_inventory", "hs_graph_get_pool", "hs_graph_get_inventory"):
        assert re.search(rf"\bint {sym}\(hs_graph \*g", hdr) and sym in N.EXPORTED_SYMBOLS
    assert N.GRAPH_LEVEL_STOCK == 11 == N.GRAPH_LEVEL_HEDGE + 1
    src = open(os.path.join(N.CSRC, "hs_graph.hip")).read()
    # the four kinds fill the kind word: 64 of 64, asserted with equality where the loop's tables are built
    assert "kEvStKinds = kEvHgKinds + HS_STOCK_KINDS" in src and 'static_assert(kEvStKinds <= 64' in src
    assert 53 + N.HEDGE_KINDS + N.STOCK_KINDS == 64 == ST.N_KINDS
    for name in ("InventoryBuffer", "InventoryStats", "PooledCycleResource", "PooledCycleStats"):
        assert hasattr(hs, name)


def test_a_simulation_without_the_entities_lowers_exactly_as_before():
    sim = _chain(lambda server, sink: (hs.ConveyorBelt("cv", server, 0.1), []))
    a = sim.lowered().arrays
    assert not a.has_stock and a.st_params is None and "_st_params" not in vars(a) and "st_params" not in vars(a)
    assert "PooledCycleResource" not in sim._station_refusal
    sim = _chain(lambda server, sink: (hs.Hedge("hg", server, 0.05), []))
    a = sim.lowered().arrays
    assert a.has_hedges and not a.has_stock and "_st_params" not in vars(a)
    plain = hs.Simulation(duration=1.0, sources=[hs.Source.poisson(rate=5.0, target=(sv := hs.Server("s", downstream=hs.Sink("k"))))], entities=[sv, sv.downstream])
    from happy_simulator_amd.graph_engine import GeneralGraph

    assert not isinstance(plain.lowered(), GeneralGraph)                                   # (a plain chain still takes the station engine)
