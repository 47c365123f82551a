"""Specs of PooledCycleResource and InventoryBuffer (happy_simulator_amd.entities; the reference's components/industrial/pooled_cycle.py,
inventory.py) on the single-heap loop.  The format is the mixed family's (tests/mixed_specs.py, tests/graph_family.py) with two more lists:

  pools   = [dict(to=<ref | None>, n=<pool_size>, ct=<cycle_time s>, cap=<queue_capacity>)]       PooledCycleResource(f"pc{i}", ...)
  buffers = [dict(to=<ref | None>, init=, rp=, q=, lt=<lead_time s>, so=<ref | None>, sup=<ref | None>)]    InventoryBuffer(f"ib{i}", ...)
  every <ref> of the format may be ["pool", i] or ["buffer", i]; faults, probes and the schedule may name them.

`wire()` here is graph_family.wire's counterpart for these specs -- both libraries see the same objects in the same order: entities =
servers + lbs + routers + links + limiters + sinks + flows + pools + buffers; a spec of this family may hold LoadBalancers (their
backends are Servers) but no Bulkhead, TimeoutWrapper, Client, HealthChecker, Hedge or Fallback (those pools exist and are empty, so the
other families' result readers apply).

tests/golden/make_golden_stock.py records every spec listed here from the live reference as family "stock": what the "mixed" family
records, twenty-five more by_kind rows (39 .. 59: the scaler's, the deployers' and the hedges', always 0; 60 .. 63: ST_EVENTS) and
stock_results below.  STOCK reads the recordings back.  Every case has at most a few seconds of simulated time (one lead-time case: 8 s at a
low rate) and at most 60 000 Events.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded chains Source(s) -> 2 .. 5 stations -> Sink with at least one pool or buffer among them
  groups_spec()   6 disconnected groups, one of 48 and one of 49 nodes among them: the parts of hs_graph_run_parts
  growth_spec()   a line of some 400 Requests at one pool: heap, Request pool and record log grow from a capacity of one
"""
import numpy as np

import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import mixed_specs as MX
import rate_limiter_specs as RS
from happy_simulator_amd.graph_engine import GraphEngine
from recorded import Recorded

STOCK = Recorded("live_stock", "stock", "make_golden_stock.py", part_bytes=640 * 1024)
N_RANDOM = 100
EV_ST_FIRST = 60                               # the by_kind row of a Request at a pool, the first of the four
ST_EVENTS = ("pc_item", "pc_cont", "ib_item", "ib_replenish")
N_KINDS = EV_ST_FIRST + len(ST_EVENTS)
crash, pause, src, plain, srv, link, bp, cv = MX.crash, MX.pause, MX.src, MX.plain, MX.srv, MX.link, MX.bp, MX.cv
SINK, SINK1, S0, S1, L0, R0, LIM0, F0, P0, P1, B0, B1 = (["sink", 0], ["sink", 1], ["server", 0], ["server", 1], ["link", 0], ["router", 0],
                                                          ["limiter", 0], ["flow", 0], ["pool", 0], ["pool", 1], ["buffer", 0], ["buffer", 1])
THIRD = 1.0 / 3.0                              # a lead time that is no binary fraction (like 0.1)
START_1E5 = 10 ** 14                           # a start time of 10^5 s in ns: to_seconds(now) + lead_time rounds at 2^-36 s there


def pc(to, n=1, ct=0.1, cap=0):
    return dict(to=to, n=n, ct=ct, cap=cap)


def ib(to, init=100, rp=20, q=50, lt=5.0, so=None, sup=None):
    return dict(to=to, init=init, rp=rp, q=q, lt=lt, so=so, sup=sup)


def keyed(to, rate=10.0, kind="poisson", n_clients=7):
    return dict(src(to, rate, kind), n_clients=n_clients)


def _g(name, *, pools=(), buffers=(), **kw):
    return dict(MX._g(name, **kw), pools=[dict(p) for p in pools], buffers=[dict(b) for b in buffers])


def wire(spec, F, ns):
    """The spec's objects from the factory `F` (graph_family.Product, or the recorder's) and the namespace `ns` (where
    PooledCycleResource, InventoryBuffer and the flow entities come from): (pools by kind, Sources, Probes, entities)."""
    assert not (spec.get("wrappers") or spec.get("clients") or spec.get("checkers")), spec["name"]
    sinks = [F.sink(j) for j in range(spec["n_sinks"])]
    servers = [F.server(i, sv) for i, sv in enumerate(spec["servers"])]
    limiters = [F.limiter(i, lm) for i, lm in enumerate(spec.get("limiters") or [])]
    links = [F.link(l, lk) for l, lk in enumerate(spec["links"])]
    lbs = [F.lb(j, lb, [servers[b] for b in lb["backends"]]) for j, lb in enumerate(spec.get("lbs") or [])]
    pools = {"sink": sinks, "server": servers, "limiter": limiters, "link": links, "lb": lbs, "wrapper": [], "client": [], "checker": []}
    later = {kind: spec.get(key) or [] for kind, key in (("router", "routers"), ("flow", "flows"), ("pool", "pools"), ("buffer", "buffers"))}
    for kind, items in later.items():
        pools[kind] = [None] * len(items)

    def ref(r):
        return None if r is None else servers[r] if isinstance(r, int) else pools[r[0]][r[1]]

    def ready(r):
        return r is None or isinstance(r, int) or pools[r[0]][r[1]] is not None

    pending = [(kind, i) for kind, items in later.items() for i in range(len(items))]
    while pending:
        progressed = False
        for kind, i in list(pending):
            item = later[kind][i]
            needs = item["targets"] if kind == "router" else [item["to"], item["so"], item["sup"]] if kind == "buffer" else [item["to"]]
            if not all(ready(t) for t in needs):
                continue
            if kind == "router":
                pools[kind][i] = F.router(i, [ref(t) for t in needs])
            elif kind == "flow":
                pools[kind][i] = GF.make_flow(ns, i, item, ref(item["to"]))
            elif kind == "pool":
                pools[kind][i] = ns.PooledCycleResource(f"pc{i}", item["n"], item["ct"], downstream=ref(item["to"]), queue_capacity=item["cap"])
            else:
                pools[kind][i] = ns.InventoryBuffer(f"ib{i}", initial_stock=item["init"], reorder_point=item["rp"], order_quantity=item["q"],
                                                    lead_time=item["lt"], supplier=ref(item["sup"]), downstream=ref(item["to"]),
                                                    stockout_target=ref(item["so"]))
            pending.remove((kind, i))
            progressed = True
        assert progressed, "routers, flows, pools and buffers form a cycle"
    for l, lk in enumerate(spec["links"]):
        links[l].egress = None if lk["to"] is None else ref(lk["to"])
    for i, lm in enumerate(spec.get("limiters") or []):
        limiters[i]._downstream = ref(lm["out"])
    for i, sv in enumerate(spec["servers"]):
        if sv.get("out") is not None:
            servers[i].downstream = ref(sv["out"])
    sources = pools["source"] = [F.source(k, sc, ref(sc["to"])) for k, sc in enumerate(spec["sources"])]
    probes = pools["probe"] = [F.probe(ref(on), metric, interval) for on, metric, interval in spec.get("probes") or []]
    entities = servers + lbs + pools["router"] + links + limiters + sinks + pools["flow"] + pools["pool"] + pools["buffer"]
    return pools, sources, probes, entities


def build(spec, seed=None, **sim_kw):
    """(Simulation, entities by pool) of the product, wired like the recorded reference run."""
    pools, sources, probes, entities = wire(spec, GF.Product, hs)
    start_ns = int(spec.get("start_ns", 0))

    def at(t_s):
        return hs.Instant(start_ns + hs.Instant.from_seconds(t_s).nanoseconds)

    fs, handles = GF.make_schedule(hs, spec, pools)
    sim = hs.Simulation(sources=sources, entities=entities, seed=spec["seed"] if seed is None else seed, max_graph_events=400_000,
                        fault_schedule=fs, **({} if spec.get("auto") else {"end_time": at(spec["end_s"])}),
                        **({"start_time": hs.Instant(start_ns)} if start_ns else {}), **({"probes": [p for p, _ in probes]} if probes else {}),
                        **sim_kw)
    GF.cancel_after(spec, handles)
    GF.schedule_all(spec, pools, sim, hs.Event, at, [])
    pools["probes"] = probes
    pools["fault_schedule"], pools["handles"] = fs, handles
    return sim, pools


def stock_state(pools):
    """The object state of every pool and buffer, as arrays.  pc_state rows: _available, _active, len(_queue), _completed, _rejected,
    _crashed; ib_state rows: _stock, _stockouts, _reorders, _items_consumed, _items_replenished, _order_pending, _crashed."""
    pc_rows = [[p._available, p._active, len(p._queue), p._completed, p._rejected, int(bool(getattr(p, "_crashed", False)))] for p in pools["pool"]]
    ib_rows = [[b._stock, b._stockouts, b._reorders, b._items_consumed, b._items_replenished, int(b._order_pending),
                int(bool(getattr(b, "_crashed", False)))] for b in pools["buffer"]]
    return dict(pc_state=np.asarray(pc_rows, np.int64).reshape(-1, 6), ib_state=np.asarray(ib_rows, np.int64).reshape(-1, 7))


def window_states(states):
    return {"window_" + k: [s[k] for s in states] for k in states[0]}


def stock_results(spec, pools):
    """What both libraries' pools and buffers show after a run: the state, then the public interface (properties and frozen stats)."""
    out = stock_state(pools)
    for p, row in zip(pools["pool"], out["pc_state"]):
        st = p.stats
        assert (p.available, p.active, p.queued, p.completed, p.rejected) == tuple(int(v) for v in row[:5]) == (
            st.available, st.active, st.queued, st.completed, st.rejected) and st.pool_size == p.pool_size and st.utilization == p.utilization
    for b, row in zip(pools["buffer"], out["ib_state"]):
        st = b.stats
        assert (b.stock, st.stockouts, st.reorders, st.items_consumed, st.items_replenished) == tuple(int(v) for v in row[:5]) and st.current_stock == b.stock
    out["pc_utilization"] = np.asarray([p.utilization for p in pools["pool"]], np.float64)
    out["ib_fill_rate"] = np.asarray([b.stats.fill_rate for b in pools["buffer"]], np.float64)
    out["pc_params"] = [[p.pool_size, float(p.cycle_time), p._queue_capacity] for p in pools["pool"]]
    out["ib_params"] = [[b.reorder_point, b.order_quantity, float(b.lead_time)] for b in pools["buffer"]]
    out["st_downstream"] = [[d.name for d in x.downstream_entities()] for x in pools["pool"] + pools["buffer"]]
    return out


def results(spec, sim, pools):
    """Everything the recorder records for "stock" except the trace, read off the product's objects after run()."""
    out = MX.results(spec, sim, pools)
    out.update(stock_results(spec, pools))
    out["idle_by_kind"] = np.zeros(EV_ST_FIRST - MX.BY_KIND_SLICES[-1][1], np.int64)      # the scaler's, the deployers', the hedges': none here
    for key in ("_autoscaler_by_kind", "_deployer_by_kind", "_canary_by_kind", "_hedge_by_kind"):
        assert not hasattr(sim, key), key
    out["stock_by_kind"] = np.asarray(getattr(sim, "_stock_by_kind", np.zeros(len(ST_EVENTS))), np.int64)
    return out


WINDOW_KEYS = {"window_pc_state", "window_ib_state"}
# (requeued / lost: what the recorder counts for the coverage checks of tests/test_stock_host.py)
NOT_COMPARED = MX.NOT_COMPARED | WINDOW_KEYS | {"requeued", "lost"}
BY_KIND_SLICES = MX.BY_KIND_SLICES + [("idle_by_kind", EV_ST_FIRST), ("stock_by_kind", N_KINDS)]


def compare(name, got, ref):
    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    """The spec on a GraphEngine of its own (not yet run), with its faults and its scheduled Events, as Simulation.run() sets it up."""
    sim, pools = build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, bool(spec.get("auto")))
    eng = GraphEngine(g.arrays, seed=spec["seed"], start_ns=start_ns, **caps)
    eng.add_faults(sim._general_faults(g))
    for entry in sched:
        eng.schedule(*entry)
    return sim, pools, g, eng, end_ns, start_ns, cancelled


def engine_run(spec, ends_s, read=None, **caps):
    """engine(spec), run to every end of `ends_s` in turn (None: the spec's own end); the results bound like Simulation.run() binds
    them.  `read(sim, pools, g, eng)` is called behind every end, with the results of the run so far bound."""
    sim, pools, g, eng, end_ns, start_ns, cancelled = engine(spec, **caps)
    with eng:
        for t in ends_s:
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
            if read is not None:
                sim._general_finish(g, eng, end_ns, cancelled, 0.0)
                read(sim, pools, g, eng)
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    return sim, pools


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def pooled(name, pool, sources=None, **kw):
    """Source(s) -> pool -> Sink (or wherever `pool` says)."""
    return _g(name, pools=[pool], servers=kw.pop("servers", []), sources=sources or [src(P0, 10.0, "constant")], end_s=kw.pop("end_s", 3.0), **kw)


def stocked(name, buffer, sources=None, **kw):
    """Source(s) -> buffer -> Sink 0, its stock-outs wherever `buffer` says."""
    return _g(name, buffers=[buffer], servers=kw.pop("servers", []), sources=sources or [src(B0, 20.0, "poisson")], end_s=kw.pop("end_s", 3.0),
              n_sinks=kw.pop("n_sinks", 2), **kw)


def _fixtures():
    f = []
    two = [src(P0, 10.0, "constant"), src(P0, 10.0, "constant")]
    # ---- PooledCycleResource
    # three arrivals 0.1 s apart into one unit of 0.5 s and a line of one: accepted, queued, rejected
    f.append(pooled("pool_accepts_queues_and_rejects_within_three_arrivals", pc(SINK, 1, 0.5, cap=1), seed=11, traced=True))
    # two constant Sources of one period, the cycle as long as the period: both arrivals of a nanosecond sort ahead of the re-sent
    # Request, the first takes the unit and the re-sent one queues again at the back
    f.append(pooled("resent_request_loses_the_unit_to_an_arrival_of_its_nanosecond", pc(SINK, 1, 0.1), two, end_s=2.0, seed=12, traced=True))
    f.append(pooled("resent_request_meets_arrivals_with_two_units", pc(SINK, 2, 0.2), two + [src(P0, 5.0, "constant")], end_s=2.0, seed=13, traced=True))
    f.append(pooled("resent_request_into_a_bounded_line", pc(SINK, 1, 0.1, cap=2), two, end_s=2.0, seed=14, traced=True))
    f.append(pooled("pool_with_a_cycle_time_of_zero", pc(SINK, 1, 0.0), two, end_s=2.0, seed=15, traced=True))
    f.append(pooled("pool_with_a_cycle_time_of_zero_poisson", pc(S0, 2, 0.0, cap=1), [src(P0, 30.0, "poisson")], servers=[srv(0.02)], seed=16))
    f.append(pooled("pool_without_a_downstream", pc(None, 2, 0.15), [src(P0, 20.0, "poisson")], seed=17, traced=True))
    f.append(_g("pool_feeding_a_pool", pools=[pc(P1, 2, 0.07), pc(SINK, 1, 0.05, cap=2)], servers=[], sources=[src(P0, 25.0, "poisson")], end_s=3.0,
                seed=18, traced=True))
    f.append(pooled("pool_of_many_units_poisson", pc(SINK, 5, 0.3), [src(P0, 25.0, "poisson")], seed=19))
    f.append(pooled("client_keyed_source_through_a_pool", pc(S0, 2, 0.1), [keyed(P0, 15.0)], servers=[srv(0.03)], seed=20, traced=True))
    # the line is not empty when the pool crashes: the cycle in progress ends and forwards, the re-sent Request is dropped at the
    # crashed pool (the item is lost, the unit stays free), arrivals are dropped until the restart
    f.append(pooled("crashed_pool_restarts_with_a_line", pc(SINK, 1, 0.3), faults=[crash(P0, 0.5, 1.5)], seed=21, traced=True))
    f.append(pooled("crashed_pool_for_good", pc(SINK, 2, 0.25), [src(P0, 20.0, "poisson")], faults=[crash(P0, 1.0)], seed=22))
    f.append(pooled("paused_pool_across_a_cycle_end", pc(SINK, 1, 0.3), faults=[pause(P0, 0.55, 0.95)], seed=23, traced=True))
    f.append(pooled("paused_pool_poisson", pc(S0, 2, 0.12, cap=4), [src(P0, 30.0, "poisson")], servers=[srv(0.02)], faults=[pause(P0, 1.0, 1.6)], seed=24))
    f.append(pooled("crashed_server_behind_a_pool", pc(S0, 2, 0.1), [src(P0, 20.0, "poisson")], servers=[srv(0.03)], faults=[crash(S0, 0.8, 1.7)], seed=25))
    # ---- InventoryBuffer
    f.append(stocked("buffer_with_no_initial_stock", ib(SINK, 0, 0, 5, 0.3, so=SINK1), seed=31, traced=True))
    f.append(stocked("reorder_point_at_the_initial_stock_reorders_at_the_first_consume", ib(SINK, 5, 5, 8, 0.4, so=SINK1), seed=32, traced=True))
    f.append(stocked("reorder_point_above_the_initial_stock", ib(SINK, 3, 10, 4, 0.2, so=SINK1), seed=33))
    f.append(stocked("reorder_point_zero", ib(SINK, 6, 0, 6, 0.5, so=SINK1), seed=34, traced=True))
    f.append(stocked("lead_time_zero", ib(SINK, 2, 1, 3, 0.0, so=SINK1), seed=35, traced=True))
    f.append(stocked("lead_time_zero_constant_sources", ib(SINK, 1, 0, 1, 0.0, so=SINK1), [src(B0, 10.0, "constant"), src(B0, 10.0, "constant")], seed=36, traced=True))
    # lead times that are no binary fraction, at start times up to 10^5 s: the binary64 sum of seconds and its truncation to ns decide
    for tag, start in (("epoch", 0), ("12345_s", 12_345_678_901_234), ("1e5_s", START_1E5)):
        for lt_tag, lt in (("a_tenth", 0.1), ("a_third", THIRD)):
            f.append(stocked(f"lead_time_{lt_tag}_from_{tag}", ib(SINK, 2, 2, 2, lt, so=SINK1), [src(B0, 30.0, "poisson")], start_ns=start, end_s=3.0,
                             seed=40 + len(f), traced=start == START_1E5))
    # (where the sum and the integer addition part company depends on both numbers: at these three pairs a fifth to a third of the
    #  replenishments land one nanosecond below now + int(lead_time * 1e9) -- the recorder counts them)
    for tag, start, lt_tag, lt, end, rate in (("30000_s", 3 * 10 ** 13, "a_tenth", 0.1, 3.0, 30.0), ("1e4_s", 10 ** 13, "three_tenths", 0.3, 8.0, 15.0),
                                              ("1e5_s", START_1E5, "three_twentieths", 0.15, 4.0, 30.0)):
        f.append(stocked(f"lead_time_{lt_tag}_from_{tag}", ib(SINK, 2, 2, 2, lt, so=SINK1), [src(B0, rate, "poisson")], start_ns=start, end_s=end,
                         seed=40 + len(f), traced=True))
    f.append(stocked("lead_time_a_tenth_constant_source_from_1e5_s", ib(SINK, 1, 1, 1, 0.1, so=SINK1), [src(B0, 7.0, "constant")], start_ns=START_1E5, seed=47))
    f.append(stocked("stock_out_with_a_target", ib(SINK, 4, 1, 3, 0.6, so=SINK1), seed=48, traced=True))
    f.append(stocked("stock_out_without_a_target", ib(SINK, 4, 1, 3, 0.6), seed=49, traced=True))
    f.append(stocked("buffer_without_a_downstream", ib(None, 4, 1, 3, 0.3, so=SINK1), seed=50))
    f.append(stocked("buffer_without_any_target", ib(None, 4, 1, 3, 0.3), seed=51))
    f.append(stocked("both_targets_are_one_sink", ib(SINK, 3, 1, 3, 0.5, so=SINK), n_sinks=1, seed=52, traced=True))
    f.append(stocked("buffer_with_a_supplier", ib(SINK, 5, 2, 4, 0.3, so=SINK1, sup=S0), servers=[srv(0.02)], seed=53))
    f.append(stocked("large_order_quantity", ib(SINK, 1, 0, (1 << 61) + 7, 0.2, so=SINK1), seed=54))
    # the replenish is dropped at the crashed buffer: `_order_pending` stays set, no order is ever placed again
    f.append(stocked("crash_over_a_replenish_leaves_the_order_pending", ib(SINK, 4, 2, 5, 0.5, so=SINK1), [src(B0, 10.0, "constant")],
                     faults=[crash(B0, 0.45, 1.2)], seed=55, traced=True))
    f.append(stocked("paused_buffer", ib(SINK, 6, 2, 5, 0.25, so=SINK1), faults=[pause(B0, 1.0, 1.5)], seed=56))
    f.append(stocked("crashed_stockout_target", ib(SINK, 2, 0, 2, 0.5, so=S0), servers=[srv(0.02, out=SINK1)], faults=[crash(S0, 0.8, 1.6)], seed=57))
    f.append(stocked("client_keyed_source_through_a_buffer", ib(S0, 5, 2, 4, 0.2, so=SINK1), [keyed(B0, 20.0)], servers=[srv(0.02)], seed=58))
    # ---- both
    f.append(_g("buffer_pool_server_sink", buffers=[ib(P0, 5, 2, 6, 0.3, so=SINK1)], pools=[pc(S0, 2, 0.08, cap=3)], servers=[srv(0.03)],
                sources=[src(B0, 25.0, "poisson")], n_sinks=2, end_s=3.0, seed=61, traced=True))
    f.append(_g("pool_feeds_a_buffer_whose_stock_outs_return_to_a_second_pool", pools=[pc(B0, 2, 0.05), pc(SINK1, 1, 0.2, cap=2)],
                buffers=[ib(SINK, 3, 1, 4, 0.4, so=P1)], servers=[], sources=[src(P0, 25.0, "poisson")], n_sinks=2, end_s=3.0, seed=62, traced=True))
    f.append(_g("buffer_feeds_a_buffer", buffers=[ib(B1, 6, 2, 5, 0.3, so=SINK1), ib(SINK, 2, 1, 2, THIRD, so=SINK1)], servers=[],
                sources=[src(B0, 20.0, "poisson")], n_sinks=2, end_s=3.0, seed=63))
    f.append(_g("behind_a_server_a_link_a_router_and_a_limiter", pools=[pc(SINK, 1, 0.06, cap=2)], buffers=[ib(P0, 4, 1, 4, 0.3, so=SINK1)],
                servers=[srv(0.02, out=L0)], links=[link(R0, 0.02, "exp", 0.01)], routers=[dict(targets=[LIM0, P0])], limiters=[MX.token(3, B0)],
                sources=[src(S0, 25.0, "poisson")], n_sinks=2, end_s=3.0, seed=64, traced=True))
    f.append(_g("in_front_of_a_link_a_router_a_limiter_and_flows", pools=[pc(L0, 2, 0.05)], buffers=[ib(P0, 5, 2, 5, 0.2, so=F0)],
                flows=[bp(SINK1, 3, 0.05, 0.2), cv(SINK, 0.1, 3)], links=[link(R0, 0.02)], routers=[dict(targets=[LIM0, ["flow", 1]])],
                limiters=[MX.token(3, SINK)], servers=[], sources=[src(B0, 25.0, "poisson")], n_sinks=2, end_s=3.0, seed=65, traced=True))
    f.append(_g("behind_a_batch_processor_and_a_conveyor", pools=[pc(SINK, 2, 0.1, cap=1)], buffers=[ib(SINK, 3, 1, 5, 0.3, so=SINK1)],
                flows=[bp(P0, 4, 0.05, 0.3), cv(B0, 0.15, 0)], servers=[], sources=[src(F0, 20.0, "poisson"), src(["flow", 1], 15.0, "poisson")],
                n_sinks=2, end_s=3.0, seed=66))
    f.append(_g("scheduled_requests_at_a_pool_and_a_buffer", pools=[pc(SINK, 1, 0.2)], buffers=[ib(SINK, 1, 0, 2, 0.25, so=SINK1)], servers=[],
                sources=[src(P0, 5.0, "constant")], schedule=plain(P0, 0.2, 0.2, 0.4) + plain(B0, 0.1, 0.1, 0.35, 0.35, 1.0), n_sinks=2, end_s=2.0,
                seed=67, traced=True))
    f.append(_g("auto_terminating_run_of_scheduled_requests", pools=[pc(B0, 1, 0.2)], buffers=[ib(SINK, 1, 1, 2, 0.5, so=SINK1)], servers=[],
                sources=[], schedule=plain(P0, 0.1, 0.1, 0.15, 0.3) + plain(B0, 0.1), n_sinks=2, end_s=0.0, auto=True, seed=68, traced=True))
    # ---- in front of a LoadBalancer: the Request a pool or a buffer forwards takes the LoadBalancer's completion hook like any other
    LB0 = ["lb", 0]
    f.append(_g("pool_in_front_of_a_load_balancer", pools=[pc(LB0, 2, 0.05, cap=3)], lbs=[MX.lb("round_robin", [0, 1])], servers=[srv(0.03), srv(0.05, cap=1)],
                sources=[src(P0, 30.0, "poisson")], faults=[crash(S1, 1.0, 1.8)], end_s=3.0, seed=70, traced=True))
    f.append(_g("stock_outs_go_to_a_load_balancer", buffers=[ib(SINK, 3, 1, 4, 0.4, so=LB0)], lbs=[MX.lb("least_conn", [0, 1, 2])],
                servers=[srv(0.04, out=SINK1), srv(0.06, out=SINK1), srv(0.05, out=SINK1)], sources=[src(B0, 30.0, "poisson")], n_sinks=2, end_s=3.0,
                seed=71, traced=True))
    f.append(_g("buffer_and_pool_in_front_of_a_weighted_load_balancer", buffers=[ib(P0, 6, 2, 6, THIRD, so=LB0)], pools=[pc(LB0, 1, 0.04)],
                lbs=[MX.lb("wrr", [0, 1])], servers=[srv(0.03, c=2), srv(0.04)], sources=[keyed(B0, 30.0)], end_s=3.0, seed=72))
    f.append(_g("probes_on_all_four_metrics", pools=[pc(SINK, 2, 0.15, cap=3)], buffers=[ib(P0, 4, 2, 6, 0.4, so=SINK1)], servers=[],
                sources=[src(B0, 25.0, "poisson")], probes=[[P0, "available", 0.1], [P0, "active", 0.1], [P0, "queued", 0.1], [B0, "stock", 0.1]],
                faults=[pause(P0, 1.5, 1.9)], n_sinks=2, end_s=3.0, seed=69, traced=True))
    by_name = {s["name"]: s for s in f}
    for base, windows in (("resent_request_loses_the_unit_to_an_arrival_of_its_nanosecond", [0.2, 0.2, 0.55, 1.0, 1.7]),
                          ("crashed_pool_restarts_with_a_line", [0.4, 0.8, 1.1, 1.5, 2.2]),
                          ("crash_over_a_replenish_leaves_the_order_pending", [0.3, 0.45, 0.9, 1.2, 2.5]),
                          ("buffer_pool_server_sink", [0.31, 0.9, 0.9, 1.75, 2.6])):
        f.append(dict(by_name[base], name=base + "_in_windows", traced=False, windows=windows))
    for s in f:
        s.setdefault("traced", False)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
# traced one-buffer cases in which the binary64 sum of seconds puts replenishments on another nanosecond than an integer addition would
ROUNDED = ("lead_time_a_tenth_from_30000_s", "lead_time_three_tenths_from_1e4_s", "lead_time_three_twentieths_from_1e5_s")
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """One chain Source(s) -> 2 .. 5 stations drawn from {Server, link, router, limiter, BatchProcessor, ConveyorBelt, pool, buffer} ->
    Sink, built from the Sink backwards, with 0 .. 2 faults over everything; the first station in front of the Sources is a pool or a
    buffer where the chain holds none yet.  Every third spec: constant Sources (arrivals that meet re-sent Requests and replenishments
    on their nanosecond); every fourth: a start time of 10^5 s."""
    rng = np.random.default_rng(977_000 + k)
    pools = {p: [] for p in ("server", "link", "router", "limiter", "flow", "pool", "buffer")}
    constant = k % 3 == 0
    end = float(rng.choice([2.0, 3.0]))

    def add(pool, item):
        pools[pool].append(item)
        return [pool, len(pools[pool]) - 1]

    def stock(to):
        if rng.random() < 0.5:
            return add("pool", pc(to if rng.random() < 0.9 else None, int(rng.integers(1, 4)), float(rng.choice([0.0, 0.05, 0.1, 0.2, THIRD])),
                                  int(rng.choice([0, 0, 1, 3]))))
        so = None if rng.random() < 0.3 else SINK if rng.random() < 0.5 else SINK1
        return add("buffer", ib(to, int(rng.integers(0, 8)), int(rng.integers(0, 6)), int(rng.integers(1, 9)),
                                float(rng.choice([0.0, 0.1, THIRD, 0.3, 0.7])), so=so))

    at = SINK
    n_stations = int(rng.integers(2, 6))
    for j in range(n_stations):
        r = int(rng.integers(0, 9))
        if j == n_stations - 1 and not pools["pool"] and not pools["buffer"]:
            r = 8
        if r == 0:
            at = add("server", srv(float(np.round(rng.uniform(0.01, 0.06), 3)), int(rng.integers(1, 3)), None if rng.random() < 0.6 else int(rng.integers(0, 3)), out=at))
        elif r == 1:
            at = add("link", link(at, float(rng.choice([0.02, 0.04])), *(("exp", 0.01) if rng.random() < 0.5 else (None, None)), float(rng.choice([0.0, 0.0, 0.2]))))
        elif r == 2:
            at = add("router", dict(targets=[at, SINK]))
        elif r == 3:
            at = add("limiter", dict(policy=list(RS.FOUR["token"]), cap=int(rng.choice([0, 1, 3])), out=at))
        elif r == 4:
            at = add("flow", bp(at, int(rng.integers(1, 5)), float(rng.choice([0.0, 0.05])), float(rng.choice([0.0, 0.1, 0.25]))))
        elif r == 5:
            at = add("flow", cv(at, float(rng.choice([0.0, 0.1])), int(rng.choice([0, 0, 3]))))
        else:
            at = stock(at)
    rate = float(rng.choice([5.0, 10.0])) if constant else float(np.round(rng.uniform(8.0, 30.0), 1))
    sources = [src(at, rate, "constant" if constant else "poisson") for _ in range(int(rng.integers(1, 4)) if constant else 1)]
    if k % 5 == 4:
        sources[0] = keyed(at, rate, sources[0]["kind"])
    sizes = dict({p: len(v) for p, v in pools.items()}, sink=2)
    names = [p for p in ("pool", "buffer", "pool", "buffer", "server", "link", "sink", "router", "limiter", "flow") if sizes[p]]
    faults = []
    for _ in range(int(rng.integers(0, 3))):
        pool = str(rng.choice(names))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        t0 = float(np.round(rng.uniform(0.0, end), 2))
        t1 = float(np.round(rng.uniform(t0, end * 1.05), 2))
        faults.append(pause(on, t0, t1) if rng.random() < 0.5 else crash(on, t0, None if rng.random() < 0.3 else t1))
    schedule = plain(at, *[float(x) for x in np.round(rng.uniform(0.0, end, size=2), 1)]) if k % 2 == 1 else []
    return _g(f"stock_graph_{k}", pools=pools["pool"], buffers=pools["buffer"], flows=pools["flow"], servers=pools["server"], links=pools["link"],
              routers=pools["router"], limiters=pools["limiter"], sources=sources, faults=faults, n_sinks=2, end_s=end, seed=int(rng.integers(1, 10_000)),
              **({"start_ns": START_1E5} if k % 4 == 3 else {}), **({"schedule": schedule} if schedule else {}))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups=6, name="stock_groups", end_s=2.0, wide=(44, 45)):
    """`n_groups` disconnected groups in ONE Simulation: Source -> buffer -> pool -> Server(s) -> Sink g, the stock-outs into the same
    Sink.  Group g < len(wide) runs through wide[g] Servers in a row: with 44 of them the group has 48 nodes, with 45 it has 49 --
    either side of the 48 node rows a side-by-side run keeps in LDS."""
    servers, pools, buffers, sources, faults = [], [], [], [], []
    for g in range(n_groups):
        first = len(servers)
        tandem = wide[g] if g < len(wide) else 1
        for j in range(tandem):
            servers.append(srv(0.004 + 0.001 * (g % 3), c=2, out=["sink", g] if j == tandem - 1 else ["server", first + j + 1]))
        pools.append(pc(["server", first], 1 + g % 3, 0.03 + 0.01 * (g % 4), cap=(0, 2, 4)[g % 3]))
        buffers.append(ib(["pool", g], 3 + g % 4, g % 3, 4 + g % 5, (0.1, THIRD, 0.25)[g % 3], so=["sink", g] if g % 2 else None))
        sources.append(src(["buffer", g], 12.0 + g % 5, "poisson"))
        if g % 3 == 2:
            faults.append(pause(["pool", g], 0.7 + 0.01 * g, 1.1 + 0.02 * g))
    return _g(name, pools=pools, buffers=buffers, servers=servers, sources=sources, n_sinks=n_groups, faults=faults, end_s=end_s, seed=73)


def group_sizes(spec):
    """The node counts of the parts the product splits the spec's graph into."""
    from happy_simulator_amd.graph_arrays import split_parts

    sim, _pools = build(spec)
    return [len(ids) for ids, _pos, _b in split_parts(sim.lowered().arrays)]


def growth_spec():
    """One unit with a cycle of one second and an unbounded line in front of 200 arrivals a second: the line holds some 400 Requests
    at the end (tests/test_gpu_stock.py grows heap, Request pool and record log from a capacity of one)."""
    return _g("line_of_400_requests_at_one_pool", pools=[pc(SINK, 1, 1.0)], buffers=[ib(P0, 50, 10, 100, 0.1, so=SINK1)], servers=[],
              sources=[src(B0, 200.0, "constant")], n_sinks=2, end_s=2.0, seed=83)


def recorded_specs():
    """Everything make_golden_stock.py records: the fixtures, the random chains, the groups and the growth case."""
    return all_specs() + [groups_spec(), growth_spec()]
