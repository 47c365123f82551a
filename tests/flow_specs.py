"""Specs for BatchProcessor, ConveyorBelt and GateController, in the graph-spec format of tests/client_specs.py with one more list:

  flows = [dict(kind="batch", to=<ref>, n=<batch_size>, pt=<process_time>, ts=<timeout_s>),
           dict(kind="conveyor", to=<ref>, tt=<transit_time>, cap=<capacity>),
           dict(kind="gate", to=<ref>, sched=[[open_at_s, close_at_s], ...], open=<initially_open>, cap=<queue_capacity>)]
  every <ref> of the format may be ["flow", i]; faults and probes may name ["flow", i].
  schedule = [[<ref>, t_s], ...] as before (a plain Event) and [["flow", i], None, "gate"]: sim.schedule(ev) for every Event of the
     gate's start_events(), at that place of the call order.
  pre = [[["flow", i], "open" | "close"], ...]: GateController.open() / close() on the host before the Simulation is built.
  a Source may hold stop_s: stop_after, in seconds.

`wire`, `fault_targets` and `schedule_all` are tests/graph_family.py's; this family keeps its own `build` and `results`.
tests/golden/make_golden_flow.py runs the LIVE reference on every spec listed here through tests/golden/record_family.py
(tests/recorded.py-style store: FLOW below).  Entities: servers + lbs + routers + links + limiters + sinks + wrappers + clients +
flows + checkers -- node numbers in the recorded traces and the process-wide sort counter depend on that order and on the order of the
schedule() calls.  Every case stays small: a few seconds of a Source of rate ~10.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs: one or two chains of the three entities mixed with limiters, links, routers, LoadBalancers
                  and faults

A `_BatchTimeout` that finds an empty buffer is a processed no-op in the reference, but no run of the reference's own classes gets
there: the buffer is only ever emptied by `_process_batch`, which cancels the pending timeout in the same step.  Only a hand-made
`_BatchTimeout` Event could, and `Simulation.schedule()` refuses one by name; so there is no such fixture.
"""
import numpy as np

import fault_specs as FS
import graph_family as GF
import happy_simulator_amd as hs
import rate_limiter_specs as RS
import resilience_specs as XS
from recorded import Recorded

FLOW = Recorded("live_flow", "flow", "make_golden_flow.py", part_bytes=640 * 1024, max_part_bytes=900 * 1024)
N_RANDOM = 100
crash, pause = FS.crash, FS.pause
srv, link = XS.srv, XS.link
F0, F1, F2, F3 = (["flow", i] for i in range(4))
SINK = ["sink", 0]
# trace / by_kind kinds behind the Client's three (tests/golden/record_family.py EV): 31 .. 38
EV_FLOW = ("bp_item", "bp_timeout", "bp_cont", "cv_item", "cv_cont", "gt_item", "gt_open", "gt_close")
EV_FLOW_FIRST = 31


def src(to, rate=10.0, kind="constant", stop_s=None):
    return dict(kind=kind, rate=rate, to=to, **({} if stop_s is None else {"stop_s": stop_s}))


def bp(to, n=10, pt=1.0, ts=0.0):
    return dict(kind="batch", to=to, n=n, pt=pt, ts=ts)


def cv(to, tt, cap=0):
    return dict(kind="conveyor", to=to, tt=tt, cap=cap)


def gt(to, sched=None, open=True, cap=0):  # noqa: A002 -- the reference's argument is initially_open
    return dict(kind="gate", to=to, sched=[list(x) for x in sched or []], open=open, cap=cap)


def gate_events(i):
    return [["flow", i], None, "gate"]


def plain(on, *times):
    return [[on, t] for t in times]


def _g(name, flows, *, wrappers=(), **kw):
    return XS._g(name, list(wrappers), flows=list(flows), **kw)


make_flow = GF.make_flow


def wire(spec, F, ns):
    """graph_family.wire: the one wiring of every recorded family (a flow spec holds no checker)."""
    return GF.wire(spec, F, ns)


def fault_targets(pools):
    """graph_family.fault_targets: the flow entities stand behind the Clients."""
    return GF.fault_targets(pools)


def schedule_all(spec, pools, sim, event_cls, at):
    """graph_family.schedule_all: plain Requests and the gates' start_events()."""
    GF.schedule_all(spec, pools, sim, event_cls, at, GF.early_starts(spec, pools))


Product = GF.Product


def build(spec, seed=None, **sim_kw):
    """graph_family.build: (Simulation, entities by pool) of the product, wired like the recorded reference run."""
    return GF.build(spec, seed, **sim_kw)


def flow_results(pools):
    """What both libraries' flow entities show after a run.  flow_stats rows: BatchProcessor batches_processed, items_processed,
    timeouts, buffer_depth; ConveyorBelt items_transported, items_in_transit, items_rejected, has_capacity(); GateController
    passed_through, queued_while_closed, rejected, open_cycles, is_open, queue_depth."""
    rows = []
    for x in pools["flow"]:
        st = x.stats
        if hasattr(st, "batches_processed"):
            row = [st.batches_processed, st.items_processed, st.timeouts, x.buffer_depth]
            assert (x.batches_processed, x.items_processed, x.timeouts) == tuple(row[:3])
        elif hasattr(st, "items_transported"):
            row = [st.items_transported, st.items_in_transit, st.items_rejected, int(x.has_capacity())]
            assert (x.items_transported, x.items_in_transit, x.items_rejected) == tuple(row[:3])
        else:
            row = [st.passed_through, st.queued_while_closed, st.rejected, st.open_cycles, int(st.is_open), x.queue_depth]
            assert x.is_open == st.is_open
        rows.append(row + [0] * (6 - len(row)))
    return dict(flow_stats=np.asarray(rows, np.int64).reshape(-1, 6))


def results(spec, sim, pools):
    """Everything make_golden_flow.run_case records except the trace, read off the product's objects after run()."""
    out = GF.results(spec, sim, pools, "faults")
    out.update(FS.fault_results(pools["fault_schedule"], fault_targets(pools)))
    out.update(flow_results(pools))
    out["flow_by_kind"] = np.asarray(sim._flow_by_kind, np.int64)
    # health checks, wrappers and Clients: none in this family's specs, and the loop counted none of their Events
    out["other_by_kind"] = np.concatenate([np.asarray(getattr(sim, k, np.zeros(n)), np.int64) for k, n in
                                           (("_health_by_kind", 3), ("_resilience_by_kind", 6), ("_client_by_kind", 3))])
    return out


# what the engine has no counterpart for (the reference heap's length, the recorder's time-travel count) or what is compared in a form
# of its own (by_kind: the engine reports the public fifteen kinds, the internal ones per graph; trace: the tests that replay it)
NOT_COMPARED = {"trace", "by_kind", "pending_events", "time_travel"}
# the public kinds, the four internal ones, the twelve of health checks, wrappers and Client (zero in this family), the eight flow kinds
BY_KIND_SLICES = [("by_kind", 15), ("internal_by_kind", 19), ("other_by_kind", EV_FLOW_FIRST), ("flow_by_kind", EV_FLOW_FIRST + len(EV_FLOW))]


def compare(name, got, ref):
    """family_checks.compare with this family's set and slices."""
    import family_checks as FC

    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    """family_checks.engine over this family's build: the spec on a GraphEngine of its own (not yet run), with its faults and its
    scheduled Events, as Simulation.run() sets it up."""
    from happy_simulator_amd.graph_engine import GraphEngine

    sim, pools = build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, bool(spec.get("auto")))
    eng = GraphEngine(g.arrays, seed=spec["seed"], start_ns=start_ns, **caps)
    for node, t, on, c in sim._general_faults(g):
        eng.add_fault(node, t, on, c)
    for entry in sched:
        eng.schedule(*entry)
    return sim, pools, g, eng, end_ns, start_ns, cancelled


def engine_run(spec, ends_s, read=None, **caps):
    """engine(spec), run to every end of `ends_s` in turn (None: the spec's own end, Infinity included); the results bound like
    Simulation.run() binds them.  `read(eng, g)` is called before the engine is closed; (sim, pools, what it returned)."""
    sim, pools, g, eng, end_ns, start_ns, cancelled = engine(spec, **caps)
    with eng:
        for t in ends_s:
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
        extra = read(eng, g) if read else None
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    return sim, pools, extra


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _fixtures():
    f = []
    one = dict(servers=[srv(0.01, svc="const")], end_s=3.0)
    # ---- BatchProcessor
    f.append(_g("batch_size_one_no_timeout", [bp(SINK, 1, 0.1)], sources=[src(F0, 4.0)], end_s=3.0, seed=1))
    # the first item of an empty buffer returns the timeout alone: batch_size = 1 releases on the second item or on the timeout
    f.append(_g("batch_size_one_with_timeout", [bp(SINK, 1, 0.0, 0.5)], sources=[src(F0, 4.0, stop_s=1.0)], end_s=3.0, seed=2, traced=True))
    f.append(_g("batch_size_one_timeout_fires", [bp(SINK, 1, 0.05, 0.1)], sources=[src(F0, 4.0)], end_s=2.0, seed=3))
    # items at 0.1, 0.2, 0.3; the timeout of the first (0.1 + 0.2) lands on the nanosecond of the item that would fill the batch
    f.append(_g("timeout_on_the_filling_items_nanosecond_source", [bp(0, 3, 0.05, 0.2)], sources=[src(F0, 10.0)], seed=4, traced=True, **one))
    f.append(_g("timeout_on_the_filling_items_nanosecond_scheduled", [bp(0, 3, 0.05, 0.2)], schedule=plain(F0, 0.1, 0.2, 0.3, 0.3, 0.5, 0.7, 0.7, 0.7),
                seed=5, traced=True, **one))
    f.append(_g("two_batches_in_process", [bp(0, 2, 0.5)], sources=[src(F0, 10.0)], seed=6, traced=True, **one))
    f.append(_g("process_time_zero", [bp(0, 3, 0.0)], sources=[src(F0, 10.0)], seed=7, **one))
    f.append(_g("partial_batches_on_timeout", [bp(0, 5, 0.05, 0.15)], servers=[srv(0.02)], sources=[src(F0, 10.0, "poisson")], end_s=4.0, seed=8))
    f.append(_g("integer_times", [bp(SINK, 4, 1, 2)], sources=[src(F0, 1.0), src(F0, 2.0)], end_s=12.0, seed=9))
    f.append(_g("processor_behind_a_link", [bp(0, 4, 0.1, 0.3)], servers=[srv(0.02)], links=[link(F0, 0.05, "exp", 0.05)],
                sources=[src(["link", 0], 12.0, "poisson")], end_s=3.0, seed=10))
    # ---- ConveyorBelt
    f.append(_g("conveyor_transit_zero", [cv(0, 0.0, 1)], sources=[src(F0, 10.0), src(F0, 10.0)], seed=11, **one))
    f.append(_g("conveyor_unlimited", [cv(0, 0.25)], servers=[srv(0.03)], sources=[src(F0, 15.0, "poisson")], end_s=3.0, seed=12))
    f.append(_g("conveyor_at_capacity", [cv(SINK, 0.35, 3)], sources=[src(F0, 10.0)], end_s=3.0, seed=13))
    # a gate flushes 5 on one nanosecond into a conveyor of capacity 2: two go on, three are rejected
    f.append(_g("gate_flushes_five_into_a_conveyor_at_capacity", [gt(F1, [(1.0, 2.0)], False, 5), cv(SINK, 0.2, 2)], sources=[src(F0, 10.0)],
                schedule=[gate_events(0)], end_s=3.0, seed=14, traced=True))
    # ---- GateController
    f.append(_g("gate_opened_twice_closed_twice", [gt(0, [(1.0, 2.0), (1.5, 2.5)], True)], sources=[src(F0, 10.0)], schedule=[gate_events(0)],
                seed=15, **one))
    f.append(_g("gate_closed_while_closed", [gt(0, [(2.0, 1.0), (2.2, 2.1)], False)], sources=[src(F0, 10.0)], schedule=[gate_events(0)], seed=16, **one))
    f.append(_g("gate_flush_into_a_small_server_queue", [gt(0, [(1.0, 2.5)], False)], servers=[srv(0.05, cap=3, svc="const")], sources=[src(F0, 10.0)],
                schedule=[gate_events(0)], end_s=3.0, seed=17, traced=True))
    f.append(_g("gate_flush_into_a_load_balancer", [gt(["lb", 0], [(1.0, 1.5), (2.0, 2.2)], False, 8)], servers=[srv(0.04), srv(0.06), srv(0.05)],
                lbs=[dict(strategy="round_robin", backends=[0, 1, 2])], sources=[src(F0, 12.0, "poisson")], schedule=[gate_events(0)], end_s=3.0, seed=18))
    f.append(_g("gate_flush_into_least_connections", [gt(["lb", 0], [(1.0, 3.0)], False)], servers=[srv(0.2), srv(0.2)],
                lbs=[dict(strategy="least_conn", backends=[0, 1])], sources=[src(F0, 10.0)], schedule=[gate_events(0)], end_s=3.0, seed=19))
    f.append(_g("gate_into_gate", [gt(F1, [(1.0, 2.0)], False), gt(0, [(1.5, 2.5)], False, 7)], sources=[src(F0, 10.0)],
                schedule=[gate_events(1), gate_events(0)], seed=20, **one))
    f.append(_g("gate_without_events_queues_for_ever", [gt(0, None, False, 4)], sources=[src(F0, 10.0)], seed=21, **one))
    f.append(_g("gate_opened_and_closed_on_the_host", [gt(0, [(1.0, 2.0)], True), gt(0, [(0.5, 1.5)], False)], sources=[src(F0, 10.0), src(F1, 10.0)],
                pre=[[F0, "close"], [F0, "close"], [F1, "open"], [F1, "open"], [F1, "close"], [F1, "open"]], schedule=[gate_events(0), gate_events(1)],
                seed=22, **one))
    # schedule()d Requests on the nanosecond of a gate Event, constructed in front of it and behind it
    f.append(_g("scheduled_requests_on_a_gate_events_nanosecond", [gt(0, [(1.0, 2.0)], False)], schedule=plain(F0, 0.5, 1.0, 2.0) + [gate_events(0)] +
                plain(F0, 1.0, 1.0, 2.0, 2.5), seed=23, traced=True, **one))
    f.append(_g("auto_terminating_run", [gt(F1, [(0.5, 1.0), (3.0, 4.0)], False), bp(0, 3, 0.1, 0.4)], schedule=plain(F0, 0.1, 0.2, 0.3, 0.4, 0.6, 1.2, 1.3) +
                [gate_events(0)], servers=[srv(0.01, svc="const")], end_s=0.0, auto=True, seed=24, traced=True))
    # ---- the chain of the issue: Source 10 / s -> gate -> conveyor -> processor -> Server -> Sink
    f.append(_g("gate_conveyor_processor_chain", [gt(F1, [(1.0, 2.0), (3.0, 3.5)], False, 5), cv(F2, 0.2, 2), bp(0, 4, 0.05, 0.3)], sources=[src(F0, 10.0)],
                schedule=[gate_events(0)], servers=[srv(0.01, svc="const")], end_s=5.0, seed=25, traced=True))
    # ---- every upstream that may stand in front of one of the three
    f.append(_g("behind_server_router_and_limiter", [bp(["sink", 1], 3, 0.05, 0.2), cv(["sink", 1], 0.1, 2), gt(["sink", 1], [(0.5, 1.5)], False, 3)], n_sinks=2,
                servers=[srv(0.02, out=F0)], routers=[dict(targets=[F1, F2, ["sink", 0]])], limiters=[dict(policy=list(RS.FOUR["token"]), cap=3, out=F2)],
                sources=[src(0, 10.0, "poisson"), src(["router", 0], 20.0, "poisson"), src(["limiter", 0], 10.0)], schedule=[gate_events(2)], end_s=3.0, seed=26))
    f.append(_g("into_link_router_and_limiter", [bp(["link", 0], 3, 0.05, 0.2), cv(["router", 0], 0.1), gt(["limiter", 0], [(1.0, 2.0)], False)],
                servers=[srv(0.02)], links=[link(0, 0.05, "exp", 0.02, loss=0.1)], routers=[dict(targets=[0, SINK])],
                limiters=[dict(policy=list(RS.FOUR["leaky"]), cap=2, out=0)], sources=[src(F0, 10.0), src(F1, 10.0, "poisson"), src(F2, 10.0)],
                schedule=[gate_events(2)], end_s=3.0, seed=27))
    # ---- faults: what is aimed at a crashed or paused entity is dropped, what it holds goes on
    chain = dict(sources=[src(F0, 10.0)], servers=[srv(0.01, svc="const")], end_s=4.0)
    f.append(_g("processor_paused_timeout_dropped", [bp(0, 4, 0.05, 0.25)], faults=[pause(F0, 1.15, 1.45)], seed=28, traced=True, **chain))
    f.append(_g("processor_crashed_with_a_batch_in_process", [bp(0, 3, 0.4)], faults=[crash(F0, 1.0, 2.0)], seed=29, **chain))
    f.append(_g("processor_crashed_for_good", [bp(0, 3, 0.1, 0.5)], faults=[crash(F0, 1.55)], seed=30, **chain))
    f.append(_g("conveyor_crashed_with_items_in_transit", [cv(0, 0.35, 3)], faults=[crash(F0, 1.0, 1.8)], seed=31, **chain))
    f.append(_g("conveyor_paused", [cv(0, 0.1)], faults=[pause(F0, 1.0, 1.5), pause(["server", 0], 2.0, 2.3)], seed=32, **chain))
    f.append(_g("gate_paused_open_event_dropped", [gt(0, [(1.0, 2.0), (3.0, 3.5)], False, 6)], faults=[pause(F0, 0.95, 1.05)], schedule=[gate_events(0)],
                seed=33, traced=True, **chain))
    f.append(_g("gate_crashed_close_event_dropped", [gt(0, [(1.0, 2.0), (3.0, 3.5)], False)], faults=[crash(F0, 1.5, 2.5)], schedule=[gate_events(0)],
                seed=34, **chain))
    f.append(_g("cancelled_fault", [gt(F1, [(1.0, 2.0)], False, 5), bp(0, 3, 0.05, 0.2)], schedule=[gate_events(0)],
                faults=[crash(F1, 1.5, 3.0, cancel="after"), pause(F0, 0.5, 1.5, cancel="before"), pause(F1, 2.0, 2.3)], seed=35, **chain))
    # ---- a Probe on each metric
    f.append(_g("probes_on_the_three_metrics", [gt(F1, [(1.0, 2.0), (3.0, 3.5)], False, 5), cv(F2, 0.3, 4), bp(0, 4, 0.05, 0.6)], sources=[src(F0, 10.0, "poisson")],
                schedule=[gate_events(0)], servers=[srv(0.02)], probes=[[F0, "queue_depth", 0.1], [F1, "items_in_transit", 0.1], [F2, "buffer_depth", 0.25]],
                faults=[pause(F1, 1.2, 1.4)], end_s=4.0, seed=36))
    f.append(_g("start_time_not_zero", [gt(F1, [(6.0, 7.0)], False, 5), bp(0, 3, 0.05, 0.2)], sources=[src(F0, 10.0)], schedule=[gate_events(0)],
                servers=[srv(0.02)], faults=[pause(F1, 6.5, 6.8)], start_ns=5 * 10 ** 9, end_s=3.0, seed=37))
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """One or two chains Source(s) -> [Server | link | router | limiter | nothing] -> one to three of the three entities in a row ->
    [Server | Sink | link | router | limiter | LoadBalancer], with 0 .. 2 faults over everything."""
    rng = np.random.default_rng(131_000 + k)
    servers, links, routers, limiters, lbs, flows, sources, schedule = [], [], [], [], [], [], [], []

    def add(pool, item, kind):
        pool.append(item)
        return [kind, len(pool) - 1]

    def server(out=("sink", 0)):
        servers.append(srv(float(np.round(rng.uniform(0.01, 0.08), 3)), int(rng.integers(1, 3)), None if rng.random() < 0.6 else int(rng.integers(0, 3)), out=out))
        return len(servers) - 1

    def tail():
        r = int(rng.integers(0, 6))
        if r == 0:
            return server()
        if r == 1:
            return ["sink", 0]
        if r == 2:
            return add(links, link(server(), float(np.round(rng.uniform(0.01, 0.2), 3)), "exp", float(np.round(rng.uniform(0.01, 0.1), 3)),
                                   float(rng.choice([0.0, 0.0, 0.2]))), "link")
        if r == 3:
            return add(routers, dict(targets=[["sink", 0], server()]), "router")
        if r == 4:
            return add(limiters, dict(policy=RS._random_policy(rng), cap=int(rng.choice([0, 1, 3])), out=server()), "limiter")
        return add(lbs, dict(strategy=str(rng.choice(["round_robin", "least_conn"])), backends=[server(), server()]), "lb")

    for _chain in range(2 if k % 4 == 3 else 1):
        at = tail()
        for _ in range(int(rng.integers(1, 4))):
            r = int(rng.integers(0, 3))
            if r == 0:
                at = add(flows, bp(at, int(rng.integers(1, 7)), float(rng.choice([0.0, 0.05, 0.1, 0.3])), float(rng.choice([0.0, 0.0, 0.1, 0.25, 0.5]))), "flow")
            elif r == 1:
                at = add(flows, cv(at, float(rng.choice([0.0, 0.1, 0.2, 0.35])), int(rng.choice([0, 0, 1, 3]))), "flow")
            else:
                times = sorted(float(x) for x in np.round(rng.uniform(0.0, 3.0, size=2 * int(rng.integers(0, 3))), 1))
                at = add(flows, gt(at, [times[i:i + 2] for i in range(0, len(times), 2)], bool(rng.random() < 0.5), int(rng.choice([0, 0, 2, 5]))), "flow")
                if times:
                    schedule.append(gate_events(at[1]))
        up = int(rng.integers(0, 5))
        if up == 1:
            at = server(out=at)
        elif up == 2:
            at = add(links, link(at, 0.02, "exp", 0.01), "link")
        elif up == 3:
            at = add(routers, dict(targets=[at, ["sink", 0]]), "router")
        elif up == 4:
            at = add(limiters, dict(policy=RS._random_policy(rng), cap=3, out=at), "limiter")
        kind = "constant" if k % 3 == 0 else "poisson"
        rate = float(rng.choice([2.0, 5.0, 10.0])) if kind == "constant" else float(np.round(rng.uniform(4.0, 16.0), 1))
        for _ in range(int(rng.integers(1, 3)) if kind == "constant" else 1):
            sources.append(src(at, rate, kind))
        if rng.random() < 0.4 and flows:
            for t in rng.choice([0.0, 0.5, 1.0, 1.5], size=2):
                schedule.append([["flow", int(rng.integers(0, len(flows)))], float(t)])
    end = float(rng.choice([2.0, 3.0, 4.0]))
    sizes = dict(server=len(servers), link=len(links), flow=len(flows), sink=1, router=len(routers), limiter=len(limiters), lb=len(lbs))
    pools = [p for p in ("flow", "flow", "flow", "server", "link", "sink", "router", "limiter", "lb") if sizes[p]]
    faults = []
    for _ in range(int(rng.integers(0, 3))):
        pool = str(rng.choice(pools))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        at = float(np.round(rng.uniform(0.0, end), 3))
        later = float(np.round(rng.uniform(at, end * 1.05), 3))
        faults.append(pause(on, at, later) if rng.random() < 0.5 else crash(on, at, None if rng.random() < 0.3 else later))
    return _g(f"flow_graph_{k}", flows, servers=servers, links=links, routers=routers, limiters=limiters, lbs=lbs, sources=sources, faults=faults,
              end_s=end, seed=int(rng.integers(1, 10_000)), **({"schedule": schedule} if schedule else {}))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="flow_groups", end_s=3.0):
    """`n_groups` disconnected Source -> GateController -> ConveyorBelt -> BatchProcessor -> Server -> Sink groups in ONE Simulation:
    the parts of hs_graph_run_parts.  No two groups share a rate, so no two parts meet on a nanosecond with a pre-run Event."""
    servers, flows, sources, schedule = [], [], [], []
    for g in range(n_groups):
        servers.append(srv(0.02 + 0.005 * (g % 3), out=("sink", g)))
        flows += [gt(["flow", 3 * g + 1], [(0.5 + 0.01 * (g % 7), 1.5), (2.0, 2.5 + 0.01 * (g % 5))], False, 4 + g % 3),
                  cv(["flow", 3 * g + 2], 0.1 + 0.01 * (g % 4), 3 + g % 2), bp(g, 2 + g % 3, 0.05, 0.2 + 0.05 * (g % 2))]
        sources.append(src(["flow", 3 * g], 10.0 + g % 7, "poisson"))
        schedule.append(gate_events(3 * g))
    return _g(name, flows, servers=servers, sources=sources, n_sinks=n_groups, schedule=schedule, end_s=end_s, seed=29)


# ---- growth: the two cases of the issue ------------------------------------------------------------------------------------------------
def big_flush_spec():
    """A closed gate with 1 100 queued Requests opens: ONE handler constructs 1 100 Events.  The Requests come from a Source, one per
    millisecond, so the heap holds a handful of entries until then: a handle created with the smallest heap (1 024 entries + 4 per
    node) has to grow in front of that one Event, and the heap passes the 1 024 entries a side-by-side run keeps in LDS."""
    return _g("gate_flushes_1100", [gt(SINK, [(1.5, 1.8)], False)], sources=[src(F0, 1000.0, stop_s=1.1)], schedule=[gate_events(0)], end_s=2.0, seed=41)


def big_batch_spec():
    """Batches of 300 are released into a Server that serves 100 a second: some 2 000 Requests are alive at the end, a Request pool
    created with the smallest capacity (1 024 + 4 per node) grows while batches are in process."""
    return _g("batches_of_300", [bp(0, 300, 0.1)], servers=[srv(0.01, svc="const")], sources=[src(F0, 1000.0)], end_s=2.4, seed=42)


GROWTH = (big_flush_spec, big_batch_spec)
