"""Specs that mix the entity families of the single-heap loop in ONE connected graph: limiters, HealthCheckers, Bulkhead / TimeoutWrapper,
Clients and the three flow entities (BatchProcessor, ConveyorBelt, GateController), with faults over all of them.  The format is the
union of the families' (tests/graph_family.py), with one more schedule mode:

  schedule = [..., [["checker", i], None, "start"]]: sim.schedule(checker.start()) at that place of the call order (such a checker is
     listed with starts=0, so that nothing starts it a second time behind the list).

tests/golden/make_golden_mixed.py runs the LIVE reference on every spec listed here through tests/golden/record_family.py (family
"mixed": what the Client family records, plus the flow entities' section); MIXED below reads the recordings back.  Entities:
servers + lbs + routers + links + limiters + sinks + wrappers + clients + flows + checkers.  Every case is one connected graph (the
groups of `groups_spec` are the exception: the parts of hs_graph_run_parts), has at most 20 s of simulated time and at most 40 000
Events in the reference.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs: one or two chains Source(s) -> 2 .. 5 stations of every family -> Sink
  REFUSED         shapes the lowering refuses by name: {name: (spec, text of the refusal)}
"""
import numpy as np

import client_specs as CS
import fault_specs as FS
import flow_specs as FL
import graph_family as GF
import health_specs as HS
import rate_limiter_specs as RS
import resilience_specs as XS
from recorded import Recorded

MIXED = Recorded("live_mixed", "mixed", "make_golden_mixed.py", part_bytes=640 * 1024, max_part_bytes=900 * 1024)
N_RANDOM = 150
crash, pause = FS.crash, FS.pause
srv, link, bh, tw = XS.srv, XS.link, XS.bh, XS.tw
cl, fixed, exp, send = CS.cl, CS.fixed, CS.exp, CS.send
src, bp, cv, gt, gate_events, plain = FL.src, FL.bp, FL.cv, FL.gt, FL.gate_events, FL.plain
checker = HS.checker
F0, F1, F2 = FL.F0, FL.F1, FL.F2
C0, C1, W0, W1, L0, SINK = ["client", 0], ["client", 1], ["wrapper", 0], ["wrapper", 1], ["link", 0], ["sink", 0]
LB0, LIM0, R0 = ["lb", 0], ["limiter", 0], ["router", 0]
FAMILIES = ("limiter", "health", "wrapper", "client", "flow")
# the by_kind rows of each of the five (tests/golden/record_family.py EV)
FAMILY_KINDS = dict(limiter=(15, 17), health=(19, 22), wrapper=(22, 28), client=(28, 31), flow=(31, 39))


def start_checker(i=0):
    return [["checker", i], None, "start"]


def cancelled_send(on, t):
    return [on, t, "cancel"]


def lb(strategy, backends):
    out = dict(strategy=strategy, backends=list(backends))
    if strategy in HS.WEIGHTED:
        out["weights"] = [1 + (j % 3) for j in range(len(backends))]
    return out


def token(cap=3, out=0):
    return dict(policy=list(RS.FOUR["token"]), cap=cap, out=out)


def _g(name, *, flows=(), wrappers=(), clients=(), **kw):
    return FL._g(name, list(flows), wrappers=list(wrappers), clients=list(clients), **kw)


def families_of(ref):
    """The five families with a non-zero kind count in a recording."""
    return {f for f, (lo, hi) in FAMILY_KINDS.items() if ref["by_kind"][lo:hi].any()}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _fixtures():
    f = []
    open_twice = [(1.0, 1.5), (2.0, 2.5)]
    # ---- a flow entity in front of a hook holder: a flush puts N Requests on one nanosecond at a station that hands out ids or permits
    # (the Source's Requests hold no request_id: the Client's keys are (None, attempt), shared by every Request of the flush)
    f.append(_g("gate_flush_into_a_client_fixed_retry", flows=[gt(C0, open_twice, False)], clients=[cl(0, 0.05, fixed(3, 0.1))], servers=[srv(0.04)],
                sources=[src(F0, 10.0)], schedule=[gate_events(0)], end_s=3.0, seed=5, traced=True))
    f.append(_g("gate_flush_into_a_client_exponential_backoff", flows=[gt(C0, open_twice, False, 8)], clients=[cl(0, 0.03, exp(4, 0.05, 0.4))],
                servers=[srv(0.05, cap=2)], sources=[src(F0, 12.0, "poisson")], schedule=[gate_events(0)], end_s=3.0, seed=51))
    f.append(_g("gate_flush_into_a_small_bulkhead", flows=[gt(W0, [(1.0, 1.5)], False)], wrappers=[bh(0, 2, 3, 0.2)], servers=[srv(0.04)],
                sources=[src(F0, 10.0)], schedule=[gate_events(0)], end_s=3.0, seed=5, traced=True))
    f.append(_g("gate_flush_into_a_timeout_wrapper", flows=[gt(W0, open_twice, False)], wrappers=[tw(L0, 0.06)], servers=[srv(0.03)],
                links=[link(0, 0.02, "exp", 0.04)], sources=[src(F0, 10.0)], schedule=[gate_events(0)], end_s=3.0, seed=52))
    # the link's egress fires the wrapper's hook a second time
    f.append(_g("batch_into_a_timeout_wrapper_link_server", flows=[bp(W0, 5, 0.05, 0.3)], wrappers=[tw(L0, 0.08)], servers=[srv(0.04)],
                links=[link(0, 0.05, "exp", 0.03)], sources=[src(F0, 15.0, "poisson")], end_s=3.0, seed=7, traced=True))
    f.append(_g("conveyor_into_a_client", flows=[cv(C0, 0.2, 3)], clients=[cl(L0, 0.1, fixed(2, 0.05))], servers=[srv(0.03)], links=[link(0, 0.04, "exp", 0.05)],
                sources=[src(F0, 10.0), src(F0, 10.0)], end_s=3.0, seed=53))
    # ---- a hook holder, one handler, then a flow entity
    f.append(_g("client_server_batch_processor", flows=[bp(SINK, 4, 0.1, 0.25)], clients=[cl(0, 0.05, fixed(3, 0.1))], servers=[srv(0.04, out=F0)],
                sources=[src(C0, 12.0, "poisson")], end_s=3.0, seed=6, traced=True))
    f.append(_g("client_router_closed_gate", flows=[gt(0, [(1.5, 2.0)], False, 4)], clients=[cl(R0, 0.1, fixed(2, 0.1))], servers=[srv(0.03)],
                routers=[dict(targets=[F0, 0, SINK])], sources=[src(C0, 12.0, "poisson")], schedule=[gate_events(0)], end_s=3.0, seed=54))
    f.append(_g("bulkhead_limiter_conveyor_at_capacity", flows=[cv(SINK, 0.35, 2)], wrappers=[bh(LIM0, 2, 2, 0.3)], limiters=[token(3, F0)],
                sources=[src(W0, 10.0), src(W0, 10.0)], end_s=3.0, seed=55, traced=True))
    # the permit comes back with the Server's enqueue while the item waits in the gate
    f.append(_g("bulkhead_server_closed_gate", flows=[gt(SINK, [(2.0, 2.5)], False, 6)], wrappers=[bh(0, 2, 2, 0.3)], servers=[srv(0.05, out=F0)],
                sources=[src(W0, 10.0), src(W0, 5.0)], schedule=[gate_events(0)], end_s=3.0, seed=56))
    # ---- two hook holders in a row through a Server
    f.append(_g("client_server_client_server", clients=[cl(0, 0.08, fixed(3, 0.05)), cl(1, 0.05, exp(3, 0.05, 0.2))], servers=[srv(0.03, out=C1), srv(0.04)],
                sources=[src(C0, 12.0, "poisson")], faults=[pause(["server", 1], 1.0, 1.4), crash(["server", 0], 2.0, 2.3)], end_s=3.0, seed=57, traced=True))
    # the second Client reads the first one's metadata off the forwarded context: its request_id and its ATTEMPT -- a retry of the first
    # is a retry of the second, and an attempt the second one's policy no longer retries fails at its first timeout
    f.append(_g("retries_of_one_client_reach_a_second_with_fewer_attempts", clients=[cl(0, 0.05, fixed(4, 0.1)), cl(L0, 0.04, fixed(2, 0.02))],
                servers=[srv(0.02, out=C1), srv(0.03)], links=[link(1, 0.06)], sources=[src(C0, 10.0)], schedule=send(C0, 0.55, 0.6, 0.6),
                faults=[pause(["server", 0], 0.5, 0.85)], end_s=2.0, seed=75))
    f.append(_g("bulkhead_server_timeout_wrapper_server", wrappers=[bh(0, 2, 3, 0.25), tw(["link", 0], 0.05)], servers=[srv(0.03, out=W1), srv(0.04)],
                links=[link(1, 0.02, "exp", 0.03)], sources=[src(W0, 20.0, "poisson")], faults=[pause(["server", 1], 1.0, 1.3)], end_s=3.0, seed=58))
    # ---- a HealthChecker in the same connected graph: a flush of N on one nanosecond over a backend list that has just changed
    for k, strat in enumerate(HS.STRATEGIES):
        f.append(_g(f"gate_into_a_checked_load_balancer_{strat}", flows=[gt(LB0, [(1.0, 1.6), (2.5, 3.0)], False)], servers=[srv(0.05), srv(0.07), srv(0.06)],
                    lbs=[lb(strat, [0, 1, 2])], sources=[src(F0, 10.0)], schedule=[gate_events(0)], faults=[crash(["server", 0], 0.7, 2.2)],
                    checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=2)], end_s=4.0, seed=59 + k, traced=strat == "wrr"))
    f.append(_g("checked_backends_into_a_processor_a_client_and_a_bulkhead", flows=[bp(SINK, 3, 0.05, 0.2)], clients=[cl(3, 0.05, fixed(2, 0.1))],
                wrappers=[bh(L0, 1, 2, 0.2)], servers=[srv(0.04, out=F0), srv(0.05, out=C0), srv(0.03, out=W0), srv(0.04), srv(0.03)],
                links=[link(4, 0.03, "exp", 0.02)], lbs=[lb("round_robin", [0, 1, 2])], sources=[src(LB0, 20.0, "poisson")],
                faults=[crash(["server", 1], 1.2, 2.4), pause(["server", 3], 2.0, 2.5)], checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=2)],
                end_s=4.0, seed=63))
    # Client Requests and health probes share a bounded queue; probes are dropped
    f.append(_g("client_target_is_a_checked_bounded_backend", clients=[cl(0, 0.25, fixed(2, 0.1))], servers=[srv(0.3, cap=1, svc="const"), srv(0.05)],
                lbs=[lb("least_conn", [0, 1])], sources=[src(C0, 8.0), src(LB0, 6.0, "poisson")], checkers=[checker(interval=0.4, timeout=0.15, ht=1, ut=1)],
                end_s=4.0, seed=64, traced=True))
    f.append(_g("conveyor_limiter_checked_load_balancer", flows=[cv(LIM0, 0.15, 4)], limiters=[token(3, LB0)], servers=[srv(0.05), srv(0.06)],
                lbs=[lb("wlc", [0, 1])], sources=[src(F0, 14.0, "poisson")], faults=[crash(["server", 1], 1.1, 2.6)],
                checkers=[checker(interval=0.5, timeout=0.2, ht=2, ut=1)], end_s=4.0, seed=65))
    # ---- faults over the mix
    f.append(_g("paused_client_behind_an_opening_gate", flows=[gt(C0, [(1.0, 2.0)], False)], clients=[cl(0, 0.05, fixed(3, 0.1))], servers=[srv(0.03)],
                sources=[src(F0, 10.0)], schedule=[gate_events(0)], faults=[pause(C0, 0.9, 1.3)], end_s=3.0, seed=66, traced=True))
    f.append(_g("crashed_gate_in_front_of_a_bulkhead", flows=[gt(W0, [(1.0, 1.5), (2.5, 3.0)], False, 6)], wrappers=[bh(L0, 2, 3, 0.2)], servers=[srv(0.03)],
                links=[link(0, 0.05)], sources=[src(F0, 10.0)], schedule=[gate_events(0)], faults=[crash(F0, 1.2, 2.7)], end_s=4.0, seed=67))
    # the `_BatchTimeout` is dropped at the crashed processor; the Client's timeouts fire
    f.append(_g("crashed_processor_behind_a_clients_server", flows=[bp(SINK, 4, 0.1, 0.25)], clients=[cl(L0, 0.05, fixed(3, 0.1))], servers=[srv(0.04, out=F0)],
                links=[link(0, 0.02, "exp", 0.04)], sources=[src(C0, 12.0, "poisson")], faults=[crash(F0, 1.0, 2.0)], end_s=3.0, seed=68))
    f.append(_g("fault_on_the_checker_while_a_gate_is_closed", flows=[gt(LB0, [(2.0, 3.0)], False)], servers=[srv(0.05), srv(0.05)], lbs=[lb("round_robin", [0, 1])],
                sources=[src(F0, 10.0)], schedule=[gate_events(0)], faults=[pause(["checker", 0], 0.75, 1.75), crash(["server", 0], 0.6, 2.4)],
                checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=1)], end_s=4.0, seed=69))
    # ---- one schedule, four origins: send_request(), gate.start_events(), checker.start() and plain Requests share the pre-run sort counter
    four = dict(flows=[gt(C0, [(1.0, 2.0)], False)], clients=[cl(LIM0, 0.1, fixed(2, 0.25))], limiters=[token(2, 0)],
                servers=[srv(0.02, out=LB0, svc="const"), srv(0.05), srv(0.06)], lbs=[lb("round_robin", [1, 2])], end_s=4.0)
    f.append(_g("one_schedule_four_origins_on_a_gate_events_nanosecond", checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=1, starts=0)],
                schedule=send(C0, 0.5, 1.0) + plain(F0, 1.0, 1.0) + [gate_events(0)] + send(C0, 1.0) + [[C0, 1.0, "again"], start_checker()] +
                plain(C0, 1.0, 2.0) + plain(F0, 2.0) + send(C0, 2.0) + plain(LB0, 1.0) + [cancelled_send(C0, 1.0)],
                faults=[crash(["server", 1], 0.9, 2.1)], seed=70, traced=True, **four))
    f.append(_g("one_schedule_four_origins_on_a_checker_cycle_nanosecond", checkers=[checker(interval=0.5, timeout=0.25, ht=1, ut=1, early=True)],
                schedule=plain(F0, 0.5, 0.5) + send(C0, 0.5, 0.75) + [gate_events(0)] + plain(LB0, 0.5, 0.75, 1.5) + send(C0, 1.5) + [[C0, 1.5, "again"]] +
                plain(C0, 1.5), faults=[crash(["server", 2], 0.5, 1.5)], seed=71, traced=True, **four))
    # ---- a Probe on one metric of every family
    f.append(_g("probes_on_every_family", flows=[gt(F1, [(1.0, 2.0), (3.0, 3.5)], False, 6), cv(F2, 0.2, 4), bp(W0, 3, 0.05, 0.4)], wrappers=[bh(L0, 2, 3, 0.3), tw(2, 0.05)],
                clients=[cl(1, 0.1, fixed(2, 0.1))], limiters=[token(4, F0)], servers=[srv(0.03, out=C0), srv(0.04, out=W1), srv(0.02)], links=[link(0, 0.05, "exp", 0.03)],
                sources=[src(LIM0, 14.0, "poisson")], schedule=[gate_events(0)], faults=[pause(["server", 1], 2.2, 2.6)],
                probes=[[LIM0, "queue_depth", 0.1], [F0, "queue_depth", 0.1], [F2, "buffer_depth", 0.1], [F1, "items_in_transit", 0.1], [W0, "active_count", 0.1],
                        [W0, "available_permits", 0.25], [W1, "in_flight_count", 0.1], [C0, "in_flight_count", 0.1], [["server", 1], "depth", 0.1]],
                end_s=4.0, seed=72))
    # ---- an auto-terminating run that holds daemons of three families: a limiter's poll, gate Events, a stopped checker
    f.append(_g("auto_terminating_run_with_three_daemon_families", flows=[gt(LIM0, [(0.5, 1.0), (3.0, 4.0)], False)], limiters=[dict(policy=list(RS.FOUR["leaky"]), cap=4, out=LB0)],
                servers=[srv(0.05, svc="const"), srv(0.05, svc="const")], lbs=[lb("round_robin", [0, 1])], checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=1, stop=True)],
                schedule=plain(F0, 0.1, 0.2, 0.3, 0.4, 0.6, 0.6, 1.2) + [gate_events(0)], end_s=0.0, auto=True, seed=73, traced=True))
    # ---- events_cancelled from more than one family: BatchProcessor timeouts, a cancelled send_request() and a cancelled fault
    f.append(_g("cancelled_events_of_three_origins", flows=[bp(C0, 3, 0.05, 0.3)], clients=[cl(0, 0.1, fixed(2, 0.1))], servers=[srv(0.03)],
                sources=[src(F0, 10.0)], schedule=send(C0, 0.5) + [cancelled_send(C0, 1.0), cancelled_send(C0, 2.0)],
                faults=[crash(F0, 1.5, 2.5, cancel="after"), pause(["server", 0], 1.0, 1.3)], end_s=3.0, seed=74))
    # ---- Events that lie before the start of the Simulation: the reference pops and skips them (they count nowhere)
    f.append(_g("gate_events_and_an_early_checker_before_a_later_start_time", flows=[gt(LB0, [(1.0, 6.0), (7.0, 7.5)], False)], servers=[srv(0.05), srv(0.06)],
                lbs=[lb("round_robin", [0, 1])], sources=[src(F0, 10.0)], schedule=[gate_events(0)], faults=[crash(["server", 0], 5.6, 7.2)],
                checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=1, early=True)], start_ns=5 * 10 ** 9, end_s=3.0, seed=76))
    # ---- windows and start_ns variants
    by_name = {s["name"]: s for s in f}
    for base, extra in (("gate_flush_into_a_client_fixed_retry", dict(windows=[0.5, 1.0, 1.05, 1.5, 2.0, 2.75])),
                        ("gate_into_a_checked_load_balancer_least_conn", dict(windows=[0.5, 0.7, 1.0, 1.5, 2.2, 2.5, 2.5, 3.0])),
                        ("client_server_batch_processor", dict(windows=[0.3, 0.9, 0.9, 2.0, 2.6]))):
        f.append(dict(by_name[base], name=base + "_in_windows", traced=False, **extra))
    for base in ("gate_flush_into_a_small_bulkhead", "one_schedule_four_origins_on_a_gate_events_nanosecond", "crashed_processor_behind_a_clients_server"):
        s = dict(by_name[base], name=base + "_start_time_not_zero", traced=False, start_ns=5 * 10 ** 9)
        s["flows"] = [dict(fl, sched=[[a + 5.0, b + 5.0] for a, b in fl["sched"]]) if fl["kind"] == "gate" else fl for fl in s["flows"]]
        s["faults"] = [dict(ft, at=ft["at"] + 5.0, **({"restart": ft["restart"] + 5.0} if ft.get("restart") is not None else {}),
                            **({"end": ft["end"] + 5.0} if ft.get("end") is not None else {})) for ft in s["faults"]]
        f.append(s)
    for s in f:
        s.setdefault("traced", True)           # (every fixture but the variants above: a few hundred rows each)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))
REFUSED = {}


def _stations(rng, k, chain, pools, schedule, grid):
    """One chain's stations, built from the Sink backwards; the entry point of the chain."""
    servers, links, routers, limiters, lbs, wrappers, clients, flows, checkers = (pools[p] for p in (
        "server", "link", "router", "limiter", "lb", "wrapper", "client", "flow", "checker"))

    def add(pool, item, kind):
        pool.append(item)
        return [kind, len(pool) - 1]

    def server(out):
        servers.append(srv(float(np.round(rng.uniform(0.01, 0.08), 3)), int(rng.integers(1, 3)), None if rng.random() < 0.6 else int(rng.integers(0, 3)), out=out))
        return ["server", len(servers) - 1]

    at, hookable = ["sink", 0], True           # hookable: a Bulkhead, a TimeoutWrapper or a Client may stand in front of `at`
    for _ in range(int(rng.integers(2, 6))):
        while True:
            r = int(rng.integers(0, 11))
            if r in (4, 5, 6) and not hookable:
                continue                       # (refused by name: a hook on a flow entity, a LoadBalancer or another hook holder -- drawn again)
            break
        if r == 0:
            at, hookable = server(at), True
        elif r == 1:
            at = add(links, link(at, float(np.round(rng.uniform(0.01, 0.1), 3)), "exp", float(np.round(rng.uniform(0.01, 0.06), 3)), float(rng.choice([0.0, 0.0, 0.2]))), "link")
        elif r == 2:
            at, hookable = add(routers, dict(targets=[at, ["sink", 0]]), "router"), True
        elif r == 3:
            at, hookable = add(limiters, dict(policy=RS._random_policy(rng), cap=int(rng.choice([0, 1, 3])), out=at), "limiter"), True
        elif r == 4:
            pol = int(rng.integers(0, 3))
            policy = (None if pol == 0 else fixed(int(rng.integers(1, 4)), float(rng.choice([0.0, 0.05, 0.1]))) if pol == 1 else
                      exp(int(rng.integers(2, 5)), float(rng.choice([0.02, 0.05])), float(rng.choice([0.1, 0.2])), float(rng.choice([1.0, 2.0]))))
            at, hookable = add(clients, cl(at, None if rng.random() < 0.1 else float(rng.choice([0.0, 0.02, 0.05, 0.1])), policy), "client"), False
            if k % 2 == 1:
                for t in rng.choice(grid, size=2):
                    schedule.append([at, float(t), "send"] if rng.random() < 0.7 else [at, float(t)])
        elif r == 5:
            at, hookable = add(wrappers, bh(at, int(rng.choice([1, 2, 3])), int(rng.choice([0, 1, 2, 4])), None if rng.random() < 0.2 else float(rng.choice([0.05, 0.125, 0.3]))), "wrapper"), False
        elif r == 6:
            at, hookable = add(wrappers, tw(at, float(rng.choice([0.02, 0.05, 0.1]))), "wrapper"), False
        elif r == 7:
            at, hookable = add(flows, bp(at, int(rng.integers(1, 6)), float(rng.choice([0.0, 0.05, 0.1])), float(rng.choice([0.0, 0.1, 0.25]))), "flow"), False
        elif r == 8:
            at, hookable = add(flows, cv(at, float(rng.choice([0.0, 0.1, 0.2])), int(rng.choice([0, 0, 1, 3]))), "flow"), False
        elif r == 9:
            times = sorted(float(x) for x in rng.choice(grid, size=2 * int(rng.integers(1, 3))))
            at, hookable = add(flows, gt(at, [times[i:i + 2] for i in range(0, len(times), 2)], bool(rng.random() < 0.4), int(rng.choice([0, 0, 2, 5]))), "flow"), False
            schedule.append(gate_events(at[1]))
            if k % 2 == 1 and rng.random() < 0.5:
                schedule.append([at, float(rng.choice(grid))])
        else:
            backs = [server(at)[1] for _ in range(int(rng.integers(2, 4)))]
            at, hookable = add(lbs, lb(str(rng.choice(HS.STRATEGIES)), backs), "lb"), False
            if rng.random() < 0.6:
                late = k % 2 == 1 and rng.random() < 0.5
                checkers.append(checker(lb=at[1], interval=float(rng.choice([0.25, 0.5])), timeout=float(rng.choice([0.1, 0.2])), ht=int(rng.integers(1, 3)),
                                        ut=int(rng.integers(1, 3)), **({"starts": 0} if late else {"early": True} if rng.random() < 0.2 else {})))
                if late:
                    schedule.append(start_checker(len(checkers) - 1))
    return at


def random_spec(k):
    """One or two chains Source(s) -> 2 .. 5 stations drawn from {Server, link, router, limiter, Client, Bulkhead, TimeoutWrapper,
    BatchProcessor, ConveyorBelt, GateController, checked or unchecked LoadBalancer over two or three Servers} -> Sink, with 0 .. 3
    faults over everything, the checkers included.  What lower_general refuses by name (a hook holder in front of a flow entity, a
    LoadBalancer or another hook holder) is drawn again.  Every third spec: constant Sources, with fault and gate times on their tick
    grid; every second one carries a mixed schedule."""
    rng = np.random.default_rng(171_000 + k)
    pools = {p: [] for p in ("server", "link", "router", "limiter", "lb", "wrapper", "client", "flow", "checker")}
    sources, schedule = [], []
    constant = k % 3 == 0
    end = float(rng.choice([2.0, 3.0, 4.0]))
    grid = [0.5 * i for i in range(int(2 * end))] if constant else [float(x) for x in np.round(np.arange(0.0, end, 0.1), 1)]
    for chain in range(2 if k % 4 == 3 else 1):
        at = _stations(rng, k, chain, pools, schedule, grid)
        rate = float(rng.choice([2.0, 10.0])) if constant else float(np.round(rng.uniform(4.0, 16.0), 1))
        for _ in range(int(rng.integers(1, 3)) if constant else 1):
            sources.append(src(at, rate, "constant" if constant else "poisson"))
        if k % 2 == 1:
            schedule.append([at, float(rng.choice(grid))])
    sizes = dict({p: len(v) for p, v in pools.items()}, sink=1)
    names = [p for p in ("flow", "wrapper", "client", "server", "link", "sink", "router", "limiter", "lb", "checker", "checker") if sizes[p]]
    faults = []
    for _ in range(int(rng.integers(0, 4))):
        pool = str(rng.choice(names))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        at = float(rng.choice(grid)) if constant else float(np.round(rng.uniform(0.0, end), 3))
        later = float(rng.choice([g for g in grid if g >= at])) if constant else float(np.round(rng.uniform(at, end * 1.05), 3))
        faults.append(pause(on, at, later) if rng.random() < 0.5 else crash(on, at, None if rng.random() < 0.3 else later))
    rng.shuffle(schedule)                      # (the four origins interleaved in one call order)
    schedule = [list(e) for e in schedule]
    return _g(f"mixed_graph_{k}", flows=pools["flow"], wrappers=pools["wrapper"], clients=pools["client"], servers=pools["server"], links=pools["link"],
              routers=pools["router"], limiters=pools["limiter"], lbs=pools["lb"], sources=sources, faults=faults, end_s=end, seed=int(rng.integers(1, 10_000)),
              **({"checkers": pools["checker"]} if pools["checker"] else {}), **({"schedule": schedule} if schedule else {}),
              # every eighth spec starts at 2 s: gate Events, fault Events and early checker starts before that lie in the past
              **({"start_ns": 2 * 10 ** 9} if k % 8 == 5 else {}))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="mixed_groups", end_s=3.0, tandem=0):
    """`n_groups` disconnected groups in ONE Simulation, each a chain of four families: Source -> limiter -> GateController -> Client ->
    NetworkLink -> Server (downstream = Bulkhead) -> Server -> `tandem` more Servers -> Sink: the parts of hs_graph_run_parts, 9 + `tandem`
    nodes each."""
    servers, links, limiters, wrappers, clients, flows, sources, schedule, faults = [], [], [], [], [], [], [], [], []
    per = 2 + tandem
    for g in range(n_groups):
        first = per * g
        servers.append(srv(0.02 + 0.005 * (g % 3), out=["wrapper", g]))
        for j in range(1, per):
            servers.append(srv(0.01 + 0.005 * (g % 2), c=2, out=("sink", g) if j == per - 1 else ("server", first + j + 1)))
        wrappers.append(bh(first + 1, 1 + g % 3, 2, 0.25))
        links.append(link(first, 0.03 + 0.01 * (g % 4), "exp", 0.02))
        clients.append(cl(["link", g], 0.08 + 0.01 * (g % 3), exp(3, 0.05, 0.4) if g % 2 else fixed(3, 0.1)))
        flows.append(gt(["client", g], [(0.5 + 0.01 * (g % 7), 1.5), (2.0, 2.5 + 0.01 * (g % 5))], False, 4 + g % 3))
        limiters.append(dict(policy=list(RS.FOUR["token" if g % 2 else "sliding"]), cap=3, out=["flow", g]))
        sources.append(src(["limiter", g], 10.0 + g % 7, "poisson"))
        schedule.append(gate_events(g))
        faults.append(pause(["server", first], 0.71 + 0.013 * g, 1.12 + 0.017 * g))
    return _g(name, flows=flows, wrappers=wrappers, clients=clients, servers=servers, links=links, limiters=limiters, sources=sources, n_sinks=n_groups,
              schedule=schedule, faults=faults, end_s=end_s, seed=31)


def wide_groups_specs():
    """Two groups of 49 nodes and two of 48: around the 48 node rows a side-by-side run keeps in LDS (kLdsNodesBatch)."""
    return [groups_spec(2, name="mixed_groups_49_nodes", end_s=2.0, tandem=40), groups_spec(2, name="mixed_groups_48_nodes", end_s=2.0, tandem=39)]


# ---- growth: the two cases of the issue ------------------------------------------------------------------------------------------------
def big_flush_spec():
    """A closed gate with 1 100 queued Requests opens in front of a Bulkhead of 4 permits with a wait queue of 40: ONE handler constructs
    1 100 Events, of which 4 are forwarded, 40 wait and the others are rejected on that nanosecond."""
    return _g("gate_flushes_1100_into_a_bulkhead", flows=[gt(W0, [(1.5, 1.8)], False)], wrappers=[bh(L0, 4, 40, 0.1)], servers=[srv(0.002, svc="const")],
              links=[link(0, 0.01)], sources=[src(F0, 1000.0, stop_s=1.1)], schedule=[gate_events(0)], end_s=2.0, seed=41)


def retry_storm_spec():
    """A Client's retries against a backend that is down, behind a BatchProcessor: batches of 50 keyless Requests reach the Client on
    one nanosecond (they share the keys (None, attempt)), and 300 send_request() ids are each sent four times over a slow link to a
    crashed Server."""
    return _g("retry_storm_behind_a_batch_processor", flows=[bp(C0, 50, 0.05, 0.2)], clients=[cl(L0, 0.3, fixed(4, 0.2))], servers=[srv(0.01, svc="const")],
              links=[link(0, 0.4, "exp", 0.2)], sources=[src(F0, 400.0)], schedule=send(C0, *[round(0.35 + 0.005 * k, 3) for k in range(300)]), faults=[crash(["server", 0], 0.3, 2.6)],
              end_s=3.0, seed=42)


GROWTH = (big_flush_spec, retry_storm_spec)


def recorded_specs():
    """Everything make_golden_mixed.py records: the fixtures, the random graphs, the growth cases and the groups."""
    return all_specs() + [make() for make in GROWTH] + [groups_spec(32)] + wide_groups_specs()


def build(spec, seed=None, **sim_kw):
    return GF.build(spec, seed, **sim_kw)


class _WithInternal:
    """A Simulation with the four internal kinds filled in where the loop reported none."""

    def __init__(self, sim, internal):
        self._sim, self._internal_by_kind = sim, internal

    def __getattr__(self, key):
        return getattr(self._sim, key)


def results(spec, sim, pools):
    """Everything record_family.run_case records for "mixed" except the trace, read off the product's objects after run(): every
    family's result reader and all by_kind slices."""
    if not hasattr(sim, "_internal_by_kind"):
        # neither a fault nor an entity of the four later families: the loop reports the limiters' Events per limiter only
        ev = np.array([x._events for x in pools["limiter"]], np.int64).reshape(-1, 2)
        sim = _WithInternal(sim, np.array([ev[:, 0].sum(), ev[:, 1].sum(), 0, 0], np.int64))
    out = GF.results(spec, sim, pools, "resilience")
    out.update(CS.client_results(pools))
    for key, n in (("health_by_kind", 3), ("resilience_by_kind", 6), ("client_by_kind", 3)):       # (a spec may hold none of a family)
        out[key] = np.asarray(getattr(sim, "_" + key, np.zeros(n)), np.int64)
    out.update(FL.flow_results(pools))
    out["flow_by_kind"] = np.asarray(getattr(sim, "_flow_by_kind", np.zeros(len(FL.EV_FLOW))), np.int64)
    return out


# what the engine has no counterpart for (the reference heap's length, the recorder's time-travel count and its count of probes that a
# full queue refused) or what is compared in a form of its own (by_kind: the slices; trace: the tests that replay it)
NOT_COMPARED = {"trace", "by_kind", "pending_events", "time_travel", "probe_drops"}
BY_KIND_SLICES = [("by_kind", 15), ("internal_by_kind", 19), ("health_by_kind", 22), ("resilience_by_kind", 28), ("client_by_kind", 31),
                  ("flow_by_kind", FL.EV_FLOW_FIRST + len(FL.EV_FLOW))]


def compare(name, got, ref):
    """family_checks.compare with this family's set and slices."""
    import family_checks as FC

    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    import family_checks as FC

    return FC.engine(spec, **caps)


def engine_run(spec, ends_s, read=None, **caps):
    """flow_specs.engine_run (None: the spec's own end, Infinity included) over graph_family.build."""
    return FL.engine_run(spec, ends_s, read, **caps)
