"""Specs for Client with timeouts and retry policies, in the graph-spec format of tests/resilience_specs.py with one more list:

  clients = [dict(to=<ref>, timeout=<s | None>, policy=None | ["fixed", max_attempts, delay] |
                  ["exp", max_attempts, initial_delay, max_delay, multiplier])]
  every <ref> of the format may be ["client", i]; faults and probes may name ["client", i].
  schedule = [[<ref>, t_s], ...] as before (a plain Event: no request_id) and, for a Client, [<ref>, t_s, mode]:
     "send"    client.send_request() with its time set to t_s;
     "again"   the Event object scheduled last, scheduled once more (its own time);
     "cancel"  a send_request() Event that is cancelled after it was scheduled (only behind every live one).

tests/golden/make_golden_client.py runs the LIVE reference on every spec listed here (tests/recorded.py CLIENT reads the recordings
back); tests/graph_family.py `build()` wires the product's objects the same way.  Entities: servers + lbs + routers + links + limiters + sinks + wrappers +
clients + checkers.  Every case stays small: 2 - 20 requests, or a few seconds of a Source of rate ~10.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs: the families of resilience_specs.random_spec with a Client where the wrapper stood

A `_client_timeout` Event is constructed with the request, the `_client_response` only when the target's handler returns: on one
nanosecond the timeout's index is the smaller one, so it pops first (`timeout_zero_sink`, `link_delay_equals_timeout`).
"""
import numpy as np

import fault_specs as FS
import health_specs as HS
import rate_limiter_specs as RS
import resilience_specs as XS

N_RANDOM = 120
crash, pause = FS.crash, FS.pause
srv, link, src, tw = XS.srv, XS.link, XS.src, XS.tw
C0, C1, L0 = ["client", 0], ["client", 1], ["link", 0]


def cl(to, timeout=None, policy=None):
    return dict(to=to, timeout=timeout, policy=None if policy is None else list(policy))


def fixed(n, delay):
    return ["fixed", n, delay]


def exp(n, initial, max_delay, multiplier=2.0):
    return ["exp", n, initial, max_delay, multiplier]


def make_policy(ns, pol):
    """The spec's policy from the namespace `ns` (the product or the reference's client package)."""
    if pol is None:
        return None
    if pol[0] == "fixed":
        return ns.FixedRetry(max_attempts=pol[1], delay=pol[2])
    return ns.ExponentialBackoff(max_attempts=pol[1], initial_delay=pol[2], max_delay=pol[3], multiplier=pol[4])


def _g(name, clients, *, wrappers=(), **kw):
    return XS._g(name, list(wrappers), clients=list(clients), **kw)


def send(on, *times):
    return [[on, t, "send"] for t in times]


def plain(on, *times):
    return [[on, t] for t in times]


def _fixtures():
    f = []
    tenth = [round(0.1 * k, 1) for k in range(10)]
    # ---- NoRetry, with and without a timeout
    f.append(_g("no_retry_no_timeout", [cl(0)], servers=[srv(0.03)], sources=[src(C0, 10.0)], end_s=3.0, seed=1))
    f.append(_g("no_retry_no_timeout_crashed_server", [cl(0)], servers=[srv(0.03)], sources=[src(C0, 10.0)], faults=[crash(["server", 0], 1.0, 2.0)],
                end_s=3.0, seed=2))
    f.append(_g("no_retry_timeout", [cl(0, 0.2)], servers=[srv(0.03)], sources=[src(C0, 10.0)], faults=[pause(["server", 0], 1.0, 1.6)], end_s=3.0, seed=3))
    f.append(_g("keyless_ten_plain_events", [cl(0, 0.5)], servers=[srv(0.01, svc="const")], faults=[pause(["server", 0], 0.25, 0.55)],
                schedule=plain(C0, *tenth), end_s=3.0, seed=4, traced=True))
    f.append(_g("fixed_retry_of_one_attempt", [cl(0, 0.2, fixed(1, 0.1))], servers=[srv(0.03)], sources=[src(C0, 10.0)],
                faults=[crash(["server", 0], 0.5, 1.5)], end_s=3.0, seed=5))
    # ---- timeout = 0: the timeout pops in front of the response
    f.append(_g("timeout_zero_sink", [cl(["sink", 0], 0, fixed(3, 0.0))], schedule=send(C0, 0.0, 0.1, 0.1, 0.2, 0.5), end_s=2.0, seed=6))
    f.append(_g("timeout_zero_server_no_retry", [cl(0, 0.0)], servers=[srv(0.02)], sources=[src(C0, 10.0, "constant")], end_s=1.0, seed=7))
    # ---- retries against a Server that is down
    down = dict(servers=[srv(0.02)], sources=[src(C0, 10.0)], end_s=4.0)
    f.append(_g("fixed_retry_crash_with_restart", [cl(0, 0.2, fixed(3, 0.3))], faults=[crash(["server", 0], 1.0, 1.7)], seed=8, traced=True, **down))
    f.append(_g("fixed_retry_crash_without_restart", [cl(0, 0.2, fixed(3, 0.3))], faults=[crash(["server", 0], 1.0)], seed=9, **down))
    f.append(_g("fixed_retry_pause", [cl(0, 0.15, fixed(4, 0.1))], faults=[pause(["server", 0], 1.0, 1.5), pause(["server", 0], 2.5, 2.55)], seed=10, **down))
    f.append(_g("exponential_backoff_crash_with_restart", [cl(0, 0.2, exp(4, 0.1, 1.0))], faults=[crash(["server", 0], 1.0, 1.9)], seed=11, **down))
    f.append(_g("exponential_backoff_crash_without_restart", [cl(0, 0.1, exp(6, 0.1, 1.0))], faults=[crash(["server", 0], 2.0)], seed=12,
                servers=[srv(0.02)], sources=[src(C0, 5.0)], end_s=6.0))
    f.append(_g("exponential_backoff_pause", [cl(0, 0.1, exp(5, 0.05, 0.4, 3.0))], faults=[pause(["server", 0], 1.0, 2.0)], seed=13, **down))
    f.append(_g("exponential_backoff_at_its_cap", [cl(0, 0.05, exp(6, 0.1, 0.25, 2.0))], faults=[pause(["server", 0], 0.5, 2.0)], seed=14,
                servers=[srv(0.02)], schedule=send(C0, 0.6, 0.7, 1.4), end_s=4.0))
    f.append(_g("integer_timeout_and_delay", [cl(0, 1, fixed(3, 1))], faults=[crash(["server", 0], 0.5, 2.2)], seed=15, servers=[srv(0.02)],
                schedule=send(C0, 0.0, 1.0, 1.0), end_s=8.0))
    # one request at 0.5 s, the Server down over [0.4, 1.0): attempts at 0.5, 0.95 and 1.4 -- the third lands after the restart
    f.append(_g("retry_lands_after_the_restart", [cl(0, 0.2, fixed(4, 0.25))], servers=[srv(0.01, svc="const")], faults=[crash(["server", 0], 0.4, 1.0)],
                schedule=send(C0, 0.5), end_s=3.0, seed=16, traced=True))
    # ---- behind a NetworkLink: the hook fires at the end of transit and again at the egress
    f.append(_g("link_double_response_twenty_requests", [cl(L0, 0.02, fixed(2, 0.05))], servers=[srv(0.01, svc="const")], links=[link(0, 0.03)],
                schedule=send(C0, *[round(0.1 * k, 1) for k in range(1, 21)]), end_s=5.0, seed=17))
    # attempt 1's response (0.3 s) arrives while attempt 2 (sent at 0.25 s) is in flight: a no-op; attempt 2 times out at 0.45 s, its
    # response at 0.55 s is a no-op too
    f.append(_g("late_response_of_attempt_one", [cl(L0, 0.2, fixed(2, 0.05))], links=[link(["sink", 0], 0.3)], schedule=send(C0, 0.0, 1.0) + plain(C0, 1.1),
                end_s=3.0, seed=18, traced=True))
    f.append(_g("late_responses_slow_link_source", [cl(L0, 0.1, fixed(3, 0.02))], servers=[srv(0.02)], links=[link(0, 0.15, "exp", 0.1)],
                sources=[src(C0, 8.0)], end_s=3.0, seed=19))
    f.append(_g("lossy_link", [cl(L0, 0.2, exp(3, 0.1, 0.5))], servers=[srv(0.02)], links=[link(0, 0.05, "exp", 0.05, loss=0.3)], sources=[src(C0, 10.0)],
                end_s=3.0, seed=20))
    f.append(_g("two_links", [cl(L0, 0.1, fixed(2, 0.1))], servers=[srv(0.02)], links=[link(["link", 1], 0.04, loss=0.1), link(0, 0.03, "exp", 0.03)],
                sources=[src(C0, 10.0)], end_s=3.0, seed=21))
    f.append(_g("link_without_egress", [cl(L0, 0.1, fixed(2, 0.1)), cl(["link", 1], 0.05)], links=[link(None, 0.06), link(None, 0.06)],
                sources=[src(C0, 10.0), src(C1, 10.0)], end_s=2.0, seed=22))
    # ---- ties on one nanosecond
    f.append(_g("link_delay_equals_timeout", [cl(L0, 0.25, fixed(2, 0.25))], links=[link(["sink", 0], 0.25)], sources=[src(C0, 8.0, "constant")],
                end_s=2.0, seed=23))
    f.append(_g("link_delay_one_nanosecond_inside_and_outside", [cl(L0, 0.25, fixed(2, 0.1)), cl(["link", 1], 0.25, fixed(2, 0.1))],
                links=[link(["sink", 0], 0.249999999), link(["sink", 0], 0.250000001)], sources=[src(C0, 9.0), src(C1, 9.0)], end_s=2.0, seed=24))
    # the retry of request 1 (0.2 + 0.3) and the timeout of request 2 (0.3 + 0.2) and a new request meet on 0.5 s
    f.append(_g("retry_timeout_and_request_on_one_nanosecond", [cl(0, 0.2, fixed(3, 0.3))], servers=[srv(0.01, svc="const")],
                faults=[pause(["server", 0], 0.0, 0.6)], schedule=send(C0, 0.0, 0.3, 0.5) + plain(C0, 0.5), end_s=3.0, seed=25))
    # ---- the other targets whose handler returns at once
    f.append(_g("sink_target", [cl(["sink", 0], 0.1, fixed(2, 0.1))], sources=[src(C0, 10.0)], faults=[pause(["sink", 0], 0.5, 1.0)], end_s=2.0, seed=26))
    f.append(_g("router_target", [cl(["router", 0], 0.1, fixed(3, 0.05))], servers=[srv(0.04), srv(0.06, out=("sink", 1))], n_sinks=2,
                routers=[dict(targets=[["server", 0], ["server", 1], ["sink", 1]])], sources=[src(C0, 12.0)], faults=[crash(["router", 0], 1.0, 1.4)],
                end_s=3.0, seed=27))
    for k, pol in RS.FOUR.items():
        f.append(_g(f"limiter_target_{k}", [cl(["limiter", 0], 0.1, fixed(2, 0.1))], servers=[srv(0.03)],
                    limiters=[dict(policy=list(pol), cap=3, out=["server", 0])], sources=[src(C0, 10.0, "constant")],
                    faults=[pause(["limiter", 0], 1.0, 1.5)], end_s=3.0, seed=28 + len(f)))
    f.append(_g("bounded_server_queue_refuses", [cl(0, 0.1, fixed(2, 0.1))], servers=[srv(0.3, cap=1, svc="const")],
                sources=[src(C0, 4.0, "constant") for _ in range(3)], end_s=2.0, seed=33))
    # ---- a Client behind a Server, a link, a router, a limiter
    f.append(_g("client_behind_a_server", [cl(1, 0.1, fixed(3, 0.1))], servers=[srv(0.03, out=C0), srv(0.02)], sources=[src(0, 10.0)],
                faults=[crash(["server", 1], 1.0, 1.5)], end_s=3.0, seed=34))
    f.append(_g("client_behind_a_link", [cl(0, 0.1, exp(3, 0.1, 0.3))], servers=[srv(0.03)], links=[link(C0, 0.04, "exp", 0.02)],
                sources=[src(L0, 10.0)], faults=[pause(["server", 0], 1.0, 1.5)], end_s=3.0, seed=35))
    f.append(_g("clients_behind_a_router_and_a_limiter", [cl(0, 0.1, fixed(2, 0.1)), cl(["sink", 1], 0.1)], servers=[srv(0.03)], n_sinks=2,
                routers=[dict(targets=[C0, ["limiter", 0], ["sink", 0]])], limiters=[dict(policy=list(RS.FOUR["token"]), cap=2, out=C1)],
                sources=[src(["router", 0], 20.0)], faults=[pause(["server", 0], 1.0, 1.4), pause(["sink", 1], 1.5, 2.0)], end_s=3.0, seed=36))
    # ---- where request ids come from: a Source, plain Events and send_request() on ONE Client
    f.append(_g("source_plain_and_send_request_mixed", [cl(L0, 0.12, fixed(3, 0.1))], servers=[srv(0.02)], links=[link(0, 0.05, "exp", 0.05)],
                sources=[src(C0, 10.0)], faults=[pause(["server", 0], 0.5, 1.2)],
                schedule=send(C0, 0.0, 0.4) + plain(C0, 0.4, 0.6) + send(C0, 0.6, 1.0) + plain(C0, 1.0), end_s=3.0, seed=37, traced=True))
    f.append(_g("source_driven_keyless_retries", [cl(0, 0.15, fixed(3, 0.1))], servers=[srv(0.02)], sources=[src(C0, 10.0, "constant"), src(C0, 7.0)],
                faults=[crash(["server", 0], 0.5, 1.5)], end_s=3.0, seed=38))
    f.append(_g("same_event_scheduled_twice", [cl(L0, 0.1, fixed(2, 0.1))], servers=[srv(0.02)], links=[link(0, 0.05)],
                schedule=send(C0, 0.1) + [[C0, 0.1, "again"]] + send(C0, 0.3) + plain(C0, 0.5) + [[C0, 0.5, "again"]],
                faults=[pause(["server", 0], 0.25, 0.45)], end_s=2.0, seed=39))
    f.append(_g("cancelled_scheduled_request", [cl(0, 0.1, fixed(2, 0.1))], servers=[srv(0.02)], faults=[pause(["server", 0], 0.15, 0.3)],
                schedule=send(C0, 0.1, 0.2) + plain(C0, 0.3) + [[C0, 0.25, "cancel"]], end_s=2.0, seed=40))
    f.append(_g("scheduled_requests_until_the_heap_drains", [cl(L0, 0.15, exp(4, 0.1, 0.5))], servers=[srv(0.05, svc="const")], links=[link(0, 0.1, "exp", 0.08)],
                faults=[crash(["server", 0], 0.1, 0.9)], schedule=send(C0, 0.0, 0.0, 0.05, 0.2, 0.2) + plain(C0, 0.2, 0.9), end_s=0.0, auto=True, seed=41,
                traced=True))
    # ---- faults on the Client itself: its retry and its timeout are dropped, the entries stay in flight
    f.append(_g("client_crash_with_restart", [cl(L0, 0.2, fixed(3, 0.2))], servers=[srv(0.02)], links=[link(0, 0.3)], sources=[src(C0, 10.0)],
                faults=[crash(C0, 1.0, 1.6), pause(["server", 0], 0.5, 2.0)], end_s=3.0, seed=42))
    f.append(_g("client_crash_without_restart", [cl(0, 0.2, fixed(3, 0.2))], servers=[srv(0.02)], sources=[src(C0, 10.0)],
                faults=[pause(["server", 0], 0.7, 2.0), crash(C0, 1.0)], schedule=send(C0, 0.7, 0.9, 0.95), end_s=3.0, seed=43))
    f.append(_g("client_pause_drops_responses", [cl(L0, None)], servers=[srv(0.02)], links=[link(0, 0.2)], sources=[src(C0, 10.0)],
                faults=[pause(C0, 1.0, 1.3)], end_s=3.0, seed=44))
    f.append(_g("cancelled_fault", [cl(0, 0.1, fixed(2, 0.1))], servers=[srv(0.02)], sources=[src(C0, 10.0)],
                faults=[crash(C0, 1.5, 3.0, cancel="after"), pause(["server", 0], 1.0, 1.5, cancel="before"), pause(["server", 0], 2.0, 2.3)],
                end_s=3.0, seed=45))
    # ---- next to the other parts of the loop
    f.append(_g("two_clients_on_one_server", [cl(0, 0.1, fixed(3, 0.1)), cl(0, 0.15, exp(3, 0.05, 0.2))], servers=[srv(0.04)],
                sources=[src(C0, 8.0), src(C1, 8.0)], schedule=send(C0, 0.5) + send(C1, 0.5), faults=[pause(["server", 0], 1.0, 1.5)], end_s=3.0, seed=46))
    f.append(_g("probe_on_in_flight_count", [cl(L0, 0.3, fixed(2, 0.1)), cl(["link", 1], None)], servers=[srv(0.03)],
                links=[link(0, 0.1, "exp", 0.05), link(["sink", 0], 0.08, "exp", 0.05)], sources=[src(C0, 10.0), src(C1, 10.0)],
                probes=[[C0, "in_flight_count", 0.1], [C1, "in_flight_count", 0.25]], faults=[pause(["server", 0], 1.0, 1.6), pause(["link", 1], 1.0, 1.2)],
                end_s=3.0, seed=47))
    f.append(_g("start_time_not_zero", [cl(L0, 0.15, fixed(3, 0.1))], servers=[srv(0.03)], links=[link(0, 0.1)], sources=[src(C0, 10.0)],
                schedule=send(C0, 0.5, 1.0), faults=[crash(["server", 0], 6.0, 6.5)], start_ns=5 * 10 ** 9, end_s=3.0, seed=48))
    f.append(_g("wrapper_and_checker_elsewhere", [cl(L0, 0.1, fixed(2, 0.1))], wrappers=[tw(["link", 1], 0.05)], servers=[srv(0.04), srv(0.1), srv(0.1)],
                links=[link(0, 0.05), link(["sink", 0], 0.04, "exp", 0.02)], lbs=[dict(strategy="round_robin", backends=[1, 2])],
                sources=[src(C0, 10.0), src(["lb", 0], 10.0), src(["wrapper", 0], 10.0)], faults=[crash(["server", 1], 1.3, 2.0), pause(["server", 0], 1.0, 1.4)],
                checkers=[HS.checker(interval=0.5, timeout=0.2, ht=1, ut=2)], end_s=3.0, seed=49))
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """Source(s) -> [Server | link | router | limiter | nothing] -> Client -> [Server | Sink | router | limiter | link | two links]
    with 0 .. 2 faults over Client, target and links; every fourth spec holds a second, independent Client group; some Clients
    also take send_request() and plain Events."""
    rng = np.random.default_rng(97_000 + k)
    servers, links, routers, limiters, clients, sources, schedule = [], [], [], [], [], [], []

    def add(pool, item, kind):
        pool.append(item)
        return [kind, len(pool) - 1]

    def target():
        r = int(rng.integers(0, 6))

        def server():
            servers.append(srv(float(np.round(rng.uniform(0.01, 0.08), 3)), int(rng.integers(1, 3)),
                               None if rng.random() < 0.6 else int(rng.integers(0, 3))))
            return len(servers) - 1

        if r == 0:
            return server()
        if r == 1:
            return ["sink", 0]
        if r == 2:
            return add(routers, dict(targets=[["sink", 0], server()]), "router")
        if r == 3:
            return add(limiters, dict(policy=RS._random_policy(rng), cap=int(rng.choice([0, 1, 3])), out=server()), "limiter")
        lk = link(server(), float(np.round(rng.uniform(0.01, 0.2), 3)), "exp" if rng.random() < 0.6 else None,
                  float(np.round(rng.uniform(0.01, 0.1), 3)), float(rng.choice([0.0, 0.0, 0.2])))
        if lk["jk"] is None:
            lk["jm"] = None
        at = add(links, lk, "link")
        if r == 5:
            at = add(links, link(at, float(np.round(rng.uniform(0.01, 0.05), 3))), "link")
        return at

    for _group in range(2 if k % 4 == 3 else 1):
        to = target()
        timeout = None if rng.random() < 0.1 else float(rng.choice([0.0, 0.02, 0.05, 0.1, 0.25]))
        p = int(rng.integers(0, 3))
        policy = (None if p == 0 else fixed(int(rng.integers(1, 5)), float(rng.choice([0.0, 0.05, 0.1, 0.3]))) if p == 1 else
                  exp(int(rng.integers(2, 6)), float(rng.choice([0.02, 0.05, 0.1])), float(rng.choice([0.1, 0.2, 0.5])), float(rng.choice([1.0, 2.0, 3.0]))))
        at = here = add(clients, cl(to, timeout, policy), "client")
        up = int(rng.integers(0, 5))
        if up == 1:
            servers.append(srv(0.01, 2, None, out=at))
            at = len(servers) - 1
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
        if rng.random() < 0.5:
            for t in rng.choice([0.0, 0.5, 1.0, 1.5], size=3):
                schedule.append([here, float(t), "send"] if rng.random() < 0.7 else [here, float(t)])
    end = float(rng.choice([2.0, 3.0, 4.0]))
    sizes = dict(server=len(servers), link=len(links), client=len(clients), sink=1, router=len(routers), limiter=len(limiters))
    pools = [p for p in ("client", "server", "server", "link", "sink", "router", "limiter") if sizes[p]]
    faults = []
    for _ in range(int(rng.integers(0, 3))):
        pool = str(rng.choice(pools))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        at = float(np.round(rng.uniform(0.0, end), 3))
        later = float(np.round(rng.uniform(at, end * 1.05), 3))
        faults.append(pause(on, at, later) if rng.random() < 0.5 else crash(on, at, None if rng.random() < 0.3 else later))
    return _g(f"client_graph_{k}", clients, servers=servers, links=links, routers=routers, limiters=limiters, sources=sources,
              faults=faults, end_s=end, seed=int(rng.integers(1, 10_000)), **({"schedule": schedule} if schedule else {}))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="client_groups", end_s=3.0):
    """`n_groups` disconnected Source -> Client -> NetworkLink -> Server -> Sink groups in ONE Simulation, one Server paused per
    group: the parts of hs_graph_run_parts."""
    servers, links, clients, sources, faults = [], [], [], [], []
    for g in range(n_groups):
        servers.append(srv(0.02 + 0.005 * (g % 3), out=("sink", g)))
        links.append(link(g, 0.03 + 0.01 * (g % 4), "exp", 0.02))
        clients.append(cl(["link", g], 0.08 + 0.01 * (g % 3), exp(4, 0.05, 0.4) if g % 2 else fixed(3, 0.1)))
        sources.append(src(["client", g], 10.0 + g % 7))
        faults.append(pause(["server", g], 0.71 + 0.013 * g, 1.52 + 0.017 * g))
    return _g(name, clients, servers=servers, links=links, sources=sources, n_sinks=n_groups, faults=faults, end_s=end_s, seed=23)


# recorded fixtures without a random draw whose heap drains before their end: what they compute does not depend on the stream indices
# or the end of the Simulation that holds them
UNION_MEMBERS = ("keyless_ten_plain_events", "timeout_zero_sink", "retry_lands_after_the_restart", "link_double_response_twenty_requests",
                 "late_response_of_attempt_one")

# ... and the two of them in which no schedule()d request meets a run-time Event on its nanosecond, three times over: six parts
UNION_PARTS = ("retry_lands_after_the_restart", "late_response_of_attempt_one") * 3


def union_spec(names, name="client_union"):
    """The fixtures `names` as the disconnected components of ONE spec (Servers, links, Clients and Sinks renumbered; their faults and
    scheduled requests with them) and [(member name, {pool: its first index in the union})]."""
    out = _g(name, [], end_s=max(FIXTURES[n]["end_s"] for n in names), seed=FIXTURES[names[0]]["seed"], schedule=[])
    pools = dict(server="servers", link="links", client="clients")
    members = []
    for n in names:
        m = FIXTURES[n]
        assert not (m["sources"] or m["routers"] or m["limiters"] or m["lbs"] or m["wrappers"] or m.get("probes") or m.get("auto") or m.get("start_ns"))
        off = dict({k: len(out[v]) for k, v in pools.items()}, sink=out["n_sinks"] if members else 0)

        def at(r):
            if r is None:
                return None
            return r + off["server"] if isinstance(r, int) else [r[0], r[1] + off[r[0]]]

        out["servers"] += [dict(sv, out=at(sv["out"])) for sv in m["servers"]]
        out["links"] += [dict(lk, to=at(lk["to"])) for lk in m["links"]]
        out["clients"] += [dict(c, to=at(c["to"])) for c in m["clients"]]
        out["faults"] += [dict(ft, on=at(ft["on"])) for ft in m["faults"]]
        out["schedule"] += [[at(on), t, *mode] for on, t, *mode in m.get("schedule") or []]
        out["n_sinks"] = off["sink"] + m["n_sinks"]
        members.append((n, off))
    return out, members


def client_results(pools):
    """What both libraries' Clients show after a run.  cl_stats rows: requests_sent, responses_received, timeouts, retries, failures,
    in_flight_count, _next_request_id; cl_keys: sorted (request_id or 0, attempt) rows of `_in_flight`; cl_response_times: the floats
    of `_response_times` in order."""
    rows, keys, koff, times, toff = [], [], [0], [], [0]
    for c in pools["client"]:
        st = c.stats
        rows.append([st.requests_sent, st.responses_received, st.timeouts, st.retries, st.failures, c.in_flight_count, c._next_request_id])
        keys.extend(sorted((int(rid or 0), int(att)) for rid, att in c._in_flight))
        koff.append(len(keys))
        times.extend(c._response_times)
        toff.append(len(times))
    return dict(cl_stats=np.asarray(rows, np.int64).reshape(-1, 7), cl_keys=np.asarray(keys, np.int64).reshape(-1, 2), cl_keys_off=np.asarray(koff, np.int64),
                cl_response_times=np.asarray(times, np.float64), cl_response_times_off=np.asarray(toff, np.int64))
