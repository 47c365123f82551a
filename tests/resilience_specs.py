"""Specs for Bulkhead and TimeoutWrapper, in the graph-spec format of tests/fault_specs.py with one more list:

  wrappers = [dict(kind="bulkhead", to=<ref>, mc=<max_concurrent>, mq=<max_wait_queue>, mw=<max_wait_time | None>),
              dict(kind="timeout", to=<ref>, timeout=<s>)]
  every <ref> of the format may be ["wrapper", i]; faults and probes may name ["wrapper", i]; `checkers` / `unhealthy` as in
  tests/health_specs.py.

tests/golden/make_golden_resilience.py runs the LIVE reference on every spec listed here (tests/recorded.py RESILIENCE reads the
recordings back); tests/graph_family.py `build()` wires the product's objects the same way.  Entities: servers + lbs + routers + links + limiters + sinks +
wrappers + checkers.  Every case stays small: at most 20 s of simulated time at 100 Requests/s or less.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs over the same shapes

Two facts about the reference that the ties below record.  A `_bh_timeout` / `_tw_timeout` Event is constructed when the request is
queued / forwarded, the response Event only when the target's handler returns: on one nanosecond the timeout's index is always the
smaller one, so it is popped first.  That is also why a queued entry whose wait equals `max_wait_time` exactly has always been removed
by its timeout before a response could take it: `link_delay_equals_max_wait_time` is the run in which both meet, and the strict `>`
of `_try_process_queued` is seen by `expired_entries_skipped_after_a_wrapper_crash`, where the timeouts were dropped.
"""
import numpy as np

import fault_specs as FS
import happy_simulator_amd as hs
import health_specs as HS
import rate_limiter_specs as RS

N_RANDOM = 120
BOUND = hs.Bulkhead.MAX_CONCURRENT
crash, pause = FS.crash, FS.pause


def bh(to, mc, mq=0, mw=None):
    return dict(kind="bulkhead", to=to, mc=mc, mq=mq, mw=mw)


def tw(to, timeout):
    return dict(kind="timeout", to=to, timeout=timeout)


def srv(mean=0.05, c=1, cap=None, out=("sink", 0), svc="exp"):
    return dict(mean=mean, c=c, cap=cap, out=None if out is None else list(out), svc=svc)


def link(to, lat=0.05, jk=None, jm=None, loss=0.0):
    return dict(lat=lat, jk=jk, jm=jm, loss=loss, to=to)


def src(to, rate=20.0, kind="poisson"):
    return dict(kind=kind, rate=rate, to=to)


W0 = ["wrapper", 0]


def _g(name, wrappers, *, servers=(), sources=(), n_sinks=1, links=(), routers=(), lbs=(), limiters=(), faults=(), end_s=6.0, seed=7, **extra):
    return dict(name=name, topology="graph", n_sinks=n_sinks, servers=list(servers), links=list(links), routers=list(routers), lbs=list(lbs),
                limiters=list(limiters), sources=list(sources), wrappers=list(wrappers), faults=list(faults), end_s=end_s, seed=seed, **extra)


def _burst(name, wrapper, n_src=3, rate=4.0, mean=0.3, c=1, cap=None, schedule_at=(0.5, 0.5, 1.0, 2.25), **extra):
    """`n_src` constant Sources of one rate and schedule()d Requests on their tick nanoseconds -> wrapper -> Server -> Sink: a Server's
    hook fires with its enqueue, so only Requests of one nanosecond are in flight together."""
    return _g(name, [wrapper], servers=[srv(mean, c, cap, svc="const")], sources=[src(W0, rate, "constant") for _ in range(n_src)],
              schedule=[[W0, t] for t in schedule_at], **extra)


def _behind_link(name, wrapper, lk, rate=30.0, kind="poisson", mean=0.02, **extra):
    """Source -> wrapper -> NetworkLink -> Server -> Sink: the wrapper limits / times real in-flight work."""
    return _g(name, [wrapper], servers=[srv(mean)], links=[lk], sources=[src(W0, rate, kind)], **extra)


L0 = ["link", 0]


def _fixtures():
    f = []
    # ---- a Server as the target: same-nanosecond bursts
    f.append(_burst("bulkhead_server_burst", bh(0, 2, 2, 0.5), n_src=5, traced=True))
    f.append(_burst("bulkhead_server_burst_bounded_queue", bh(0, 3, 1, 0.25), n_src=6, cap=1, seed=11))
    f.append(_burst("timeout_server_burst", tw(0, 0.2), n_src=4, seed=12, traced=True))
    f.append(_burst("bulkhead_no_wait_queue", bh(0, 2, 0), n_src=4, seed=13))
    f.append(_burst("bulkhead_no_wait_time", bh(0, 1, 3, None), n_src=4, seed=14))
    for mc in (1, 63, 64, 65, BOUND):
        # 70 Sources of one rate: 70 Requests on every tick nanosecond, around the 63 / 64 / 65 permits
        f.append(_burst(f"bulkhead_max_concurrent_{mc}", bh(0, mc, 4, 0.5), n_src=70, rate=2.0, mean=0.001, c=8, end_s=2.0, seed=15 + len(f),
                        schedule_at=(0.5, 1.0)))
    # ---- the other targets whose handler returns at once
    f.append(_g("bulkhead_sink_target", [bh(["sink", 0], 1, 1, 0.5)], sources=[src(W0, 20.0), src(W0, 5.0, "constant")], seed=21))
    f.append(_g("bulkhead_router_target", [bh(["router", 0], 2, 2, 0.5)], servers=[srv(0.04), srv(0.06, out=("sink", 1))], n_sinks=2,
                routers=[dict(targets=[["server", 0], ["server", 1], ["sink", 1]])], sources=[src(W0, 25.0), src(W0, 25.0)], seed=22))
    for k, pol in RS.FOUR.items():
        f.append(_g(f"bulkhead_limiter_target_{k}", [bh(["limiter", 0], 2, 2, 0.5)], servers=[srv(0.03)],
                    limiters=[dict(policy=list(pol), cap=3, out=["server", 0])], sources=[src(W0, 10.0, "constant"), src(W0, 10.0, "constant")],
                    end_s=4.0, seed=23 + len(f)))
    f.append(_g("timeout_sink_router_limiter", [tw(["router", 0], 0.3), tw(["limiter", 0], 0.3), tw(["sink", 0], 0.3)],
                servers=[srv(0.04)], n_sinks=2, routers=[dict(targets=[["server", 0], ["sink", 1], ["wrapper", 1]])],
                limiters=[dict(policy=list(RS.FOUR["token"]), cap=2, out=["wrapper", 2])], sources=[src(W0, 30.0), src(["wrapper", 1], 12.0)], seed=28))
    # ---- in front of a NetworkLink
    f.append(_behind_link("bulkhead_link_constant", bh(L0, 3, 3, 0.5), link(0, 0.08), seed=31))
    f.append(_behind_link("bulkhead_link_jitter_out_of_order", bh(L0, 4, 3, 0.5), link(0, 0.02, "exp", 0.1), rate=40.0, seed=32, traced=True))
    f.append(_behind_link("bulkhead_link_twenty_requests", bh(L0, 4, 4, 0.5), link(0, 0.05), rate=10.0, kind="constant", end_s=2.0, seed=33))
    f.append(_behind_link("bulkhead_link_packet_loss", bh(L0, 2, 2, 0.5), link(0, 0.1, "exp", 0.05, loss=0.3), seed=34))
    f.append(_g("bulkhead_two_links", [bh(L0, 3, 2, 0.4)], servers=[srv(0.02)], links=[link(["link", 1], 0.04), link(0, 0.03, "exp", 0.02)],
                sources=[src(W0, 35.0)], seed=35))
    f.append(_behind_link("timeout_link_constant", tw(L0, 0.1), link(0, 0.08), seed=36))
    f.append(_behind_link("timeout_link_jitter", tw(L0, 0.12), link(0, 0.02, "exp", 0.1), rate=40.0, seed=37, traced=True))
    f.append(_behind_link("timeout_link_packet_loss", tw(L0, 0.2), link(0, 0.1, "exp", 0.05, loss=0.3), seed=38))
    f.append(_g("timeout_two_links", [tw(L0, 0.1)], servers=[srv(0.02)], links=[link(["link", 1], 0.04, loss=0.1), link(0, 0.03, "exp", 0.03)],
                sources=[src(W0, 35.0)], seed=39))
    f.append(_g("link_without_egress", [bh(L0, 2, 1, 0.3), tw(["link", 1], 0.05)], links=[link(None, 0.06), link(None, 0.06)],
                sources=[src(W0, 20.0), src(["wrapper", 1], 20.0)], n_sinks=1, seed=40))
    # ---- ties on one nanosecond
    f.append(_g("link_delay_equals_max_wait_time", [bh(L0, 1, 3, 0.25)], links=[link(["sink", 0], 0.25)],
                sources=[src(W0, 8.0, "constant"), src(W0, 8.0, "constant")], end_s=4.0, seed=41))
    f.append(_g("link_delay_equals_timeout", [tw(L0, 0.25)], links=[link(["sink", 0], 0.25)], sources=[src(W0, 8.0, "constant"), src(W0, 16.0)],
                end_s=4.0, seed=42))
    f.append(_g("link_delay_one_nanosecond_inside_and_outside", [tw(L0, 0.25), tw(["link", 1], 0.25)],
                links=[link(["sink", 0], 0.249999999), link(["sink", 0], 0.250000001)], sources=[src(W0, 9.0), src(["wrapper", 1], 9.0)], seed=43))
    # ---- faults on the target: permits leak, requests time out
    issue = _g("paused_server_leaks_permits", [bh(0, 4, 3, 0.5)], servers=[srv(0.02)], sources=[src(W0, 40.0)], faults=[pause(["server", 0], 2.0, 3.0)],
               end_s=10.0, seed=44)
    f.append(issue)
    f.append(_behind_link("crashed_server_behind_a_link", bh(L0, 4, 3, 0.5), link(0, 0.03), faults=[crash(["server", 0], 1.0, 2.0)], seed=45))
    f.append(_behind_link("crashed_link_target_no_restart", bh(L0, 6, 2, 0.3), link(0, 0.03), faults=[crash(["link", 0], 2.5)], seed=46))
    f.append(_g("timeout_target_paused_and_crashed", [tw(0, 0.2)], servers=[srv(0.03)], sources=[src(W0, 30.0)],
                faults=[pause(["server", 0], 1.0, 1.5), crash(["server", 0], 3.0, 4.2), crash(["sink", 0], 5.0)], seed=47))
    # ---- faults on the wrapper itself
    f.append(_behind_link("bulkhead_crash_with_restart", bh(L0, 2, 3, 0.4), link(0, 0.1, "exp", 0.05), faults=[crash(W0, 1.5, 3.0)], seed=48, traced=True))
    f.append(_behind_link("bulkhead_crash_without_restart", bh(L0, 2, 3, 0.4), link(0, 0.1), faults=[crash(W0, 2.0)], seed=49))
    f.append(_behind_link("bulkhead_pause", bh(L0, 2, 3, None), link(0, 0.1), faults=[pause(W0, 1.0, 1.2), pause(W0, 3.0, 3.05)], seed=50))
    # the timeouts of the queued entries are dropped while the wrapper is down; the responses that leaked with them never come: a later
    # Request cannot be forwarded, the entries wait -- until the permits' responses of Requests forwarded AFTER the restart skip them
    f.append(_behind_link("expired_entries_skipped_after_a_wrapper_crash", bh(L0, 3, 4, 0.2), link(0, 0.3), rate=40.0, mean=0.005,
                          faults=[crash(W0, 1.0, 1.25)], end_s=4.0, seed=51))
    f.append(_behind_link("timeout_wrapper_crash_with_restart", tw(L0, 0.3), link(0, 0.2, "exp", 0.1), faults=[crash(W0, 1.5, 3.0)], seed=52))
    # link delay 1.0 s, the wrapper down from 1.2 s to 1.9 s: the timeouts of the Requests of 0.9 .. 1.2 s are dropped, their responses
    # come after the restart and resolve them as successful
    f.append(_behind_link("timeout_response_after_the_wrappers_restart", tw(L0, 0.5), link(0, 1.0), rate=15.0, faults=[crash(W0, 1.2, 1.9)],
                          end_s=5.0, seed=53))
    f.append(_behind_link("timeout_wrapper_crash_without_restart", tw(L0, 0.3), link(0, 0.2), faults=[crash(W0, 2.0)], seed=54))
    f.append(_behind_link("cancelled_fault", bh(L0, 2, 3, 0.4), link(0, 0.1),
                          faults=[crash(W0, 1.5, 3.0, cancel="after"), pause(["server", 0], 2.0, 2.5, cancel="before"), pause(["link", 0], 4.0, 4.3)], seed=55))
    # ---- a wrapper behind a Server, a link, a router, a limiter and schedule()
    f.append(_g("wrappers_behind_a_server", [bh(["server", 1], 1, 2, 0.3), tw(["server", 1], 0.2)],
                servers=[srv(0.03, out=W0), srv(0.05), srv(0.02, out=["wrapper", 1])], sources=[src(0, 25.0), src(2, 10.0)], seed=56))
    f.append(_g("wrappers_behind_a_link", [bh(["link", 1], 2, 2, 0.3), tw(0, 0.2)], servers=[srv(0.03)],
                links=[link(W0, 0.04, "exp", 0.02), link(0, 0.06), link(["wrapper", 1], 0.01)], sources=[src(L0, 25.0), src(["link", 2], 10.0)], seed=57))
    f.append(_g("wrappers_behind_a_router", [bh(0, 1, 1, 0.3), tw(["sink", 1], 0.2)], servers=[srv(0.03)], n_sinks=2,
                routers=[dict(targets=[W0, ["wrapper", 1], ["sink", 0]])], sources=[src(["router", 0], 40.0)], seed=58))
    f.append(_g("wrappers_behind_a_limiter", [bh(L0, 2, 1, 0.3), tw(["link", 1], 0.05)], servers=[srv(0.03)],
                links=[link(0, 0.05), link(["sink", 0], 0.04, "exp", 0.02)],
                limiters=[dict(policy=list(RS.FOUR["token"]), cap=4, out=W0), dict(policy=list(RS.FOUR["sliding"]), cap=4, out=["wrapper", 1])],
                sources=[src(["limiter", 0], 20.0), src(["limiter", 1], 20.0)], seed=59))
    f.append(_g("scheduled_requests_until_the_heap_drains", [bh(L0, 2, 2, 0.3), tw(["link", 1], 0.15)], servers=[srv(0.05, svc="const")],
                links=[link(0, 0.1), link(0, 0.1, "exp", 0.08)], sources=[], end_s=0.0, auto=True, seed=60,
                schedule=[[W0, t] for t in (0.0, 0.0, 0.0, 0.05, 0.05, 0.2, 0.2, 0.2, 0.2, 0.2, 0.9)] + [[["wrapper", 1], t] for t in (0.0, 0.1, 0.1, 0.5)],
                traced=True))
    # ---- next to the other parts of the loop
    hc = _g("health_checker_elsewhere", [bh(L0, 3, 2, 0.4)], servers=[srv(0.04), srv(0.1), srv(0.1)], links=[link(0, 0.05)],
            lbs=[dict(strategy="round_robin", backends=[1, 2])], sources=[src(W0, 25.0), src(["lb", 0], 15.0)],
            faults=[crash(["server", 1], 1.3, 3.7)], checkers=[HS.checker(interval=0.5, timeout=0.2, ht=1, ut=2)], seed=61)
    f.append(hc)
    f.append(_g("probes_on_the_four_metrics", [bh(L0, 2, 3, 0.5), tw(["link", 1], 0.1)], servers=[srv(0.03)],
                links=[link(0, 0.1, "exp", 0.05), link(["sink", 0], 0.08, "exp", 0.05)], sources=[src(W0, 30.0), src(["wrapper", 1], 30.0)],
                probes=[[W0, "active_count", 0.1], [W0, "queue_depth", 0.1], [W0, "available_permits", 0.25], [["wrapper", 1], "in_flight_count", 0.1]],
                faults=[pause(["server", 0], 2.0, 2.6)], end_s=5.0, seed=62))
    f.append(_g("start_time_not_zero", [bh(L0, 2, 3, 0.5), tw(["link", 1], 0.1)], servers=[srv(0.03)],
                links=[link(0, 0.1), link(["sink", 0], 0.08, "exp", 0.05)], sources=[src(W0, 30.0), src(["wrapper", 1], 30.0)],
                faults=[crash(W0, 7.0, 8.0)], start_ns=5 * 10 ** 9, end_s=5.0, seed=63))
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """Source(s) -> [Server | link | router | limiter | nothing] -> wrapper -> [Server | Sink | router | limiter | link | two links]
    with 0 .. 2 faults over wrapper, target and links; every fourth spec holds a second, independent wrapper group."""
    rng = np.random.default_rng(96_000 + k)
    servers, links, routers, limiters, wrappers, sources, schedule = [], [], [], [], [], [], []
    n_sinks = 1

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
        if (k + _group) % 2 == 0:
            w = bh(to, int(rng.choice([1, 1, 2, 3, 5])), int(rng.choice([0, 1, 2, 4])), None if rng.random() < 0.2 else float(rng.choice([0.05, 0.125, 0.3, 0.5])))
        else:
            w = tw(to, float(rng.choice([0.02, 0.05, 0.1, 0.25])))
        at = add(wrappers, w, "wrapper")
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
        rate = float(rng.choice([5.0, 10.0, 20.0])) if kind == "constant" else float(np.round(rng.uniform(10.0, 60.0), 1))
        for _ in range(int(rng.integers(1, 4)) if kind == "constant" else 1):
            sources.append(src(at, rate, kind))
        if rng.random() < 0.3:
            schedule += [[["wrapper", len(wrappers) - 1], float(t)] for t in rng.choice([0.0, 0.5, 1.0, 1.5], size=3)]
    end = float(rng.choice([3.0, 4.0, 6.0]))
    sizes = dict(server=len(servers), link=len(links), wrapper=len(wrappers), sink=1, router=len(routers), limiter=len(limiters))
    pools = [p for p in ("wrapper", "wrapper", "server", "link", "sink", "router", "limiter") if sizes[p]]
    faults = []
    for _ in range(int(rng.integers(0, 3))):
        pool = str(rng.choice(pools))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        at = float(np.round(rng.uniform(0.0, end), 3))
        later = float(np.round(rng.uniform(at, end * 1.05), 3))
        faults.append(pause(on, at, later) if rng.random() < 0.5 else crash(on, at, None if rng.random() < 0.3 else later))
    return _g(f"resilience_graph_{k}", wrappers, servers=servers, links=links, routers=routers, limiters=limiters, sources=sources,
              n_sinks=n_sinks, faults=faults, end_s=end, seed=int(rng.integers(1, 10_000)), **({"schedule": schedule} if schedule else {}))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="groups", end_s=3.0, paused=True):
    """`n_groups` disconnected Source -> wrapper -> NetworkLink -> Server -> Sink groups in ONE Simulation (odd groups: a TimeoutWrapper),
    one Server paused per group: the parts of hs_graph_run_parts."""
    servers, links, wrappers, sources, faults = [], [], [], [], []
    for g in range(n_groups):
        servers.append(srv(0.02 + 0.005 * (g % 3), out=("sink", g)))
        links.append(link(g, 0.03 + 0.01 * (g % 4), "exp", 0.02))
        wrappers.append(tw(["link", g], 0.08) if g % 2 else bh(["link", g], 2 + g % 3, 2, 0.25))
        sources.append(src(["wrapper", g], 30.0 + g % 7))
        if paused:
            faults.append(pause(["server", g], 0.71 + 0.013 * g, 1.52 + 0.017 * g))
    return _g(name, wrappers, servers=servers, links=links, sources=sources, n_sinks=n_groups, faults=faults, end_s=end_s, seed=23)


def wrapper_results(pools):
    """What both libraries' wrappers show after a run.  wrap_stats rows -- Bulkhead: total, accepted, rejected, timed_out, queued,
    peak_concurrent, peak_queue_depth, active_count, queue_depth, available_permits, _next_request_id, len(_in_flight);
    TimeoutWrapper: total, successful, timed_out, in_flight_count, _next_request_id, zeros."""
    rows, live, loff, queue, qoff = [], [], [0], [], [0]
    for w in pools["wrapper"]:
        st = w.stats
        if hasattr(w, "max_concurrent"):
            rows.append([st.total_requests, st.accepted_requests, st.rejected_requests, st.timed_out_requests, st.queued_requests, st.peak_concurrent,
                         st.peak_queue_depth, w.active_count, w.queue_depth, w.available_permits, w._next_request_id, len(w._in_flight)])
            queue.extend(int(getattr(x, "request_id", x)) for x in w._wait_queue)
        else:
            rows.append([st.total_requests, st.successful_requests, st.timed_out_requests, w.in_flight_count, w._next_request_id] + [0] * 7)
        live.extend(sorted(int(i) for i in w._in_flight))
        loff.append(len(live))
        qoff.append(len(queue))
    return dict(wrap_stats=np.asarray(rows, np.int64).reshape(-1, 12), wrap_in_flight=np.asarray(live, np.int64), wrap_in_flight_off=np.asarray(loff, np.int64),
                wrap_queue=np.asarray(queue, np.int64), wrap_queue_off=np.asarray(qoff, np.int64))
