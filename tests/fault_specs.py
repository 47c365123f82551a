"""Specs for FaultSchedule with CrashNode / PauseNode, in the graph-spec format of tests/rate_limiter_specs.py with one more list:

  faults = [dict(kind="crash", on=<target>, at=<s>, restart=<s> | None, cancel=None | "before" | "after"),
            dict(kind="pause", on=<target>, at=<s>, end=<s>, cancel=...)]
      <target>: [pool, index] with pool in source / probe / server / link / router / lb / limiter / sink, or the entity's NAME
      as a string.  Times are absolute seconds, as the reference's faults take them (Instant.from_seconds, faults/node_faults.py:52).
      cancel="before": FaultHandle.cancel() before the Simulation is constructed (cancels nothing: the Events do not exist yet);
      "after": between construction and run() (the Events pop as cancelled).
  names = [[[pool, index], name]]: entities renamed after wiring (a duplicate name resolves to the last such object,
      faults/schedule.py:121-124).

tests/golden/make_golden_faults.py runs the LIVE reference on every spec listed here (tests/recorded.py FAULTS reads the recordings
back); tests/graph_family.py `build()` wires the product's objects the same way (its `wire()` is shared by both).

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs of rate_limiter_specs.random_spec with 1 .. 4 node faults over every entity kind
"""
import numpy as np

import rate_limiter_specs as RS

N_RANDOM = 120
POOLS = ("source", "probe", "server", "link", "router", "lb", "limiter", "sink")
GRID_SHARE = 3                 # every third random graph takes its fault times from the tick grid of a constant-rate Source


def _graph(name, *, servers, sources, n_sinks=1, links=(), routers=(), lbs=(), limiters=(), end_s=4.0, seed=7, **extra):
    return dict(name=name, topology="graph", n_sinks=n_sinks, servers=list(servers), links=list(links), routers=list(routers), lbs=list(lbs),
                limiters=list(limiters), sources=list(sources), end_s=end_s, seed=seed, **extra)


def _chain(name, faults, *, c=1, cap=None, kind="poisson", rate=14.0, svc="exp", mean=0.08, **extra):
    """Source -> Server -> Sink."""
    return _graph(name, servers=[dict(mean=mean, c=c, cap=cap, out=["sink", 0], svc=svc)], sources=[dict(kind=kind, rate=rate, to=0)],
                  faults=faults, **extra)


def crash(on, at, restart=None, cancel=None):
    return dict(kind="crash", on=on, at=at, restart=restart, cancel=cancel)


def pause(on, at, end, cancel=None):
    return dict(kind="pause", on=on, at=at, end=end, cancel=cancel)


def _lb(name, strategy, faults, seed):
    return _graph(name, servers=[dict(mean=0.12, c=1, cap=None, out=["sink", 0], svc="exp") for _ in range(3)],
                  lbs=[dict(strategy=strategy, backends=[0, 1, 2])], sources=[dict(kind="poisson", rate=20.0, to=["lb", 0])],
                  faults=faults, seed=seed)


def _fixtures():
    f = []
    # a Server crashed and restarted with work in service and in its queue
    for c in (1, 2):
        for cap in (None, 2):
            f.append(_chain(f"server_crash_c{c}_{'unbounded' if cap is None else 'bounded'}", [crash(["server", 0], 1.3, 2.6)], c=c, cap=cap,
                            rate=14.0 * c, seed=10 + len(f), traced=True))
    f.append(_chain("permanent_crash", [crash(["server", 0], 2.0)], seed=15))
    f.append(_chain("pause_sink", [pause(["sink", 0], 1.0, 2.5)], seed=16))
    f.append(_chain("source_crash_restart", [crash(["source", 0], 2.0, 4.0)], kind="poisson", rate=8.0, end_s=10.0, seed=17))
    f.append(_chain("probe_crash", [crash(["probe", 0], 1.1, 2.0)], seed=18,
                    probes=[[["server", 0], "depth", 0.25], [["sink", 0], "events_received", 0.5]]))
    f.append(_graph("link_crash_in_transit", servers=[dict(mean=0.03, c=1, cap=None, out=["sink", 0], svc="exp")],
                    links=[dict(lat=0.2, jk="exp", jm=0.05, loss=0.0, to=0)], sources=[dict(kind="poisson", rate=20.0, to=["link", 0])],
                    faults=[crash(["link", 0], 1.0, 2.0)], seed=19, traced=True))
    f.append(_graph("router_crash", n_sinks=2,
                    servers=[dict(mean=0.05, c=1, cap=None, out=["sink", 0], svc="exp"), dict(mean=0.04, c=1, cap=None, out=["sink", 0], svc="exp")],
                    routers=[dict(targets=[["server", 0], ["server", 1], ["sink", 1]])], sources=[dict(kind="poisson", rate=25.0, to=["router", 0])],
                    faults=[crash(["router", 0], 1.0, 1.5), pause(["server", 1], 2.0, 3.0)], seed=20))
    f.append(_lb("lb_crash_round_robin", "round_robin", [crash(["lb", 0], 1.0, 2.0)], 21))
    f.append(_lb("lb_crash_least_connections", "least_conn", [crash(["lb", 0], 1.0, 2.0)], 22))
    f.append(_lb("backend_crash_least_connections", "least_conn", [crash(["server", 1], 1.0, 2.5)], 23))
    for k, pol in RS.FOUR.items():
        # constant 10 / s against the policy: a poll is pending at 1.03 s (rate_limiter_specs.ISSUE_VALUES: every policy queues)
        f.append(dict(RS._chain(f"limiter_{k}_crash", pol, end_s=4.0, seed=24 + len(f)), faults=[crash(["limiter", 0], 1.03, 2.0)], traced=True))
    f.append(_chain("overlapping_crash_and_pause", [crash(["server", 0], 1.0, 3.0), pause(["server", 0], 2.0, 2.5)], seed=30))
    f.append(_graph("two_faults_two_entities", n_sinks=2,
                    servers=[dict(mean=0.05, c=1, cap=None, out=["sink", 0], svc="exp"), dict(mean=0.05, c=2, cap=3, out=["sink", 1], svc="exp")],
                    sources=[dict(kind="poisson", rate=12.0, to=0), dict(kind="poisson", rate=15.0, to=1)],
                    faults=[crash(["server", 0], 0.8, 1.9), pause(["sink", 1], 1.2, 3.1)], seed=31))
    f.append(_graph("duplicate_name", n_sinks=2,
                    servers=[dict(mean=0.05, c=1, cap=None, out=["sink", 0], svc="exp"), dict(mean=0.05, c=1, cap=None, out=["sink", 1], svc="exp")],
                    sources=[dict(kind="poisson", rate=12.0, to=0), dict(kind="poisson", rate=12.0, to=1)],
                    names=[[["server", 1], "srv0"]], faults=[crash("srv0", 1.0, 2.0)], seed=32))
    f.append(_chain("cancelled_before_construction", [crash(["server", 0], 1.0, 2.0, cancel="before")], seed=33))
    f.append(_chain("cancelled_after_construction", [crash(["server", 0], 1.0, 2.0, cancel="after"), pause(["sink", 0], 3.0, 3.5)], seed=34))
    f.append(_chain("fault_before_start", [crash(["server", 0], 2.0, 6.0), crash(["sink", 0], 6.5, 7.0)], start_ns=5 * 10 ** 9, seed=35))
    # Poisson(10): the first arrival beyond 3 s lies ~0.1 s out; the fault 10 us beyond the end is the one Event the loop still takes
    f.append(_chain("fault_is_the_event_beyond_the_end", [crash(["server", 0], 3.00001, 3.5)], rate=10.0, mean=0.02, end_s=3.0, seed=36))
    f.append(_chain("fault_later_than_the_event_beyond_the_end", [crash(["server", 0], 3.5)], rate=10.0, mean=0.02, end_s=3.0, seed=36))
    f.append(_graph("auto_terminate_pending_restart", servers=[dict(mean=0.1, c=1, cap=None, out=["sink", 0], svc="const")], sources=[],
                    end_s=0.0, auto=True, seed=37, schedule=[[["server", 0], t] for t in (0.0, 0.1, 0.2, 0.5)],
                    faults=[crash(["server", 0], 0.15, 100.0)]))
    # the two-counter case: lock-step constant Sources (ticks every 0.5 s), faults exactly on tick nanoseconds, schedule()d Requests
    # at the same instants
    f.append(_graph("lockstep_tick_grid", n_sinks=2,
                    servers=[dict(mean=0.1, c=1, cap=None, out=["sink", 0], svc="const"), dict(mean=0.1, c=1, cap=None, out=["sink", 1], svc="const")],
                    sources=[dict(kind="constant", rate=2.0, to=0), dict(kind="constant", rate=2.0, to=1)],
                    schedule=[[["server", 0], 2.0], [["server", 1], 2.0], [["server", 0], 3.0], [["sink", 1], 2.5], [["server", 1], 3.5]],
                    faults=[crash(["server", 0], 2.0, 3.0), crash(["source", 1], 2.5, 3.5), pause(["sink", 1], 3.0, 3.5)], end_s=5.0, seed=38,
                    traced=True))
    # more nodes than the loop keeps in LDS on ONE heap: 60 chains = 240 nodes, every third Server paused
    f.append(chains_spec(60, "nodes_beyond_lds", end_s=1.0))
    return {s["name"]: s for s in f}


def chains_spec(n, name, *, grid=False, end_s=2.0, kind="poisson"):
    """n disconnected Source -> limiter -> Server -> Sink chains, every third with a fault on its Server, limiter or Sink at a
    per-chain offset (grid=True: the first fault on a tick nanosecond of lock-step constant Sources instead)."""
    faults = []
    for j in range(0, n, 3):
        on = [("server", "limiter", "sink")[(j // 3) % 3], j]
        at = 0.5 if grid and j == 0 else 0.3 + 0.001 * (j % 700) + 0.0003
        faults.append(pause(on, at, at + 0.4) if (j // 3) % 2 else crash(on, at, at + 0.5 if j % 2 else None))
    return dict(name=name, topology="graph", n_sinks=n, links=[], routers=[], lbs=[], end_s=end_s, seed=11,
                servers=[dict(mean=0.03, c=1, cap=None, out=["sink", j], svc="exp") for j in range(n)],
                limiters=[dict(policy=list(RS.FOUR[RS.POLICIES[j % 4]]), cap=3, out=["server", j]) for j in range(n)],
                sources=[dict(kind=kind, rate=6.0 + (j % 3 if kind == "poisson" else 0), to=["limiter", j]) for j in range(n)], faults=faults)


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """rate_limiter_specs.random_spec(k) -- a general graph with Servers, links, routers, LoadBalancers, limiters, schedule()d
    Requests -- with 1 .. 4 node faults.  The first fault's entity kind is forced by `k` so that the cases cover every kind the graphs
    hold (make_golden_faults.py asserts it); every GRID_SHARE-th graph takes its times from the tick grid of a constant-rate Source (or
    of 0.1 s where it has none)."""
    spec = RS.random_spec(k)
    rng = np.random.default_rng(93_000 + k)
    spec["name"] = f"fault_graph_{k}"
    sizes = dict(source=len(spec["sources"]), probe=len(spec.get("probes") or []), server=len(spec["servers"]), link=len(spec["links"]),
                 router=len(spec["routers"]), lb=len(spec["lbs"]), limiter=len(spec["limiters"]), sink=spec["n_sinks"])
    pools = [p for p in POOLS if sizes[p]]
    end = float(spec["end_s"])
    const = [sc["rate"] for sc in spec["sources"] if sc["kind"] == "constant"]
    step = 1.0 / const[0] if const else 0.1
    grid = k % GRID_SHARE == 0

    def when(lo=0.0):
        if grid:
            return float(step * int(rng.integers(int(lo / step) + 1, max(int(end / step), int(lo / step) + 2) + 1)))
        return float(np.round(rng.uniform(lo, end * 1.05), 4))

    faults = spec["faults"] = []
    for j in range(int(rng.integers(1, 5))):
        want = POOLS[k % len(POOLS)]
        pool = want if j == 0 and want in pools else str(rng.choice(pools))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        at = when()
        if rng.random() < 0.5:
            faults.append(pause(on, at, when(at)))
        else:
            faults.append(crash(on, at, None if rng.random() < 0.3 else when(at)))
    return spec


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def fault_results(fs, targets):
    st = fs.stats
    return dict(crashed=np.array([bool(getattr(x, "_crashed", False)) for x in targets], np.int64),
                fault_stats=np.array([st.faults_scheduled, st.faults_activated, st.faults_deactivated, st.faults_cancelled], np.int64))
