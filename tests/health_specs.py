"""Specs for HealthChecker and the LoadBalancer's health marks, in the graph-spec format of tests/fault_specs.py with two more lists:

  checkers = [dict(lb=<LoadBalancer index>, interval=<s>, timeout=<s>, ht=<healthy_threshold>, ut=<unhealthy_threshold>,
                   starts=<how often sim.schedule(checker.start()) is called, default 1>, stop=<stop() before run()>,
                   early=<start() is called before the Simulation exists>)]
  unhealthy = [[<LoadBalancer index>, <position among its backends>]]: LoadBalancer.mark_unhealthy before the run
  faults may name ["checker", i].

tests/golden/make_golden_health.py runs the LIVE reference on every spec listed here (tests/recorded.py HEALTH reads the
recordings back); tests/graph_family.py `build()` wires the product's objects the same way.  Entities: servers + lbs + routers + links + limiters +
sinks + checkers.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs: 1 .. 6 backends, the four lowered strategies, 0 .. 3 faults over backends, LoadBalancer and
                  checker, Poisson and constant Sources, small queue capacities -- written to stay inside the lowered set
"""
import numpy as np

import fault_specs as FS

N_RANDOM = 120
STRATEGIES = ("round_robin", "wrr", "least_conn", "wlc")
WEIGHTED = ("wrr", "wlc")
crash, pause = FS.crash, FS.pause


def checker(lb=0, interval=1.0, timeout=0.25, ht=2, ut=3, **extra):
    return dict(lb=lb, interval=interval, timeout=timeout, ht=ht, ut=ut, **extra)


def _pool(name, strategy, n_backends, *, faults=(), checkers=None, unhealthy=(), weights=None, rate=20.0, kind="poisson", mean=0.12, svc="exp",
          c=1, cap=None, end_s=12.0, seed=7, **extra):
    """Source -> LoadBalancer -> n Servers -> Sink, a checker on the LoadBalancer."""
    lb = dict(strategy=strategy, backends=list(range(n_backends)))
    if strategy in WEIGHTED:
        lb["weights"] = list(weights) if weights is not None else [1 + (j % 3) for j in range(n_backends)]
    return dict(name=name, topology="graph", n_sinks=1, links=[], routers=[], limiters=[], end_s=end_s, seed=seed,
                servers=[dict(mean=mean, c=c, cap=cap, out=["sink", 0], svc=svc) for _ in range(n_backends)], lbs=[lb],
                sources=[dict(kind=kind, rate=rate, to=["lb", 0])], faults=list(faults),
                checkers=[checker()] if checkers is None else list(checkers), unhealthy=[list(u) for u in unhealthy], **extra)


def _fixtures():
    f = []
    # backend count and thresholds: 1, 2 and 3 backends per strategy, thresholds 1/1 and 2/3; backend 0 crashes and restarts
    for strat in STRATEGIES:
        for nb in (1, 2, 3):
            for ht, ut in ((1, 1), (2, 3)):
                f.append(_pool(f"{strat}_{nb}_backends_thresholds_{ht}_{ut}", strat, nb, faults=[crash(["server", 0], 2.3, 6.7)],
                               checkers=[checker(ht=ht, ut=ut)], rate=10.0 * nb, seed=100 + len(f)))
    # the issue's run: 3 Servers, interval 1.0, timeout 0.25, CrashNode("s1", 3.3, restart_at=9.7), RoundRobin, 20 s
    f.append(_pool("crash_then_restart_of_one_backend", "round_robin", 3, faults=[crash(["server", 1], 3.3, 9.7)], end_s=20.0, seed=41,
                   traced=True))
    f.append(_pool("pause_of_one_backend", "least_conn", 3, faults=[pause(["server", 2], 2.2, 7.4)], seed=42))
    f.append(_pool("all_backends_down_then_one_back", "round_robin", 3, checkers=[checker(ht=1, ut=2)],
                   faults=[crash(["server", 0], 1.5), crash(["server", 1], 1.6, 6.2), crash(["server", 2], 1.7)], seed=43, traced=True))
    f.append(_pool("lb_crashed_while_marks_arrive", "wlc", 3, checkers=[checker(ht=1, ut=2)],
                   faults=[crash(["lb", 0], 2.5, 8.5), crash(["server", 0], 3.1, 6.1)], seed=44))
    f.append(_pool("checker_crash_with_restart", "round_robin", 3, checkers=[checker(ht=1, ut=1)],
                   faults=[crash(["checker", 0], 2.1, 5.0), crash(["server", 1], 1.5, 9.0)], seed=45, traced=True))
    f.append(_pool("checker_paused_over_a_cycle", "least_conn", 2, checkers=[checker(ht=1, ut=1)],
                   faults=[pause(["checker", 0], 2.9, 3.1), crash(["server", 0], 1.2, 1.9)], seed=46))
    # probe timing
    f.append(_pool("probe_meets_a_full_bounded_queue", "round_robin", 2, rate=60.0, mean=0.4, cap=1, faults=[], seed=47, end_s=8.0))
    f.append(_pool("response_then_its_stale_timeout", "round_robin", 2, faults=[], seed=48, end_s=6.0, traced=True))
    f.append(_pool("timeout_and_next_cycle_on_adjacent_nanoseconds", "round_robin", 2, checkers=[checker(timeout=0.999999999, ht=1, ut=2)],
                   faults=[crash(["server", 0], 1.5, 6.5)], seed=49))
    f.append(_pool("constant_ticks_on_the_cycle_nanoseconds", "least_conn", 3, kind="constant", rate=4.0, svc="const", mean=0.3,
                   checkers=[checker(interval=0.5, timeout=0.25, ht=1, ut=2)], faults=[crash(["server", 1], 2.0, 5.0)], seed=50, traced=True))
    # starting and stopping
    f.append(_pool("start_scheduled_twice", "round_robin", 3, checkers=[checker(starts=2)], faults=[crash(["server", 0], 2.3, 6.7)], seed=51))
    f.append(_pool("stop_before_run", "round_robin", 3, checkers=[checker(stop=True)], faults=[crash(["server", 0], 2.3, 6.7)], seed=52))
    f.append(_pool("start_time_not_zero", "wrr", 3, checkers=[checker(ht=1, ut=2)], faults=[crash(["server", 2], 7.3, 11.7)], start_ns=5 * 10 ** 9,
                   seed=53))
    f.append(_pool("start_called_before_the_simulation_exists", "round_robin", 2, checkers=[checker(early=True)],
                   faults=[crash(["server", 0], 2.3, 6.7)], seed=54))
    f.append(_pool("early_start_before_a_later_start_time", "round_robin", 2, checkers=[checker(early=True)],
                   faults=[crash(["server", 0], 7.3)], start_ns=5 * 10 ** 9, seed=55))
    f.append(_pool("checker_never_started", "least_conn", 2, checkers=[checker(starts=0)], faults=[crash(["server", 0], 2.3)], seed=56))
    for strat in STRATEGIES:
        f.append(_pool(f"mark_unhealthy_before_the_run_without_any_checker_{strat}", strat, 3, checkers=[], unhealthy=[[0, 1]], faults=[],
                       seed=57 + len(f), end_s=6.0))
    f.append(_pool("every_backend_marked_unhealthy_without_a_checker", "round_robin", 2, checkers=[], unhealthy=[[0, 0], [0, 1]], faults=[],
                   seed=64, end_s=3.0))
    f.append(_pool("marked_unhealthy_before_the_run_and_checked_back_in", "wrr", 3, checkers=[checker(ht=2, ut=3)], unhealthy=[[0, 0], [0, 2]],
                   faults=[], seed=65, end_s=8.0))
    # WeightedRoundRobin: unequal weights, the unhealthy backend is the heaviest
    f.append(_pool("weighted_round_robin_heaviest_backend_out", "wrr", 3, weights=[5, 1, 2], checkers=[checker(ht=1, ut=2)],
                   faults=[crash(["server", 0], 2.1, 7.2)], rate=30.0, mean=0.05, seed=66, traced=True))
    f.append(_pool("weighted_round_robin_two_out_at_different_times", "wrr", 4, weights=[3, 7, 2, 2], checkers=[checker(interval=0.5, timeout=0.2, ht=1, ut=1)],
                   faults=[crash(["server", 1], 1.3, 4.4), pause(["server", 3], 2.6, 6.1)], rate=30.0, mean=0.05, seed=67))
    # two LoadBalancers in one Simulation, one of them checked; the other keeps its hashed strategy (all of its backends stay healthy)
    two = _pool("checked_and_unchecked_load_balancers", "least_conn", 3, faults=[crash(["server", 1], 2.2, 6.6), crash(["server", 4], 3.0, 5.0)],
                seed=68)
    two["servers"] += [dict(mean=0.1, c=1, cap=None, out=["sink", 0], svc="exp") for _ in range(2)]
    two["lbs"].append(dict(strategy="ip_hash", backends=[3, 4]))
    two["sources"].append(dict(kind="poisson", rate=15.0, to=["lb", 1], n_clients=40))
    f.append(two)
    # 33, 65 and 130 backends: just over kCoopMinBackends, past one and two wavefront strides
    for nb in (33, 65, 130):
        for strat in ("least_conn", "wlc", "wrr"):
            out = [[0, q] for q in (0, 31, 32, 63, 64, nb - 1) if q < nb]
            # healthy_threshold 4: the slots marked unhealthy before the run stay out while traffic flows and return with the fourth
            # cycle, at 3 s (WIDE_OUT_UNTIL_S)
            f.append(_pool(f"{strat}_{nb}_backends", strat, nb, unhealthy=sorted(set(map(tuple, out))), checkers=[checker(ht=4, ut=2)],
                           weights=[1 + (j * 7) % 5 for j in range(nb)], faults=[crash(["server", 1], 1.2, 3.4), crash(["server", nb - 2], 0.7)],
                           rate=float(int(1.25 * nb / 0.8)), mean=0.8, end_s=5.0, seed=70 + len(f), wide=True))     # (more offered than served:
                                                                                                   # every backend is busy, a returning one is the minimum at once)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))
WIDE = sorted(n for n, s in FIXTURES.items() if s.get("wide"))


def wide_returning(spec):
    """The initially unhealthy slots of a wide fixture that no fault keeps down: they are marked healthy at WIDE_OUT_UNTIL_S."""
    down = {ft["on"][1] for ft in spec["faults"] if ft["on"][0] == "server"}
    return [q for _j, q in spec["unhealthy"] if q not in down]


WIDE_OUT_UNTIL_S = 3.0         # the wide fixtures' initially unhealthy slots are marked healthy by the cycle at this time


def random_spec(k):
    rng = np.random.default_rng(94_000 + k)
    nb = int(rng.integers(1, 7))
    strat = STRATEGIES[k % 4]
    end = float(rng.choice([4.0, 6.0, 8.0]))
    interval = float(rng.choice([0.25, 0.5, 1.0]))
    timeout = float(np.round(interval * rng.choice([0.2, 0.5, 0.9]), 6))
    kind = "constant" if k % 3 == 0 else "poisson"
    rate = float(rng.choice([4.0, 8.0, 10.0, 20.0])) if kind == "constant" else float(np.round(rng.uniform(5.0, 40.0), 2))
    spec = _pool(f"health_graph_{k}", strat, nb, rate=rate, kind=kind, mean=float(np.round(rng.uniform(0.02, 0.3), 3)),
                 svc="const" if rng.random() < 0.3 else "exp", c=int(rng.integers(1, 3)),
                 cap=None if rng.random() < 0.5 else int(rng.integers(0, 4)),
                 weights=[int(w) for w in rng.integers(1, 6, size=nb)],
                 checkers=[checker(interval=interval, timeout=timeout, ht=int(rng.integers(1, 4)), ut=int(rng.integers(1, 4)),
                                   starts=2 if rng.random() < 0.1 else 1)],
                 end_s=end, seed=int(rng.integers(1, 10_000)))
    if rng.random() < 0.25:                                # a second Source straight at one backend
        spec["sources"].append(dict(kind="poisson", rate=float(np.round(rng.uniform(2.0, 10.0), 2)), to=int(rng.integers(0, nb))))
    if rng.random() < 0.2:
        spec["unhealthy"] = [[0, int(rng.integers(0, nb))]]
    grid = k % 4 == 1                                      # fault times on the checker's own cycle grid
    for _ in range(int(rng.integers(0, 4))):
        r = rng.random()
        on = ["server", int(rng.integers(0, nb))] if r < 0.7 else ["lb", 0] if r < 0.85 else ["checker", 0]
        at = float(interval * int(rng.integers(1, int(end / interval)))) if grid else float(np.round(rng.uniform(0.0, end), 4))
        later = float(at + interval * int(rng.integers(1, 8))) if grid else float(np.round(rng.uniform(at, end * 1.05), 4))
        if rng.random() < 0.5:
            spec["faults"].append(pause(on, at, later))
        else:
            spec["faults"].append(crash(on, at, None if rng.random() < 0.3 else later))
    return spec


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="groups", end_s=4.0):
    """`n_groups` disconnected LoadBalancer groups in ONE Simulation, each with three Servers, its own Sink, its checker and one
    crash / restart of a backend: the parts of hs_graph_run_parts."""
    servers, lbs, sources, checkers, faults = [], [], [], [], []
    for g in range(n_groups):
        servers += [dict(mean=0.05 + 0.01 * (g % 3), c=1, cap=None, out=["sink", g], svc="exp") for _ in range(3)]
        strat = STRATEGIES[g % 4]
        lb = dict(strategy=strat, backends=[3 * g, 3 * g + 1, 3 * g + 2])
        if strat in WEIGHTED:
            lb["weights"] = [1 + g % 3, 2, 1]
        lbs.append(lb)
        sources.append(dict(kind="poisson", rate=18.0 + g % 5, to=["lb", g]))
        checkers.append(checker(lb=g, interval=0.5, timeout=0.2, ht=1, ut=2))
        faults.append(crash(["server", 3 * g + g % 3], 0.73 + 0.013 * g, 2.13 + 0.017 * g))     # (off the timeouts' own nanoseconds)
    return dict(name=name, topology="graph", n_sinks=n_groups, links=[], routers=[], limiters=[], end_s=end_s, seed=19, servers=servers, lbs=lbs,
                sources=sources, faults=faults, checkers=checkers, unhealthy=[])


def health_results(spec, pools):
    """What both libraries' LoadBalancers and checkers show after a run."""
    out = {}
    flags, off, marks, cw, present = [], [0], [], [], []
    for j, lb in enumerate(pools["lb"]):
        backs = [pools["server"][b] for b in spec["lbs"][j]["backends"]]
        flags.extend(int(lb.get_backend_info(b).is_healthy) for b in backs)
        off.append(len(flags))
        st = lb.stats
        marks.append([st.backends_marked_unhealthy, st.backends_marked_healthy, lb.healthy_count, len(lb.unhealthy_backends)])
        cur = getattr(lb.strategy, "_current_weights", None)
        cw.extend(int(cur.get(b.name, 0)) if cur is not None else 0 for b in backs)
        present.extend(int(cur is not None and b.name in cur) for b in backs)     # (no entry for a backend no select() ever saw)
    out["lb_healthy"], out["lb_healthy_off"] = np.asarray(flags, np.int64), np.asarray(off, np.int64)
    out["lb_marks"] = np.asarray(marks, np.int64).reshape(-1, 4)
    out["lb_current_weights"] = np.asarray(cw, np.int64)
    out["lb_current_weights_present"] = np.asarray(present, np.int64)
    stats, states, pend = [], [], []
    for ck, hc in zip(spec.get("checkers") or [], pools["checker"]):
        st = hc.stats
        stats.append([st.checks_performed, st.checks_passed, st.checks_failed, st.checks_timed_out, st.backends_marked_healthy,
                      st.backends_marked_unhealthy, int(hc.is_running), hc._next_check_id])
        for b in spec["lbs"][ck["lb"]]["backends"]:
            name = pools["server"][b].name
            s = hc.get_backend_state_by_name(name)
            states.append([-1] * 5 if s is None else [s.consecutive_successes, s.consecutive_failures,
                                                      -1 if s.last_check_time is None else int(s.last_check_time.nanoseconds),
                                                      -1 if s.last_check_passed is None else int(s.last_check_passed), int(s.is_checking)])
            pend.append(int(hc._pending_checks.get(name, 0)))
    out["checker_stats"] = np.asarray(stats, np.int64).reshape(-1, 8)
    out["checker_states"] = np.asarray(states, np.int64).reshape(-1, 5)
    out["checker_pending"] = np.asarray(pend, np.int64)
    return out
