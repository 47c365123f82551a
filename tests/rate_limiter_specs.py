"""Specs for RateLimitedEntity and its four policies, in the graph-spec format of tests/strategy_specs.py with one more pool:

  limiters = [dict(policy=[kind, *args], cap=<queue_capacity>, out=[pool, index])]
      kind "token" (capacity, refill_rate, initial_tokens | None), "leaky" (leak_rate), "sliding" (window_size_seconds, max_requests),
      "fixed" (requests_per_window, window_size)

and ["limiter", i] wherever a Request can be aimed: a Source's `to`, a Server's `out`, a link's `to`, a router target, a schedule()
target, another limiter's `out`.  `auto=True`: no end time (the run ends when only daemon events are pending); `windows`: the
reference driven by `_run_window` with these ends before `end_s`; `start_ns`: Simulation(start_time=).
tests/golden/make_golden_rate_limiter.py runs the LIVE reference on every spec listed here and records what it computed
(tests/recorded.py RATE_LIMITER reads it back); tests/graph_family.py `build()` wires the product's objects the same way (its `wire()`
is shared by both).

  FIXTURES        named cases, recorded with their full event trace
  random_spec(k)  N_RANDOM seeded general graphs (random_specs.graph_spec / lb_graph_spec) with limiters put on their edges
  POLICY_CALLS    call sequences for the host-Python policy classes
  guard_spec      the seeded search for a run that meets a policy's `wait == Duration.ZERO -> Duration(1)` guard
"""
import numpy as np

import happy_simulator_amd as hs
from random_specs import graph_spec, lb_graph_spec

POLICIES = ("token", "leaky", "sliding", "fixed")
UPSTREAMS = ("source", "server", "link", "router", "schedule", "limiter")
N_RANDOM = 120
GUARD_TRIES = 10_000


def make_policy(ns, pol):
    """The policy object of `pol` = [kind, *args] from the namespace `ns` (the product's or the reference's classes)."""
    kind, args = pol[0], list(pol[1:])
    if kind == "token":
        return ns.TokenBucketPolicy(args[0], args[1], args[2] if len(args) > 2 else None)
    if kind == "leaky":
        return ns.LeakyBucketPolicy(args[0])
    if kind == "sliding":
        return ns.SlidingWindowPolicy(args[0], int(args[1]))
    return ns.FixedWindowPolicy(int(args[0]), args[1])


def _chain(name, policy, *, source="constant", rate=10.0, cap=4, svc="const", mean=0.05, end_s=5.0, seed=7, **extra):
    """Source -> limiter -> Server -> Sink."""
    return dict(name=name, topology="graph", n_sinks=1, servers=[dict(mean=mean, c=1, cap=None, out=["sink", 0], svc=svc)], links=[],
                routers=[], lbs=[], limiters=[dict(policy=policy, cap=cap, out=["server", 0])],
                sources=[dict(kind=source, rate=rate, to=["limiter", 0])], end_s=end_s, seed=seed, **extra)


FOUR = dict(token=["token", 3, 5.0], leaky=["leaky", 4.0], fixed=["fixed", 3, 0.5], sliding=["sliding", 0.5, 3])
# (received, forwarded, queued, dropped, events) of the four deterministic fixtures, as the issue states them
ISSUE_VALUES = dict(token=(50, 27, 26, 19, 341), leaky=(50, 20, 23, 26, 280), fixed=(50, 33, 29, 16, 342), sliding=(50, 30, 31, 16, 395))


def _fixtures():
    f = []
    for k, pol in FOUR.items():
        f.append(_chain(f"{k}_constant", pol))
        f.append(_chain(f"{k}_poisson", pol, source="poisson", rate=11.0, svc="exp", mean=0.06, seed=20 + len(f)))
    f += [
        _chain("token_queue_capacity_0", ["token", 2, 4.0], cap=0, source="poisson", seed=31),
        _chain("leaky_queue_capacity_1", ["leaky", 5.0], cap=1, source="poisson", seed=32),
        _chain("token_capacity_1", ["token", 1, 6.0], source="poisson", rate=9.0, seed=33),
        _chain("token_initial_0", ["token", 4, 5.0, 0.0], source="poisson", seed=34),
        _chain("token_initial_half", ["token", 4, 5.0, 0.5], seed=35),
        _chain("probed_limiter", ["leaky", 6.0], cap=8, source="poisson", rate=12.0, seed=36,
               probes=[[["limiter", 0], "queue_depth", 0.1], [["server", 0], "depth", 0.25]]),
        _chain("scheduled_same_ns", ["token", 2, 3.0], rate=2.0, seed=37,
               schedule=[[["limiter", 0], t] for t in (0.0, 0.25, 0.25, 0.25, 1.0, 1.5, 1.5, 4.999, 5.0, 5.5)]),
        _chain("windows", ["sliding", 0.4, 3], source="poisson", rate=12.0, svc="exp", seed=38, windows=[0.3, 0.9, 0.9, 2.0, 3.75]),
    ]
    # a limiter behind a Server, and behind a lossy link
    f.append(dict(name="behind_server_and_lossy_link", topology="graph", n_sinks=2,
                  servers=[dict(mean=0.03, c=2, cap=None, out=["limiter", 0]), dict(mean=0.02, c=1, cap=None, out=["link", 0]),
                           dict(mean=0.05, c=1, cap=None, out=["sink", 1])],
                  links=[dict(lat=0.004, jk="exp", jm=0.003, loss=0.2, to=["limiter", 1])], routers=[], lbs=[],
                  limiters=[dict(policy=["fixed", 4, 0.25], cap=6, out=["sink", 0]), dict(policy=["token", 3, 8.0], cap=3, out=["server", 2])],
                  sources=[dict(kind="poisson", rate=20.0, to=0), dict(kind="poisson", rate=15.0, to=1)], end_s=4.0, seed=41))
    # two limiters in a row
    f.append(dict(name="two_in_a_row", topology="graph", n_sinks=1, servers=[dict(mean=0.04, c=1, cap=None, out=["sink", 0])], links=[],
                  routers=[], lbs=[],
                  limiters=[dict(policy=["token", 5, 9.0], cap=10, out=["limiter", 1]), dict(policy=["leaky", 7.0], cap=3, out=["server", 0])],
                  sources=[dict(kind="poisson", rate=14.0, to=["limiter", 0]), dict(kind="constant", rate=2.0, to=["limiter", 0])],
                  end_s=5.0, seed=42))
    # in front of a ConsistentHash LoadBalancer with client-keyed Sources
    f.append(dict(name="before_chash_lb", topology="graph", n_sinks=1,
                  servers=[dict(mean=0.08, c=1, cap=None, out=["sink", 0]) for _ in range(4)], links=[], routers=[],
                  lbs=[dict(strategy="chash", vnodes=20, backends=[0, 1, 2, 3])],
                  limiters=[dict(policy=["sliding", 0.25, 4], cap=20, out=["lb", 0])],
                  sources=[dict(kind="poisson", rate=10.0, to=["limiter", 0], n_clients=40),
                           dict(kind="poisson", rate=8.0, to=["limiter", 0], n_clients=40)], end_s=5.0, seed=43))
    # one of several router targets
    f.append(dict(name="router_target", topology="graph", n_sinks=2,
                  servers=[dict(mean=0.01, c=1, cap=None, out=["router", 0]), dict(mean=0.05, c=1, cap=None, out=["sink", 1])], links=[],
                  routers=[dict(targets=[["limiter", 0], ["sink", 0], ["server", 1], ["limiter", 0]])], lbs=[],
                  limiters=[dict(policy=["fixed", 2, 0.25], cap=5, out=["server", 1])],
                  sources=[dict(kind="poisson", rate=30.0, to=0)], end_s=4.0, seed=44))
    # end_time = Infinity: three scheduled Requests; the run ends after 4 events with two Requests still queued
    f.append(dict(name="auto_terminate", topology="graph", n_sinks=1, servers=[], links=[], routers=[], lbs=[],
                  limiters=[dict(policy=["leaky", 1.0], cap=1000, out=["sink", 0])], sources=[], end_s=0.0, auto=True, seed=45,
                  schedule=[[["limiter", 0], t] for t in (0.0, 0.1, 0.2)]))
    # FixedWindowPolicy's float floor division at growing magnitudes of the clock (at 4 x 10^6 s one ulp of to_seconds is about a
    # nanosecond).  With these window sizes the REFERENCE does not survive a Request that is still queued at certain window ends:
    # `now_s // w` puts the first nanosecond of the new window into the old one (0.3 // 0.1 == 2.0; with w = 1/3 at every window,
    # because Instant + w truncates w to 333 333 333 ns), time_until_available then answers Duration.ZERO (`remaining <= 0`) and the
    # poll is rescheduled for its own nanosecond for ever.  Such a run cannot be recorded, so these cases use queue_capacity = 0
    # (every denied Request is dropped: try_acquire and the window starts at every arrival, no poll) ...
    for w, wn in ((0.1, "0p1"), (0.3, "0p3"), (1.0 / 3.0, "third")):
        for start_s in (0, 10 ** 5, 4 * 10 ** 6):
            f.append(_chain(f"fixed_w{wn}_start{start_s}", ["fixed", 2, w], source="poisson", rate=25.0, mean=0.01, end_s=3.0,
                            seed=50 + len(f), start_ns=start_s * 10 ** 9, cap=0))
    # ... plus, where a search over Poisson(8) / Poisson(5) Sources and seeds 0 .. 149 found a run that queues and still ends in the
    # reference, that run (most queued Requests per window size and start; none exists for w = 1/3)
    for w, wn, start_s, seed in ((0.1, "0p1", 0, 10), (0.1, "0p1", 10 ** 5, 61), (0.3, "0p3", 0, 36), (0.3, "0p3", 10 ** 5, 74),
                                 (0.3, "0p3", 4 * 10 ** 6, 25)):
        f.append(_chain(f"fixed_w{wn}_start{start_s}_queued", ["fixed", 1, w], source="poisson", rate=5.0, mean=0.01, end_s=3.0, seed=seed,
                        start_ns=start_s * 10 ** 9))
    # more nodes than the loop keeps in LDS: 70 chains = 280 nodes
    f.append(dict(name="nodes_beyond_lds", topology="graph", n_sinks=70,
                  servers=[dict(mean=0.05, c=1, cap=None, out=["sink", j], svc="exp") for j in range(70)], links=[], routers=[], lbs=[],
                  limiters=[dict(policy=list(FOUR[POLICIES[j % 4]]), cap=3, out=["server", j]) for j in range(70)],
                  sources=[dict(kind="poisson", rate=6.0 + j % 5, to=["limiter", j]) for j in range(70)], end_s=1.0, seed=46))
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()


def _random_policy(rng, kind=None, odd_windows=False):
    kind = kind or str(rng.choice(POLICIES))
    if kind == "token":
        cap = float(rng.choice([1, 2, 3.5, 6]))
        init = [None, None, 0.0, 0.5, cap][int(rng.integers(0, 5))]
        return ["token", cap, float(rng.choice([2.0, 5.0, 7.5, 20.0])), init]
    if kind == "leaky":
        return ["leaky", float(rng.choice([3.0, 4.0, 7.0, 12.5]))]
    if kind == "sliding":
        return ["sliding", float(rng.choice([0.1, 0.25, 1.0 / 3.0, 0.7])), int(rng.integers(1, 6))]
    # (runs: window sizes whose multiples are exact in binary64 -- with 0.1, 0.3 or 1/3 the reference itself never returns once a
    #  Request is queued at certain window ends, see _fixtures; call sequences take those too)
    return ["fixed", int(rng.integers(1, 6)), float(rng.choice([0.1, 0.3, 1.0 / 3.0, 0.5] if odd_windows else [0.125, 0.25, 0.5, 0.75]))]


def _is_random_lb(spec, ref):
    return isinstance(ref, list) and ref[0] == "lb" and spec["lbs"][ref[1]]["strategy"] == "random"


def random_spec(k):
    """A general graph of random_specs with limiters put on its edges: in front of what a Source, a Server, a link, a router or a
    schedule()d Request aims at, and behind other limiters; policy and upstream kind of the first limiters are forced by `k` so that
    the 120 cases cover every (policy, upstream) pair (make_golden_rate_limiter.py asserts it)."""
    spec = lb_graph_spec(k) if k % 2 else graph_spec(k)
    rng = np.random.default_rng(91_000 + k)
    spec["name"] = f"limiter_graph_{k}"
    spec.setdefault("lbs", [])
    lims = spec["limiters"] = []
    used = spec["limiter_upstreams"] = []

    def put(dest, up, kind=None):
        lims.append(dict(policy=_random_policy(rng, kind), cap=int(rng.choice([0, 1, 2, 5, 1000])), out=dest))
        used.append(up)
        return ["limiter", len(lims) - 1]

    want_pol, want_up = POLICIES[k % 4], UPSTREAMS[(k // 4) % 6]
    edges = []                                                     # (upstream kind, the dict / list that holds the reference, its key)
    for sc in spec["sources"]:
        edges.append(("source", sc, "to"))
    for sv in spec["servers"]:
        if sv.get("out") is not None:
            edges.append(("server", sv, "out"))
    for lk in spec["links"]:
        edges.append(("link", lk, "to"))
    for rt in spec["routers"]:
        for q in range(len(rt["targets"])):
            edges.append(("router", rt["targets"], q))
    for entry in spec.get("schedule") or []:
        edges.append(("schedule", entry, 0))

    def dest_of(holder, key):
        d = holder[key]
        return ["server", d] if isinstance(d, int) else list(d)

    forced = False
    order = rng.permutation(len(edges))
    for e in order:
        up, holder, key = edges[e]
        dest = dest_of(holder, key)
        if _is_random_lb(spec, dest):
            continue                                               # (a Random LoadBalancer chooses by the draw of a Source that aims AT it)
        force = not forced and (up == want_up or want_up == "limiter")
        if not force and rng.random() > 0.25:
            continue
        kind = None
        if force:
            forced, kind = True, want_pol
            if want_up == "limiter":                               # a limiter behind a limiter: the forced policy sits behind
                dest = put(dest, "limiter", kind)
                kind = None
        holder[key] = put(dest, up, kind)
    if not forced and want_up == "schedule":                       # (a spec without schedule()d Requests gets one)
        spec.setdefault("schedule", []).append([put(["sink", 0], "schedule", want_pol), float(np.round(rng.uniform(0, spec["end_s"]), 3))])
    return spec


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def guard_spec(kind, j):
    """Try `j` of the search for a run in which `time_until_available` of policy `kind` returns Duration(1)."""
    rng = np.random.default_rng(97_000 + 17 * j + POLICIES.index(kind))
    source = "constant" if j % 2 == 0 else "poisson"
    return _chain(f"guard_{kind}_{j}", _random_policy(rng, kind), source=source, rate=float(rng.choice([8.0, 10.0, 12.0, 30.0])),
                  cap=int(rng.integers(1, 6)), mean=0.01, end_s=2.0, seed=int(rng.integers(1, 10_000)))


def policy_calls(kind, j):
    """Call sequence `j` for policy `kind`: (policy spec, [(now_ns, method)]) -- non-decreasing times with repeats, gaps from below a
    nanosecond's worth of capacity to several windows, both methods mixed."""
    rng = np.random.default_rng(95_000 + 31 * j + POLICIES.index(kind))
    pol = _random_policy(rng, kind, odd_windows=True)
    start = int(rng.choice([0, 0, 10 ** 14, 4 * 10 ** 15]))
    gaps = rng.choice([0, 1, 2, 999, 10 ** 6, 33_333_333, 10 ** 8, 3 * 10 ** 8, 10 ** 9], size=400,
                      p=[0.1, 0.05, 0.05, 0.05, 0.15, 0.2, 0.2, 0.15, 0.05])
    jitter = rng.integers(0, 1000, size=400) * (gaps > 2)
    t = start + np.cumsum(gaps + jitter)
    methods = rng.choice(["try_acquire", "time_until_available"], size=400, p=[0.7, 0.3])
    return pol, [(int(a), str(m)) for a, m in zip(t, methods)]


N_POLICY_CALLS = 6


def policy_state(pol):
    """The visible state of a policy object (either library's) as integers and floats."""
    def ns(x):
        return -1 if x is None else int(x.nanoseconds)
    if hasattr(pol, "_refill_rate"):
        return [float(pol._tokens), ns(pol._last_refill_time)]
    if hasattr(pol, "_leak_interval"):
        return [ns(pol._last_leak_time)]
    if hasattr(pol, "_request_log"):
        log = pol._request_log
        return [len(log), ns(log[0]) if log else -1, ns(log[-1]) if log else -1]
    return [ns(pol._current_window_start), int(pol._current_window_count)]


def replay(pol, calls):
    """Every call's result (bool, or the wait in nanoseconds) and the state it leaves."""
    out = []
    for now_ns, method in calls:
        r = getattr(pol, method)(replay.instant(now_ns))
        out.append([int(r) if isinstance(r, bool) else int(r.nanoseconds)] + policy_state(pol))
    return out


replay.instant = hs.Instant       # (make_golden_rate_limiter.py sets the reference's Instant)


def limiter_results(lims):
    """What both libraries' limiters show after a run (recorded keys of the rate_limiter family and of every later one)."""
    out = dict(lim_stats=np.array([[x.stats.received, x.stats.forwarded, x.stats.queued, x.stats.dropped, x.queue_depth,
                                    int(x._poll_scheduled)] for x in lims], np.int64).reshape(-1, 6))
    for name in ("received_times", "forwarded_times", "dropped_times"):
        flat, off = [], [0]
        for x in lims:
            flat.extend(int(t.nanoseconds) for t in getattr(x, name))
            off.append(len(flat))
        out["lim_" + name] = np.asarray(flat, np.int64)
        out["lim_" + name + "_off"] = np.asarray(off, np.int64)
    state, logs, loff = [], [], [0]
    for x in lims:
        st = policy_state(x.policy)
        state.append([float(v) for v in st] + [0.0] * (3 - len(st)))
        logs.extend(int(t.nanoseconds) for t in getattr(x.policy, "_request_log", []))
        loff.append(len(logs))
    out["lim_policy_state"] = np.asarray(state, np.float64).reshape(-1, 3)
    out["lim_log"], out["lim_log_off"] = np.asarray(logs, np.int64), np.asarray(loff, np.int64)
    return out
