"""CPU: RateLimitedEntity and its policies on the host -- constructors and error texts against the recorded live reference
(tests/golden/live_rate_limiter/), the host-Python policies against the recorded call sequences, the lowering's node arrays, every
refusal by name, the C ABI's new symbols.  Nothing here launches a kernel."""
import math
import os
import re

import numpy as np
import pytest

import graph_family as GF
import happy_simulator_amd as hs
import rate_limiter_specs as RS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, lower_general, split_parts
from recorded import RATE_LIMITER as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_defaults_properties_and_error_texts_equal_the_reference():
    ref = RR.get("defaults")
    tb, lb, sw, fw = hs.TokenBucketPolicy(), hs.LeakyBucketPolicy(), hs.SlidingWindowPolicy(), hs.FixedWindowPolicy(7)
    assert dict(capacity=tb.capacity, refill_rate=tb.refill_rate, tokens=tb.tokens, state=RS.policy_state(tb),
                initial=hs.TokenBucketPolicy(4, 2, 0.5).tokens,
                types=[type(tb.capacity).__name__, type(tb.refill_rate).__name__]) == ref["token"]
    assert dict(leak_rate=lb.leak_rate, interval=lb._leak_interval, state=RS.policy_state(lb),
                zero_interval=hs.LeakyBucketPolicy(0)._leak_interval) == ref["leaky"]
    assert dict(window_size_seconds=sw.window_size_seconds, max_requests=sw.max_requests, state=RS.policy_state(sw)) == ref["sliding"]
    errors = []
    for args in ((0, 1.0), (-2, 1.0), (3, 0), (3, -0.5)):
        with pytest.raises(ValueError) as e:
            hs.FixedWindowPolicy(*args)
        errors.append(str(e.value))
    assert dict(requests_per_window=fw.requests_per_window, window_size=fw.window_size, state=RS.policy_state(fw), errors=errors) == ref["fixed"]
    for pol, names in ((tb, ("capacity", "refill_rate", "tokens")), (lb, ("leak_rate",)), (sw, ("window_size_seconds", "max_requests")),
                       (fw, ("requests_per_window", "window_size"))):
        for name in names:                                     # read-only, as the reference's properties are
            with pytest.raises(AttributeError):
                setattr(pol, name, 1)
    k = hs.Sink("k")
    ent = hs.RateLimitedEntity("lim", k, tb)
    s = ent.stats
    got = dict(queue_capacity=ent._queue.capacity, queue_depth=ent.queue_depth, stats=[s.received, s.forwarded, s.queued, s.dropped],
               stats_type=type(s).__name__, downstream_is=ent.downstream is k, policy_is=ent.policy is tb,
               downstream_entities=[x.name for x in ent.downstream_entities()],
               series=[ent.received_times, ent.forwarded_times, ent.dropped_times], poll_scheduled=ent._poll_scheduled)
    try:
        s.received = 1
        got["stats_frozen"] = False
    except Exception as e:  # noqa: BLE001
        got["stats_frozen"] = type(e).__name__
    assert got == ref["entity"]
    assert isinstance(ent, hs.Entity) and hs.RateLimitedEntityStats() == hs.RateLimitedEntityStats(0, 0, 0, 0)


@pytest.mark.parametrize("kind", RS.POLICIES)
def test_host_policies_reproduce_every_recorded_call(kind):
    """(now_ns, method) -> (result, state after it), 400 calls per sequence: repeated nanoseconds, gaps below one token's worth of
    time, clocks at 10^5 s and 4 x 10^6 s."""
    for j in range(RS.N_POLICY_CALLS):
        ref = RR.get("policy_calls", kind, j)
        pol, calls = RS.policy_calls(kind, j)
        assert pol == ref["policy"]
        np.testing.assert_array_equal(np.array([[t, m == "try_acquire"] for t, m in calls], np.int64), ref["calls"])
        got = np.array(RS.replay(RS.make_policy(hs, pol), calls), np.float64)
        bad = np.nonzero((got != ref["results"]).any(axis=1))[0]
        assert len(bad) == 0, (kind, j, pol, int(bad[0]), calls[int(bad[0])], got[bad[0]].tolist(), ref["results"][bad[0]].tolist())
        assert ref["results"][:, 0].min() == 0 and ref["results"][:, 0].max() >= 1        # both answers occur


def _py_fmod(x, y):
    """csrc/hs_graph.hip exact_fmod_pos, restated: the remainder of the two significands as integers."""
    if x < y:
        return x
    mx, ex = math.frexp(x)
    my, ey = math.frexp(y)
    mx, my = int(mx * 2 ** 53), int(my * 2 ** 53)
    r = mx % my
    for _ in range(ex - ey):
        r <<= 1
        if r >= my:
            r -= my
    return math.ldexp(r, ey - 53)


def _py_floordiv(v, w):
    mod = _py_fmod(v, w)
    div = (v - mod) / w
    if div == 0.0:
        return 0.0
    fl = math.floor(div)
    return float(fl + 1 if div - fl > 0.5 else fl)


def test_the_kernels_floor_division_is_pythons():
    """FixedWindowPolicy._get_window_start is `now_s // window_size` on floats.  The kernel computes it from an exact integer
    remainder (no library fmod), the quotient of the rest and a floor with CPython's half-way fix-up.  This checks the ALGORITHM, restated
    in Python, against the interpreter's own `//` and `math.fmod`; the device code itself is compared with `//` on the GPU
    (tests/test_gpu_rate_limiter.py::test_the_kernels_window_start_is_pythons)."""
    rng = np.random.default_rng(3)
    pairs = [(t / 1e9, w) for w in (0.1, 0.3, 1.0 / 3.0, 0.5, 1.0, 1e-9, 2.5e-7)
             for t in [0, 1, 99_999_999, 100_000_000, 300_000_000, 10 ** 14 + 299_999_999, 4 * 10 ** 15 + 333_333_333] +
             rng.integers(0, 5 * 10 ** 15, 400).tolist()]
    pairs += [(float(a), float(b)) for a, b in zip(rng.uniform(0, 1e7, 2000), rng.uniform(1e-6, 50.0, 2000))]
    for v, w in pairs:
        assert _py_fmod(v, w) == math.fmod(v, w), (v, w)
        assert _py_floordiv(v, w) == v // w, (v, w)


def _lowered(name):
    sim, pools = GF.build(RS.FIXTURES[name])
    g = sim.lowered()
    assert isinstance(g, GeneralGraph)
    return sim, pools, g


def test_station_lowerings_refuse_by_name_and_the_general_graph_takes_it():
    sim, pools, g = _lowered("token_constant")
    assert "RateLimitedEntity" in sim._station_refusal
    a = g.arrays
    # nodes: the Source, then entities = servers + lbs + routers + links + limiters + sinks
    assert a.kind.tolist() == [N.NODE_SOURCE, N.NODE_SERVER, N.NODE_RATE_LIMITER, N.NODE_SINK]
    assert a.target.tolist() == [2, 3, 1, -1]
    assert a.queue_cap[2] == 4 and a.lim_policy.tolist() == [255, 255, N.LIMITER_TOKEN_BUCKET, 255]
    assert a.lim_params[2].tolist() == [3.0, 5.0, 3.0] and a.lim_count[2] == 0
    for name, lb in (("before_chash_lb", True), ("behind_server_and_lossy_link", False)):
        sim, _pools, _g = _lowered(name)
        assert "RateLimitedEntity" in sim._station_refusal or (lb and "LoadBalancer" in sim._station_refusal), sim._station_refusal


def test_lower_general_edges_and_policy_parameters():
    _sim, pools, g = _lowered("behind_server_and_lossy_link")
    a, at = g.arrays, lambda x: g.node_of[id(x)]
    srv, lim, link, sink = pools["server"], pools["limiter"], pools["link"], pools["sink"]
    assert a.target[at(srv[0])] == at(lim[0]) and a.target[at(lim[0])] == at(sink[0])          # a Server's downstream
    assert a.target[at(link[0])] == at(lim[1]) and a.target[at(lim[1])] == at(srv[2])          # a link's egress
    assert (a.lim_policy[at(lim[0])], a.lim_params[at(lim[0])].tolist(), a.lim_count[at(lim[0])]) == (N.LIMITER_FIXED_WINDOW, [0.25, 0, 0], 4)
    assert a.queue_cap[at(lim[0])] == 6 and a.queue_cap[at(lim[1])] == 3
    _sim, pools, g = _lowered("two_in_a_row")
    a = g.arrays
    l0, l1 = (g.node_of[id(x)] for x in pools["limiter"])
    assert a.target[l0] == l1 and a.target[g.node_of[id(pools["source"][0])]] == l0             # a Source's target; limiter -> limiter
    assert (a.lim_policy[l1], a.lim_params[l1].tolist()) == (N.LIMITER_LEAKY_BUCKET, [7.0, 1.0 / 7.0, 0.0])
    _sim, pools, g = _lowered("router_target")
    a = g.arrays
    r = g.node_of[id(pools["router"][0])]
    lim = g.node_of[id(pools["limiter"][0])]
    assert a.rt_targets[a.rt_off[r]:a.rt_off[r] + a.rt_cnt[r]].tolist().count(lim) == 2       # a router target
    _sim, pools, g = _lowered("before_chash_lb")
    a = g.arrays
    lim = g.node_of[id(pools["limiter"][0])]
    assert a.kind[a.target[lim]] == N.NODE_LB and (a.lim_policy[lim], a.lim_params[lim, 0], a.lim_count[lim]) == (N.LIMITER_SLIDING_WINDOW, 0.25, 4)
    assert a.src_n_clients[:2].tolist() == [40, 40]                                              # the Requests keep their client ids
    sim, pools, g = _lowered("scheduled_same_ns")                                                # a schedule() target
    _end, _start, sched, _c = sim._general_prepare(g, False)
    assert [n for n, _t in sched] == [g.node_of[id(pools["limiter"][0])]] * 10 and sched[1][1] == sched[2][1] == 250_000_000


def test_parts_carry_the_limiters():
    chains = [RS._chain(f"c{i}", list(RS.FOUR[RS.POLICIES[i % 4]]), source="poisson") for i in range(4)]
    spec = dict(name="u", topology="graph", n_sinks=4, links=[], routers=[], lbs=[], end_s=1.0, seed=1,
                servers=[dict(c["servers"][0], out=["sink", i]) for i, c in enumerate(chains)],
                limiters=[dict(c["limiters"][0], out=["server", i]) for i, c in enumerate(chains)],
                sources=[dict(c["sources"][0], to=["limiter", i]) for i, c in enumerate(chains)])
    sim, _pools = GF.build(spec)
    g = sim.lowered()
    parts = split_parts(g.arrays)
    assert len(parts) == 4
    for i, (ids, _pos, b) in enumerate(parts):
        assert sorted(b.kind.tolist()) == [N.NODE_SOURCE, N.NODE_SERVER, N.NODE_SINK, N.NODE_RATE_LIMITER]
        lim = int(np.nonzero(b.kind == N.NODE_RATE_LIMITER)[0][0])
        assert b.lim_policy[lim] == i and b.kind[b.target[lim]] == N.NODE_SERVER
        np.testing.assert_array_equal(b.lim_params[lim], g.arrays.lim_params[ids[lim]])


class AdaptivePolicy:                     # any policy object the engine does not know (the reference's AdaptivePolicy among them)
    def try_acquire(self, now):
        return True

    def time_until_available(self, now):
        return hs.Duration.ZERO


class _TokenSubclass(hs.TokenBucketPolicy):
    pass


def _refusal(policy=None, build=None):
    sink = hs.Sink("k")
    if build is None:
        lim = hs.RateLimitedEntity("lim", sink, policy)
        sim = hs.Simulation(end_time=hs.Instant.from_seconds(1), sources=[hs.Source.poisson(rate=5, target=lim)], entities=[lim, sink])
    else:
        sim = build(sink)
    with pytest.raises(hs.UnsupportedTopology) as e:
        sim.lowered()
    return str(e.value)


def test_every_refusal_names_its_reason():
    assert "policy AdaptivePolicy is not lowered" in _refusal(AdaptivePolicy())
    assert "policy _TokenSubclass is not lowered" in _refusal(_TokenSubclass())
    assert "policy NoneType is not lowered" in _refusal(None)                                    # (the null limiter)
    assert "refill_rate must be > 0, got 0.0" in _refusal(hs.TokenBucketPolicy(3, 0))
    assert "refill_rate must be > 0, got -2.0" in _refusal(hs.TokenBucketPolicy(3, -2))
    assert "leak_rate must be > 0, got 0.0" in _refusal(hs.LeakyBucketPolicy(0))
    assert "leak_rate must be > 0, got -1.0" in _refusal(hs.LeakyBucketPolicy(-1))
    assert "max_requests must be >= 1, got 0" in _refusal(hs.SlidingWindowPolicy(1.0, 0))
    assert N.LIMITER_MAX_SLIDING_LOG >= 65536
    assert f"log of {N.LIMITER_MAX_SLIDING_LOG + 1} entries is beyond" in _refusal(hs.SlidingWindowPolicy(1.0, N.LIMITER_MAX_SLIDING_LOG + 1))
    assert "window of 1e-10 s is below one nanosecond" in _refusal(hs.FixedWindowPolicy(3, 1e-10))
    used = hs.LeakyBucketPolicy(2.0)
    used.try_acquire(hs.Instant(5))
    assert "has been used already" in _refusal(used)

    def as_backend(sink):
        srv = hs.Server("s", service_time=hs.ConstantLatency(0.1), downstream=sink)
        lim = hs.RateLimitedEntity("lim", srv, hs.LeakyBucketPolicy(2.0))
        lb = hs.LoadBalancer("lb", backends=[lim])
        return hs.Simulation(end_time=hs.Instant.from_seconds(1), sources=[hs.Source.poisson(rate=5, target=lb)], entities=[lb, lim, srv, sink])

    assert "backend 'lim' of 'lb' is a RateLimitedEntity: only Server backends are lowered" in _refusal(build=as_backend)

    def shared(sink):
        pol = hs.LeakyBucketPolicy(2.0)
        a, b = hs.RateLimitedEntity("a", sink, pol), hs.RateLimitedEntity("b", sink, pol)
        return hs.Simulation(end_time=hs.Instant.from_seconds(1), entities=[a, b, sink],
                             sources=[hs.Source.poisson(rate=5, target=a), hs.Source.poisson(rate=5, target=b)])

    assert "shares its policy object with 'a'" in _refusal(build=shared)


def test_parallel_simulation_partitions_refuse_limiters():
    """ParallelSimulation lowers its partitions onto the station and sharded engines, which have no limiter."""
    parts = []
    for i in range(2):
        sink = hs.Sink(f"k{i}")
        srv = hs.Server(f"s{i}", service_time=hs.ExponentialLatency(0.05), downstream=sink)
        lim = hs.RateLimitedEntity(f"lim{i}", srv, hs.TokenBucketPolicy(3, 5.0))
        parts.append(hs.SimulationPartition(name=f"p{i}", entities=[lim, srv, sink], sources=[hs.Source.poisson(rate=8, target=lim, name=f"src{i}")]))
    with pytest.raises(hs.UnsupportedTopology, match="RateLimitedEntity"):
        hs.ParallelSimulation(parts, end_time=hs.Instant.from_seconds(1)).run()


def test_new_header_symbols_are_exported():
    N.build()
    lib = N.lib()
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    for sym in ("hs_graph_set_limiter_policy", "hs_graph_get_limiter", "hs_debug_window_start"):
        assert sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(", hdr, re.M), sym
    assert re.search(r"HS_NODE_RATE_LIMITER = 7\b", hdr) and N.NODE_RATE_LIMITER == 7
    assert re.search(r"HS_PROBE_LIMITER_DEPTH = 7\b", hdr) and N.PROBE_METRICS["queue_depth"] == 7
    enum = dict(re.findall(r"HS_LIMITER_([A-Z_]+) = (\d+)", hdr))
    assert {k: int(v) for k, v in enum.items()} == dict(
        TOKEN_BUCKET=N.LIMITER_TOKEN_BUCKET, LEAKY_BUCKET=N.LIMITER_LEAKY_BUCKET, SLIDING_WINDOW=N.LIMITER_SLIDING_WINDOW,
        FIXED_WINDOW=N.LIMITER_FIXED_WINDOW, NONE=N.LIMITER_NONE, FORWARDED=N.LIMITER_FORWARDED, QUEUED=N.LIMITER_QUEUED,
        DROPPED=N.LIMITER_DROPPED, DRAINED=N.LIMITER_DRAINED)
    import ctypes as C

    assert C.sizeof(N.LimiterPolicyParams) == 40 and C.sizeof(N.LimiterState) == 8 + 12 * 8
    assert hs.entities.N_LIMITER == dict(token=0, leaky=1, sliding=2, fixed=3)
    assert "hs_graph_set_auto_terminate" not in hdr               # auto-termination is the documented end = 2^61, no switch of its own


def test_the_recordings_hold_what_the_issue_observed():
    """The four deterministic fixtures, (received, forwarded, queued, dropped) and the event total; the auto-terminating run; and the
    1-ns guard: which policies a seeded run met it for."""
    for kind, (rec, fwd, qd, dr, ev) in RS.ISSUE_VALUES.items():
        r = RR.get("case", RS.FIXTURES[f"{kind}_constant"])
        assert r["lim_stats"][0, :4].tolist() == [rec, fwd, qd, dr] and r["total_events"] == ev
        assert r["entity_summaries"] == {"lim0": ["RateLimitedEntity", 0, True]}
    r = RR.get("case", RS.FIXTURES["auto_terminate"])
    assert r["total_events"] == 4 and r["lim_stats"][0].tolist() == [3, 1, 2, 0, 2, 1] and r["received"].tolist() == [1]
    for kind in RS.POLICIES:
        g = RR.get("guard", kind)
        assert g["tries"] >= 0 or g["tries"] == -RS.GUARD_TRIES
        if g["tries"] >= 0:
            assert int(g["result"]["lim_guard_hits"].sum()) > 0


def test_queue_depth_probe_is_the_limiters():
    sink = hs.Sink("k")
    srv = hs.Server("s", service_time=hs.ConstantLatency(0.1), downstream=sink)
    lim = hs.RateLimitedEntity("lim", srv, hs.LeakyBucketPolicy(2.0))
    with pytest.raises(NotImplementedError, match="queue_depth"):
        hs.Probe.on(srv, "queue_depth")
    probe, _data = hs.Probe.on(lim, "queue_depth", interval=0.5)
    sim = hs.Simulation(end_time=hs.Instant.from_seconds(1), sources=[hs.Source.poisson(rate=5, target=lim)], entities=[lim, srv, sink],
                        probes=[probe])
    a = sim.lowered().arrays
    assert a.kind.tolist() == [N.NODE_SOURCE, N.NODE_PROBE, N.NODE_RATE_LIMITER, N.NODE_SERVER, N.NODE_SINK]
    assert a.probe_metric[1] == N.PROBE_METRICS["queue_depth"] == 7 and a.target[1] == 2
    bad, _ = hs.Probe.on(lim, "depth")
    with pytest.raises(hs.UnsupportedTopology, match="'depth' is not an attribute of RateLimitedEntity"):
        hs.Simulation(end_time=hs.Instant.from_seconds(1), sources=[hs.Source.poisson(rate=5, target=lim)], entities=[lim, srv, sink],
                      probes=[bad]).lowered()
