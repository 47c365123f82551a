"""GPU: the load-balancer sorts' run fix-ups beyond their LDS tile and halo (csrc/hs_lb.hip), bit-exact against the C oracle.

The two radix sorts of the pipeline skip the low g_arr / g_sink key bits; elements that agree above bit g leave the sort in input
order and four kernels put every such run into full-key order: hs_lb_segments (arrivals by (backend, ns)), hs_lb_rr_assign (all
Requests by ns, RoundRobin), hs_lb_sink_finish (the shared Sink's merge) and hs_lb_fix_runs (the latency statistics).  The host
picks g for <= 1 element per bucket ON AVERAGE; the specs below defeat that estimate with legal inputs -- one client key under
ConsistentHash (everything on one backend while the estimate divides by B), lock-step constant Sources (dozens of Requests on one
nanosecond at a tiny total rate) -- so that runs outgrow the halo (kSegHalo = 32: the walk leaves LDS for global memory), straddle
tile boundaries (kSegTile = 1 024: a run begins in one workgroup's tile and ends in another's) and swallow whole tiles.

Every case first ASSERTS from the oracle's results and `eng.sort_plan()` that it crosses what it claims to cross (`_crosses`), then
compares everything `helpers.compare_lb_engine_with_oracle` compares, the full Sink order included.  Also crossed here: the busiest
backend beyond the rows of the [k][backend] layout without debug flag 4 (`hs_lb_layout`), and the look-back radix variant (debug
flag 16) over more than two whole windows of W = 16 tiles.  The sizes held as literals here are pinned on the source text by
tests/test_lb_runs_host.py.
"""
import functools

import numpy as np
import pytest

import helpers as H
from happy_simulator_amd import _native as N
from oracle import hs_oracle as O
from test_gpu_lb import _python_latency_stats

pytestmark = pytest.mark.gpu

K_RADIX_TILE, K_LOOK_BACK_W = 4096, 16          # csrc/hs_radix.hpp (pinned by tests/test_lb_runs_host.py)

_DETUNED = [1.0 / (1.0 + i * 2e-6) for i in range(56)]       # 56 constant Sources whose ticks drift microseconds apart
# (lock-step specs: the first Source ticks alone on its first nanosecond -- rate 2.0, or the fastest of the detuned rates -- the
#  start-up condition test_gpu_lb.py's TIES comment explains)
SPECS = {
    # ConsistentHash with ONE client key: every Request on one backend, distinct Poisson nanoseconds
    "hot_backend": dict(n_sources=160, n_backends=2048, rate=30.0, mean=0.00012, vnodes=3, n_clients=1, end_s=6.0, seed=21),
    "hot_backend_c2": dict(n_sources=160, n_backends=2048, rate=30.0, mean=0.0002, concurrency=2, queue_cap=40, vnodes=3, n_clients=1,
                           end_s=6.0, seed=28),
    "three_hot": dict(n_sources=96, n_backends=1024, rate=30.0, mean=0.0004, vnodes=3, n_clients=3, end_s=6.0, seed=22),
    # lock-step constant Sources: 55 Requests on one nanosecond (equal keys: input order must survive), 56 on the whole seconds --
    # under debug flag 2 all of them wait in the event-order loop's in-group FIFO at once (kLbQCap = 60; it refused them at 48) ...
    "bursts_one_client": dict(n_sources=56, n_backends=64, rate=[2.0] + [1.0] * 55, mean=0.002, vnodes=50, n_clients=1, end_s=600.0,
                              seed=24, arr="constant", svc="exp"),
    "bursts_rr": dict(strategy="round_robin", n_sources=56, n_backends=64, rate=[2.0] + [1.0] * 55, mean=0.002, vnodes=1, n_clients=1,
                      end_s=600.0, seed=23, arr="constant", svc="exp"),
    # ... and detuned ones: long runs of DISTINCT keys inside one 2^g ns bucket
    "bursts_rr_distinct": dict(strategy="round_robin", n_sources=56, n_backends=64, rate=_DETUNED, mean=0.002, vnodes=1, n_clients=1,
                               end_s=600.0, seed=25, arr="constant", svc="exp"),
    "bursts_chash_distinct": dict(n_sources=56, n_backends=8, rate=_DETUNED, mean=0.0005, vnodes=50, n_clients=1, end_s=600.0, seed=26,
                                  arr="constant", svc="exp"),
    "look_back_three_windows": dict(n_sources=768, n_backends=768, rate=30.0, mean=0.01, vnodes=50, n_clients=1 << 20, end_s=6.0, seed=27),
    # constant service on idle backends: thousands of exactly equal latencies (hs_lb_fix_runs on nearly one run)
    "equal_latencies": dict(n_sources=8, n_backends=64, rate=2.0, mean=0.03, vnodes=20, n_clients=1 << 16, end_s=6.0, seed=29, svc="const"),
    # (the same at a size where the equal latencies are thousands)
    "equal_latencies_thousands": dict(n_sources=64, n_backends=4096, rate=10.0, mean=0.03, vnodes=20, n_clients=1 << 16, end_s=6.0, seed=30,
                                      svc="const"),
}

FLAG_IDS = {0: "segmented_scan", 64: "request_order", 2: "event_order", 4: "dense_layout", 16: "look_back_radix_passes"}
CASES = [(name, f) for name in ("hot_backend", "three_hot", "bursts_one_client", "bursts_rr", "bursts_rr_distinct", "bursts_chash_distinct")
         for f in (0, 64, 2, 4, 16)]
CASES += [("hot_backend_c2", f) for f in (0, 2, 16)]           # (C == 2: flag 0 already takes hs_lbk_backends<2>)
CASES += [("look_back_three_windows", f) for f in (0, 16)]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(graph, params, the oracle's run, its run once more with one Sink per backend): computed once per spec, never changed."""
    spec = SPECS[name]
    g, p = H.oracle_lb_graph_ext(spec)
    r = O.run(g, p["end_ns"], seed=spec["seed"])
    g2, p2 = H.oracle_lb_graph_ext(dict(spec, shared_sink=False))
    r2 = O.run(g2, p2["end_ns"], seed=spec["seed"])
    return g, p, r, r2


def _runs(sorted_keys, g):
    """(start, length) of the maximal stretches of equal key >> g."""
    if len(sorted_keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    hi = sorted_keys >> np.uint64(g)
    start = np.flatnonzero(np.concatenate(([True], hi[1:] != hi[:-1])))
    return start, np.diff(np.concatenate((start, [len(hi)])))


def _figures(keys, g, plan, missing=None):
    """Run-length figures of one sorted key list.  The list may lack elements of the list the device sorts (the completed records
    are a subset of the Requests): `missing` = (a lower bound of each such element's key, ascending; how many at that bound), so an
    element at `pos` here lies in [pos, pos + slack] there, slack = the missing elements whose bound does not exceed its key.  The
    position claims below hold for every such shift, the length claims because a subset's runs are no longer than the whole's."""
    tile, halo = plan["seg_tile"], plan["seg_halo"]
    start, length = _runs(keys, g)
    long_ = length > halo
    s, e = start[long_], start[long_] + length[long_]                       # the long runs: [s, e)
    slack = np.zeros(len(s), np.int64)
    if missing is not None and len(s):
        bound, count = missing
        slack = np.concatenate(([0], np.cumsum(count)))[np.searchsorted(bound, keys[s], side="right")]
    m = (s + slack) // tile * tile + tile                                   # the first tile boundary behind s + slack
    nearest = (s + tile // 2) // tile * tile
    return dict(n=len(keys), longest=int(length.max()) if len(length) else 0, long_runs=int(long_.sum()),
                straddling=int((m <= e - 1).sum()),                         # s + slack < m <= e - 1: begins in one tile, ends in another
                starts_near_a_tile_edge=int(((nearest - halo <= s) & (s + slack <= nearest + halo)).sum()))


@functools.lru_cache(maxsize=None)
def _measured(name, plan_items):
    plan = dict(plan_items)
    spec = SPECS[name]
    g, p, r, r2 = _oracle(name)
    S, B, tb = p["S"], p["B"], plan["tb"]
    per_backend = [r2.sinks[i] for i in sorted(r2.sinks)]                   # (t, created_at = the Request's arrival ns) per backend
    assert len(per_backend) == B
    n_req = int(r.lbs[S]["total_requests"].sum())
    n_rec = sum(len(t) for t, _ in per_backend)
    # Requests without a record.  One worker, unbounded FIFO: a backend completes in arrival order, so they arrived no earlier than
    # its last recorded Request; otherwise nothing is known about where they sort (bound 0: they may shift every position).
    miss = (r.lbs[S]["total_requests"] - np.array([len(t) for t, _ in per_backend])).astype(np.int64)
    fifo = set(p["conc"]) == {1} and set(p["qcap"]) == {-1}
    last = np.array([int(cr[-1]) if fifo and len(cr) else 0 for _, cr in per_backend], np.uint64)
    shl = lambda j: np.uint64(j) << np.uint64(tb)   # noqa: E731
    arr = np.sort(np.concatenate([shl(j) | cr.astype(np.uint64) for j, (_, cr) in enumerate(per_backend)]))
    arr_missing = (np.array([shl(j) | last[j] for j in range(B)], np.uint64), miss)
    allreq = np.sort(np.concatenate([cr for _, cr in per_backend]).astype(np.uint64))
    by_ns = np.argsort(last, kind="stable")
    sink_t = r.sinks[sorted(r.sinks)[0]][0]          # (the device merges exactly these records: nothing missing)
    assert (np.diff(sink_t) >= 0).all() and int(miss.sum()) == n_req - n_rec and (miss >= 0).all()
    out = dict(plan=plan, requests=n_req, records=n_rec, busiest=int(r.lbs[S]["total_requests"].max()),
               mean_load=float(sum(p["rate"])) * spec["end_s"] / B, equal_sink_ns=int(len(sink_t) - len(np.unique(sink_t))),
               arrivals=_figures(arr, plan["g_arr"], plan, arr_missing),
               all_requests=_figures(allreq, plan["g_sink"], plan, (last[by_ns], miss[by_ns])),
               sink=_figures(sink_t.astype(np.uint64), plan["g_sink"], plan),
               dense_tiles=-(-n_req // K_RADIX_TILE), pass0_tiles=-(-int(r.generated[:S].max()) * S // K_RADIX_TILE))
    print(f"\n{name}: {out}")
    return out


def _crosses(name, eng):
    """The precondition of a spec, from the oracle's results and the engine's own sort plan alone."""
    plan = eng.sort_plan()
    assert plan["g_arr"] <= plan["tb"]                                      # (a run of the arrival sort never spans two backends)
    m = _measured(name, tuple(sorted(plan.items())))
    tile, halo = plan["seg_tile"], plan["seg_halo"]
    arr, req, snk = m["arrivals"], m["all_requests"], m["sink"]
    # distinct completion ns: the one documented cross-backend tie cannot occur, so the FULL Sink order is asserted below
    assert m["equal_sink_ns"] == 0
    if name in ("hot_backend", "hot_backend_c2"):
        assert arr["longest"] >= tile + 2 * halo + 1                        # a whole tile and both halos inside one run
        assert m["busiest"] > 3 * m["mean_load"] + 64                       # beyond the rows of the [k][backend] layout
    elif name == "three_hot":
        assert arr["long_runs"] >= 100 and arr["starts_near_a_tile_edge"] >= 1
    elif name == "bursts_one_client":
        assert arr["long_runs"] >= 100 and arr["straddling"] >= 1
    elif name in ("bursts_rr", "bursts_rr_distinct"):
        assert req["long_runs"] >= 100 and req["straddling"] >= 1
        assert snk["long_runs"] >= 100 and snk["straddling"] >= 1
    elif name == "bursts_chash_distinct":
        assert arr["long_runs"] >= 100 and snk["long_runs"] >= 100
    elif name == "look_back_three_windows":
        assert m["dense_tiles"] >= 2 * K_LOOK_BACK_W + 1 and m["pass0_tiles"] >= m["dense_tiles"]
    return m


@pytest.mark.parametrize("name,flags", CASES, ids=[f"{n}-{FLAG_IDS[f]}" for n, f in CASES])
def test_lb_runs_beyond_the_halo_and_the_tile_match_oracle(name, flags):
    spec = SPECS[name]
    _, p, r, _ = _oracle(name)
    eng, _ = H.lb_engine_for_spec(spec, flags=flags)
    with eng:
        _crosses(name, eng)
        for _ in range(2):                   # (the second run restarts from start_ns: descriptors, tickets and offsets clean again)
            eng.run(p["end_ns"])
            H.compare_lb_engine_with_oracle(eng, p, r, check_sink_order=True)
            path = eng.run_path()
            if name.startswith("hot_backend") and not path & N.LB_RUN_SCAN and flags != 4:
                assert path & N.LB_RUN_DENSE             # the busiest backend outgrew the rows: dense layout without debug flag 4
            if name == "bursts_rr" and flags == 64:
                assert not path & N.LB_RUN_DENSE         # (... and the bit is no constant: here the [k][backend] layout fits)
    if name == "hot_backend":
        assert (flags in (0, 16)) == bool(path & N.LB_RUN_SCAN)


@pytest.mark.parametrize("name", ["hot_backend", "bursts_rr", "equal_latencies", "equal_latencies_thousands"])
def test_latency_statistics_past_the_run_fix_up(name):
    """hs_lb_latency_stats sorts on key bits [tb % 8, tb) and finishes with hs_lb_fix_runs (one thread per run): the reference's
    formulas on the oracle's Sink records, on runs of distinct latencies and on thousands of exactly equal ones.  (bursts_rr: tb = 40,
    whole passes and no fix-up -- the statistics of the long runs' records all the same.)"""
    spec = SPECS[name]
    _, p, r, _ = _oracle(name)
    t, cr = r.sinks[sorted(r.sinks)[0]]
    lat = ((t - cr).astype(np.float64) / 1e9).tolist()
    eng, _ = H.lb_engine_for_spec(spec)
    with eng:
        plan = eng.sort_plan()
        g = plan["tb"] % 8
        _, length = _runs(np.sort((t - cr).astype(np.uint64)), g)
        equal = int((t - cr == H.ns_from_seconds(spec["mean"])).sum())       # served at once by an idle backend, constant service
        print(f"\n{name}: tb {plan['tb']}, skipped bits {g}, {len(lat)} latencies, longest run {int(length.max())}, "
              f"runs > 1: {int((length > 1).sum())}, latencies equal to the service time: {equal}")
        if name != "bursts_rr":
            assert g > 0 and plan["tb"] > 8                                  # the fix-up runs at all
        if name == "hot_backend":
            assert (length > 1).sum() >= 100
        elif name.startswith("equal_latencies"):
            assert length.max() >= equal > 0.8 * len(lat)                    # nearly one run, of equal values
            assert equal >= (2000 if name.endswith("thousands") else 50)
        eng.run(p["end_ns"])
        got = eng.latency_stats()
        assert got == _python_latency_stats(lat)
        eng.run(p["end_ns"])                 # the statistics pass must leave the engine re-runnable
        H.compare_lb_engine_with_oracle(eng, p, r, check_sink_order=True)
        assert eng.latency_stats() == got


def test_weighted_round_robin_on_the_long_runs_agrees_with_the_single_heap_loop():
    """hs_lb_rr_assign's `table[pos % W]` branch on bursts_rr's runs of 55 equal nanoseconds.  The C oracle has no
    WeightedRoundRobin and no recording of the live reference holds this case, so the second opinion here is the product's other
    path: the single-heap loop (csrc/hs_graph.hip, pinned to the live reference on WeightedRoundRobin by test_gpu_lb_strategies.py),
    array for array; the per-backend counts are the selection table's over the oracle's Request count."""
    import family_checks as FC
    import happy_simulator_amd as hs
    import strategy_specs as SS
    from happy_simulator_amd import lowering as L

    rr = SPECS["bursts_rr"]
    weights = [3, 1, 2] * 21 + [1]
    eng, _ = H.lb_engine_for_spec(rr)                  # (same Sources, backends and horizon: the plan of the WeightedRoundRobin engine)
    with eng:
        m = _crosses("bursts_rr", eng)                 # constant Sources: the arrival nanoseconds do not depend on the strategy
    spec = SS._lb_case("bursts_wrr", "wrr", rr["n_backends"], [dict(kind="constant", rate=x) for x in rr["rate"]], weights=weights,
                       mean=rr["mean"], end_s=rr["end_s"], seed=rr["seed"], pipeline=True)
    sim, ents = SS.build(spec)
    assert isinstance(sim.lowered(), L.LbGraph)
    sim.run()
    sim2, ents2 = SS.build(spec)
    SS.force_single_heap(sim2, spec).run()
    a, b = SS.results(spec, sim, ents), SS.results(spec, sim2, ents2)
    FC.same(a, b, spec["name"])
    table = hs.WeightedRoundRobin.selection_table(weights)
    assert len(table) == sum(weights) and a["lb_stats"][0][1] == m["requests"]
    np.testing.assert_array_equal(a["lb_backend_total_requests"], np.bincount(table[np.arange(m["requests"]) % len(table)], minlength=len(weights)))
    assert len(np.unique(a["sink_t_ns"])) == len(a["sink_t_ns"]) > 30_000          # distinct completion ns: the full Sink order was compared


@pytest.mark.parametrize("name", ["bursts_rr", "hot_backend"])
def test_lb_long_runs_in_windows_equal_one_run(name):
    """test_gpu_lb.py::test_lb_windows_equal_one_run on the long runs: a run cut by a window's end is a shorter run with the same
    prefix -- against the oracle at every end."""
    spec = SPECS[name]
    g, p, _, _ = _oracle(name)
    end = p["end_ns"]
    eng, _ = H.lb_engine_for_spec(spec)
    with eng:
        _crosses(name, eng)
        for e in (end // 7, end // 3, end // 3, (2 * end) // 3, end):
            eng.run(e)
            H.compare_lb_engine_with_oracle(eng, dict(p, end_ns=e), O.run(g, e, seed=spec["seed"]), check_sink_order=True)
