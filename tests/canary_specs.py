"""Specs of the CanaryDeployer (happy_simulator_amd.entities; the reference's components/deployment/canary_deployer.py) over a
LoadBalancer of the single-heap loop.  The format is the rolling deployer's (tests/deployer_specs.py) with `canaries` in place of
`deployers`:

  canaries = [dict(lb=j, stages=[[traffic_percentage, evaluation_period], ...] | None, ev=["error", max, mult] | ["latency", max, mult] |
                   None, iv=, deploy=t_s | None, inst=dict(mean=, c=, cap=, svc=, out=pool ref))]
      CanaryDeployer(f"cn{i}", LoadBalancer j, factory, stages, evaluator, evaluation_interval=iv); the factory builds the canary
      Server(f"cn{i}_canary") as `inst` says, with SERVICE stream base len(spec["servers"]).  The deployers stand behind every other
      entity; behind the spec's own schedule deploy() is scheduled once, at `deploy` seconds.
  a fault may name ["canary", i];  auto=True: end_time = Infinity.

tests/golden/make_golden_canary.py records every spec listed here from the live reference as family "canary": what the "mixed" family
records, fourteen more by_kind rows (39: `_autoscaler_evaluate` and 40 .. 46: the rolling deployer's, always 0; 47 .. 52: the canary
deployer's six Events) and canary_results below.  CANARY reads the recordings back.  Every case has at most 20 000 Events.
"""
import numpy as np

import deployer_specs as DS
import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import mixed_specs as MX
from happy_simulator_amd.graph_engine import GraphEngine
from recorded import Recorded

CANARY = Recorded("live_canary", "canary", "make_golden_canary.py", part_bytes=640 * 1024, max_part_bytes=900 * 1024)
N_RANDOM = 100
EV_CN_FIRST = DS.N_KINDS                       # the by_kind row of `_canary_deploy_start`, the first of the six
CN_EVENTS = ("_canary_deploy_start", "_canary_stage_start", "_canary_evaluate", "_canary_promote", "_canary_rollback", "_canary_complete")
N_KINDS = EV_CN_FIRST + len(CN_EVENTS)
crash, pause, src, plain, srv, lb, _g = MX.crash, MX.pause, MX.src, MX.plain, MX.srv, MX.lb, MX._g
SINK, LB0, LB1, K0 = ["sink", 0], ["lb", 0], ["lb", 1], ["canary", 0]
STRATEGIES = DS.STRATEGIES
STATUS = {"idle": 0, "in_progress": 1, "promoting": 2, "rolled_back": 3, "completed": 4}
QUICK = [[0.01, 1.0], [0.05, 1.0], [0.25, 1.0], [1.0, 1.0]]     # the default percentages over short periods


def canary(stages=QUICK, ev=None, iv=0.5, deploy=0.5, lb=0, **instance):  # noqa: A002
    return dict(lb=lb, stages=None if stages is None else [list(s) for s in stages], ev=None if ev is None else list(ev), iv=iv,
                deploy=deploy, inst=DS.inst(**instance))


def make_evaluator(ns, ev):
    if ev is None:
        return None                                              # (the constructor's default: ErrorRateEvaluator())
    return (ns.LatencyEvaluator if ev[0] == "latency" else ns.ErrorRateEvaluator)(ev[1], ev[2])


class ProductFactory(DS.ProductFactory):
    def __init__(self, spec, i, pools):
        self.spec, self.dp, self.pools, self.made = spec, spec["canaries"][i], pools, []


def with_canaries(spec, pools, entities, ns, factory_cls):
    pools["factory"] = [factory_cls(spec, i, pools) for i in range(len(spec.get("canaries") or []))]
    pools["canary"] = [ns.CanaryDeployer(f"cn{i}", pools["lb"][cn["lb"]], pools["factory"][i],
                                         stages=None if cn["stages"] is None else [ns.CanaryStage(p, t) for p, t in cn["stages"]],
                                         metric_evaluator=make_evaluator(ns, cn["ev"]), evaluation_interval=cn["iv"])
                       for i, cn in enumerate(spec.get("canaries") or [])]
    return entities + pools["canary"]


def schedule_canaries(spec, pools, sim, at):
    for cn, deployer_ in zip(spec.get("canaries") or [], pools["canary"]):
        if cn["deploy"] is not None:
            ev = deployer_.deploy()
            ev.time = at(cn["deploy"])
            sim.schedule(ev)


def build(spec, seed=None, **sim_kw):
    pools, sources, probes, entities = GF.wire(spec, GF.Product, hs)
    entities = with_canaries(spec, pools, entities, hs, ProductFactory)
    start_ns = int(spec.get("start_ns", 0))

    def at(t_s):
        return hs.Instant(start_ns + hs.Instant.from_seconds(t_s).nanoseconds)

    fs, handles = GF.make_schedule(hs, spec, pools)
    early = GF.early_starts(spec, pools)
    sim = hs.Simulation(sources=sources, entities=entities, seed=spec["seed"] if seed is None else seed, max_graph_events=400_000,
                        fault_schedule=fs, **({} if spec.get("auto") else {"end_time": at(spec["end_s"])}),
                        **({"start_time": hs.Instant(start_ns)} if start_ns else {}), **({"probes": [p for p, _ in probes]} if probes else {}),
                        **sim_kw)
    GF.cancel_after(spec, handles)
    GF.schedule_all(spec, pools, sim, hs.Event, at, early)
    schedule_canaries(spec, pools, sim, at)
    pools["probes"] = probes
    pools["fault_schedule"], pools["handles"] = fs, handles
    return sim, pools


def canary_state(pools):
    """The object state of every canary deployer, its LoadBalancer's membership and the strategy's weights, as arrays and names."""
    rows, floats, members, baseline, weights = [], [], [], [], []
    for cn in pools["canary"]:
        st, s = cn.stats, cn.state
        rows.append([st.deployments_started, st.deployments_completed, st.deployments_rolled_back, st.stages_completed,
                     st.evaluations_performed, st.evaluations_passed, st.evaluations_failed, STATUS[s.status], s.current_stage, s.total_stages,
                     int(cn.canary is not None), -1 if cn._stage_start_time is None else cn._stage_start_time.nanoseconds])
        floats.append(float(s.canary_traffic_pct))
        members.append([b.name for b in cn._load_balancer.all_backends])
        baseline.append([b.name for b in cn._baseline_backends])
        weights.append(sorted([k, int(v)] for k, v in getattr(cn._load_balancer.strategy, "_weights", {}).items()))
    return dict(cn_state=np.asarray(rows, np.int64).reshape(-1, 12), cn_traffic_pct=np.asarray(floats, np.float64), cn_members=members,
                cn_baseline=baseline, cn_weights=weights)


def window_states(states):
    return dict(window_cn_state=np.stack([s["cn_state"] for s in states]), window_cn_traffic_pct=np.stack([s["cn_traffic_pct"] for s in states]),
                window_cn_members=[s["cn_members"] for s in states], window_cn_weights=[s["cn_weights"] for s in states])


def canary_results(spec, pools):
    out = canary_state(pools)
    downstream, inst_rows, inst_service, member_info, current, names = [], [], [], [], [], []
    for cn, factory in zip(pools["canary"], pools["factory"]):
        lb_ = cn._load_balancer
        downstream.append([s.name for s in cn.downstream_entities()])
        names.append(None if cn.canary is None else cn.canary.name)
        for s in factory.made[:int(cn.canary is not None)]:
            inst_rows.append([s.stats_accepted, s.stats_dropped, s._requests_completed, s._requests_rejected, s.depth, s.active_requests])
            inst_service.append(s._total_service_time)
        member_info.append([[b.name, int(lb_._backends[b.name].total_requests), int(lb_._backends[b.name].weight)] for b in lb_.all_backends])
        current.append(sorted([k, int(v)] for k, v in getattr(lb_.strategy, "_current_weights", {}).items()))
    out["cn_downstream"], out["cn_canary_name"] = downstream, names
    out["cn_instance_stats"] = np.asarray(inst_rows, np.int64).reshape(-1, 6)
    out["cn_instance_service_s"] = np.asarray(inst_service, np.float64)
    out["cn_member_info"], out["cn_current_weights"] = member_info, current
    return out


def results(spec, sim, pools):
    with DS.tolerant(pools["lb"]):
        out = MX.results(spec, sim, pools)
        tot, off = [], [0]
        for j, lb_ in enumerate(pools["lb"]):
            tot.extend(lb_.get_backend_info(pools["server"][b]).total_requests for b in spec["lbs"][j]["backends"])
            off.append(len(tot))
    out["lb_backend_total_requests"], out["lb_backend_off"] = np.asarray(tot, np.int64), np.asarray(off, np.int64)
    out.update(canary_results(spec, pools))
    out["autoscaler_by_kind"] = np.zeros(1, np.int64)
    out["deployer_by_kind"] = np.asarray(getattr(sim, "_deployer_by_kind", np.zeros(len(DS.RD_EVENTS))), np.int64)
    out["canary_by_kind"] = np.asarray(getattr(sim, "_canary_by_kind", np.zeros(len(CN_EVENTS))), np.int64)
    return out


WINDOW_KEYS = {"window_cn_state", "window_cn_traffic_pct", "window_cn_members", "window_cn_weights"}
NOT_COMPARED = MX.NOT_COMPARED | WINDOW_KEYS | {"python"}
BY_KIND_SLICES = DS.BY_KIND_SLICES + [("canary_by_kind", N_KINDS)]


def compare(name, got, ref):
    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    sim, pools = build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, bool(spec.get("auto")))
    eng = GraphEngine(g.arrays, seed=spec["seed"], start_ns=start_ns, **caps)
    eng.add_faults(sim._general_faults(g))
    for entry in sched:
        eng.schedule(*entry)
    return sim, pools, g, eng, end_ns, start_ns, cancelled


def engine_run(spec, ends_s, **caps):
    sim, pools, g, eng, end_ns, start_ns, cancelled = engine(spec, **caps)
    with eng:
        for t in ends_s:
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    return sim, pools


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def fleet(name, cn, strategy="wrr", n_init=3, mean=0.05, c=1, cap=None, svc="exp", sources=None, end_s=8.0, seed=11, **kw):
    """Source(s) -> LoadBalancer over `n_init` Servers with a canary deployer -> Sink."""
    kw.setdefault("canaries", [cn])
    return _g(name, servers=[srv(mean, c, cap, svc=svc) for _ in range(n_init)], lbs=[lb(strategy, range(n_init))],
              sources=DS.traffic() if sources is None else sources, end_s=end_s, seed=seed, **kw)


def _fixtures():
    f = []
    slow = [src(LB0, 4.0, "poisson")]
    # ---- the reference's defaults (four stages of 30 s, every 5 s) to the promotion, the weights written at every stage
    f.append(fleet("default_stages_to_promotion_wrr", canary(stages=None, iv=5.0, deploy=1.0), strategy="wrr", sources=slow, end_s=130.0, traced=True))
    f.append(fleet("default_stages_to_promotion_wlc", canary(stages=None, iv=5.0, deploy=1.0), strategy="wlc", sources=slow, end_s=130.0, seed=12))
    f.append(fleet("quick_stages_to_promotion_wrr", canary(), strategy="wrr", seed=13, traced=True))
    f.append(fleet("quick_stages_to_promotion_wlc", canary(), strategy="wlc", seed=14, traced=True))
    # RoundRobin / LeastConnections have no set_weight: _set_traffic_weight and _reset_weights are no-ops
    f.append(fleet("round_robin_weights_are_a_no_op", canary(), strategy="round_robin", seed=15, traced=True))
    f.append(fleet("least_conn_weights_are_a_no_op", canary(), strategy="least_conn", seed=16))
    # ---- the evaluators
    f.append(fleet("latency_evaluator_rolls_a_slow_canary_back", canary(ev=["latency", 1.0, 1.5], mean=0.12), seed=17, traced=True))
    f.append(fleet("latency_evaluator_passes_a_like_canary", canary(ev=["latency", 1.0, 5.0]), seed=18))
    f.append(fleet("latency_above_max_latency", canary(ev=["latency", 0.04, 10.0], mean=0.06, svc="const"), svc="const", seed=19))
    # constant 0.1 s against constant 0.15 s and a multiplier of 1.5: sum / count of either side lands one ulp above or below, so the
    # comparison is decided by the order of the roundings
    f.append(fleet("latency_within_an_ulp_of_the_threshold", canary(ev=["latency", 1.0, 1.5], mean=0.15, svc="const", stages=[[0.25, 2.0], [0.5, 2.0]]),
                   mean=0.1, svc="const", sources=[src(LB0, 12.0, "constant")], seed=20, traced=True))
    # rejections: concurrency 1 Servers refuse what arrives while they serve (the queue hands them on all the same under a bounded queue)
    f.append(fleet("error_rate_evaluator_default", canary(ev=None, c=1, cap=0), cap=0, sources=DS.traffic(40.0), seed=21, traced=True))
    f.append(fleet("error_rate_evaluator_strict", canary(ev=["error", 0.0, 1.0], c=1, cap=2), cap=2, c=1, sources=DS.traffic(60.0), seed=22))
    # ---- stage timing: a period shorter than, and no multiple of, the interval
    f.append(fleet("period_shorter_than_the_interval", canary(stages=[[0.1, 0.2], [0.5, 0.3]], iv=0.5), seed=23, traced=True))
    f.append(fleet("period_no_multiple_of_the_interval", canary(stages=[[0.1, 0.7], [0.6, 1.1], [1.0, 0.0]], iv=0.5), seed=24, traced=True))
    f.append(fleet("percentage_at_and_beyond_one", canary(stages=[[1.0, 0.5], [1.5, 0.5], [0.0, 0.5], [-0.5, 0.5]]), seed=25))
    f.append(fleet("no_baseline_at_all", canary(), n_init=0, seed=26))
    f.append(fleet("one_stage", canary(stages=[[0.5, 1.0]]), strategy="wlc", n_init=1, seed=27))
    f.append(fleet("never_deployed", canary(deploy=None), seed=28))
    f.append(fleet("crashed_canary_deployer", canary(), faults=[crash(K0, 1.1, 2.7)], seed=29, traced=True))
    f.append(fleet("paused_canary_deployer", canary(), faults=[pause(K0, 0.9, 2.2)], seed=30))
    f.append(fleet("crashed_baseline_backend", canary(), faults=[crash(["server", 0], 1.0, 2.5)], seed=31))
    f.append(_g("end_time_infinity_ends_with_the_promotion", servers=[srv(0.05), srv(0.05)], lbs=[lb("wrr", [0, 1])], sources=[],
                schedule=plain(LB0, *[round(0.1 * k, 2) for k in range(40)]), canaries=[canary()], auto=True, end_s=60.0, seed=32, traced=True))
    f.append(fleet("removed_baseline_finishes_its_queue", canary(stages=[[0.5, 0.25]], iv=0.25, mean=0.02), mean=0.3, svc="const",
                   sources=[src(LB0, 12.0, "constant")], seed=33, traced=True))
    f.append(fleet("later_start_time", canary(), start_ns=5 * 10 ** 9, seed=34))
    f.append(_g("canary_next_to_a_rolling_free_load_balancer", servers=[srv(0.05), srv(0.05), srv(0.04, c=2)], lbs=[lb("wrr", [0, 1]), lb("wlc", [2])],
                sources=DS.traffic() + DS.traffic(15.0, LB1), canaries=[canary(), canary(lb=1, ev=["latency", 1.0, 1.2], c=2)], end_s=6.0, seed=35))
    f.append(fleet("sixty_six_baselines_promoted", canary(stages=[[0.5, 0.5]], mean=0.3), strategy="wlc", n_init=66, mean=0.3, sources=DS.traffic(100.0),
                   end_s=2.0, seed=36))
    by_name = {s["name"]: s for s in f}
    for base, windows in (("quick_stages_to_promotion_wrr", [0.5, 1.0, 1.6, 2.5, 2.5, 3.6, 4.6]), ("quick_stages_to_promotion_wlc", [0.75, 2.0, 3.0, 4.5]),
                          ("latency_evaluator_rolls_a_slow_canary_back", [0.75, 1.0, 1.5])):
        f.append(dict(by_name[base], name=base + "_in_windows", traced=False, windows=windows))
    for s in f:
        s.setdefault("traced", False)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    rng = np.random.default_rng(411_000 + k)
    strat = STRATEGIES[int(rng.integers(0, 4))]
    n_init, c = int(rng.integers(0, 5)), int(rng.integers(1, 3))
    mean = float(np.round(rng.uniform(0.02, 0.12), 3))
    end = float(rng.choice([3.0, 4.0, 5.0]))
    stages = [[float(rng.choice([0.01, 0.05, 0.1, 0.25, 0.5, 0.99, 1.0])), float(rng.choice([0.0, 0.3, 0.5, 0.75, 1.0]))] for _ in range(int(rng.integers(1, 5)))]
    which = int(rng.integers(0, 3))
    ev = None if which == 0 else ["latency", float(rng.choice([0.05, 0.2, 1.0])), float(rng.choice([1.0, 1.1, 1.5]))] if which == 1 else [
        "error", float(rng.choice([0.0, 0.05, 0.3])), float(rng.choice([1.0, 2.0]))]
    cap = None if rng.random() < 0.5 else int(rng.integers(0, 3))
    cn = canary(stages=stages, ev=ev, iv=float(rng.choice([0.25, 0.5, 0.75])), deploy=float(np.round(rng.uniform(0.0, end * 0.5), 2)),
                mean=float(np.round(mean * rng.choice([0.8, 1.0, 1.0, 1.3, 2.0]), 3)), c=c, cap=cap, svc="const" if rng.random() < 0.3 else "exp")
    sources = [src(LB0, float(rng.choice([10.0, 20.0, 40.0])), "constant" if k % 3 == 0 else "poisson")]
    faults = []
    if k % 4 == 1:
        on = K0 if rng.random() < 0.5 or n_init == 0 else ["server", int(rng.integers(0, n_init))]
        at = float(np.round(rng.uniform(0.2, end), 2))
        faults.append(crash(on, at, None if rng.random() < 0.3 else float(np.round(rng.uniform(at, end), 2))) if rng.random() < 0.6 else
                      pause(on, at, float(np.round(rng.uniform(at, end), 2))))
    return fleet(f"canary_graph_{k}", cn, strategy=strat, n_init=n_init, mean=mean, c=c, cap=cap, svc="const" if rng.random() < 0.2 else "exp",
                 sources=sources, faults=faults, end_s=end, seed=int(rng.integers(1, 10_000)))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="canary_groups", end_s=3.0):
    servers, lbs, sources, canaries = [], [], [], []
    for g in range(n_groups):
        servers += [srv(0.04 + 0.01 * (g % 3), 1 + g % 2, out=["sink", g]), srv(0.05, 1, out=["sink", g])]
        lbs.append(lb(STRATEGIES[g % 4], [2 * g, 2 * g + 1]))
        sources.append(src(["lb", g], 15.0 + g % 7, "poisson"))
        canaries.append(canary(stages=[[0.1, 0.5], [0.5, 0.5]], ev=None if g % 2 else ["latency", 1.0, 1.0 + 0.25 * (g % 3)], iv=0.25,
                               deploy=0.25 + 0.1 * (g % 4), lb=g, mean=0.05, c=1 + g % 2, out=["sink", g]))
    return _g(name, servers=servers, lbs=lbs, sources=sources, n_sinks=n_groups, canaries=canaries, end_s=end_s, seed=61)


def recorded_specs():
    return all_specs() + [groups_spec(16)]
