"""Specs of the RollingDeployer (happy_simulator_amd.entities; the reference's components/deployment/rolling_deployer.py) over a
LoadBalancer of the single-heap loop.  The format is the mixed family's (tests/mixed_specs.py, tests/graph_family.py) with one addition:

  deployers = [dict(lb=j, batch=, iv=, thr=, fails=, deploys=[t_s, ...], inst=dict(mean=, c=, cap=, svc=, out=pool ref))]
      RollingDeployer(f"rd{i}", LoadBalancer j, factory, batch_size=batch, health_check_interval=iv, healthy_threshold=thr,
      max_failures=fails); the factory builds instance k = Server(f"rd{i}_v2_{k}") as `inst` says, with SERVICE stream base
      len(spec["servers"]) + k - 1.  The deployers stand behind every other entity in `entities=[...]`; behind the spec's own
      schedule every deployer's deploy() Event is scheduled once per entry of `deploys`, at that time (seconds behind the start).
  a fault may name ["deployer", i];  auto=True: end_time = Infinity (the deployer's Events are no daemons: the run ends when they do).

`build()` wires the product; tests/golden/make_golden_deployers.py hands the same functions the reference's classes and records every
spec listed here as family "deployer": what the "mixed" family records, eight more by_kind rows (39: `_autoscaler_evaluate`, always 0;
40 .. 46: the deployer's seven Events) and deployer_results below.  DEPLOYERS reads the recordings back.  Every case has at most
20 000 Events.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs: Source(s) -> deployed LoadBalancer of any of the four strategies -> Sink
  groups_spec(n)  n disconnected deployed chains: the parts of hs_graph_run_parts
"""
import contextlib

import numpy as np

import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import mixed_specs as MX
from happy_simulator_amd.graph_engine import GraphEngine
from recorded import Recorded

DEPLOYERS = Recorded("live_deployers", "deployer", "make_golden_deployers.py", part_bytes=640 * 1024, max_part_bytes=900 * 1024)
N_RANDOM = 100
EV_AS_EVAL = 39                                # the by_kind row of `_autoscaler_evaluate` (behind record_family.EV's 39): always 0 here
EV_RD_FIRST = 40                               # ... and of `_rolling_deploy_start`, the first of the deployer's seven
RD_EVENTS = ("_rolling_deploy_start", "_rolling_replace_batch", "_rolling_health_check", "_rolling_health_pass", "_rolling_health_timeout",
             "_rolling_rollback", "_rolling_complete")
N_KINDS = EV_RD_FIRST + len(RD_EVENTS)
crash, pause = MX.crash, MX.pause
src, plain, srv, lb = MX.src, MX.plain, MX.srv, MX.lb
SINK, LB0, LB1, D0 = ["sink", 0], ["lb", 0], ["lb", 1], ["deployer", 0]
STRATEGIES = ("round_robin", "wrr", "least_conn", "wlc")
STATUS = {"idle": 0, "in_progress": 1, "completed": 2, "rolled_back": 3}
_g = MX._g


def inst(mean=0.05, c=1, cap=None, svc="exp", out=SINK):
    return dict(mean=mean, c=c, cap=cap, svc=svc, out=None if out is None else list(out))


def deployer(batch=1, iv=0.5, thr=2, fails=1, deploys=(0.5,), lb=0, **instance):  # noqa: A002
    return dict(lb=lb, batch=batch, iv=iv, thr=thr, fails=fails, deploys=[float(t) for t in deploys], inst=inst(**instance))


class ProductFactory:
    """`server_factory` of deployer i over the product's classes; `made`: every Server it built, in call order."""

    def __init__(self, spec, i, pools):
        self.spec, self.dp, self.pools, self.made = spec, spec["deployers"][i], pools, []

    def __call__(self, name):
        v = self.dp["inst"]
        out = None if v["out"] is None else self.pools[v["out"][0]][v["out"][1]]
        service = hs.ConstantLatency(v["mean"]) if v["svc"] == "const" else hs.ExponentialLatency(v["mean"])
        server = hs.Server(name, concurrency=v["c"], queue_capacity=v["cap"], service_time=service, downstream=out)
        self.made.append(server)
        return server


def with_deployers(spec, pools, entities, ns, factory_cls):
    """wire()'s entity list with the spec's deployers behind it; pools["deployer"] holds the deployers, pools["factory"] their
    factories."""
    pools["factory"] = [factory_cls(spec, i, pools) for i in range(len(spec.get("deployers") or []))]
    pools["deployer"] = [ns.RollingDeployer(f"rd{i}", pools["lb"][dp["lb"]], pools["factory"][i], batch_size=dp["batch"],
                                            health_check_interval=dp["iv"], healthy_threshold=dp["thr"], max_failures=dp["fails"])
                         for i, dp in enumerate(spec.get("deployers") or [])]
    return entities + pools["deployer"]


def schedule_deployers(spec, pools, sim, at):
    for dp, deployer_ in zip(spec.get("deployers") or [], pools["deployer"]):
        for t_s in dp["deploys"]:
            ev = deployer_.deploy()
            ev.time = at(t_s)
            sim.schedule(ev)


def build(spec, seed=None, **sim_kw):
    """graph_family.build with the deployers among the entities and their deploy() Events behind the schedule."""
    pools, sources, probes, entities = GF.wire(spec, GF.Product, hs)
    entities = with_deployers(spec, pools, entities, hs, ProductFactory)
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
    schedule_deployers(spec, pools, sim, at)
    pools["probes"] = probes
    pools["fault_schedule"], pools["handles"] = fs, handles
    return sim, pools


class _Gone:
    """What the result readers see of a backend that is no member any more (get_backend_info is None there)."""

    total_requests, is_healthy = -1, -1


def tolerate_removed(lbs):
    """The other families' result readers ask `get_backend_info(b)` of every backend a spec lists; here a listed backend may have left."""
    for lb_ in lbs:
        lb_.get_backend_info = (lambda f: lambda b: f(b) or _Gone)(type(lb_).get_backend_info.__get__(lb_))


@contextlib.contextmanager
def tolerant(lbs):
    tolerate_removed(lbs)
    try:
        yield
    finally:
        for lb_ in lbs:
            del lb_.get_backend_info


def deployer_state(pools):
    """The object state of every deployer and of its LoadBalancer's membership, as arrays and lists of names."""
    rows, members, lists = [], [], []
    for dp in pools["deployer"]:
        st, s = dp.stats, dp.state
        rows.append([st.deployments_started, st.deployments_completed, st.deployments_rolled_back, st.instances_replaced,
                     st.health_checks_performed, st.health_checks_passed, st.health_checks_failed, STATUS[s.status], s.total_instances,
                     s.replaced, s.failed, s.current_batch, dp._next_instance_id, dp._health_fail_count])
        members.append([b.name for b in dp._load_balancer.all_backends])
        lists.append([[b.name for b in ls] for ls in (dp._old_backends, dp._new_backends, dp._current_batch_old, dp._current_batch_new)])
    return dict(rd_state=np.asarray(rows, np.int64).reshape(-1, 14), rd_members=members, rd_lists=lists)


def window_states(states):
    return dict(window_rd_state=np.stack([s["rd_state"] for s in states]), window_rd_members=[s["rd_members"] for s in states],
                window_rd_lists=[s["rd_lists"] for s in states])


def deployer_results(spec, pools):
    """What both libraries' deployers, their LoadBalancers and the instances they activated show after a run."""
    out = deployer_state(pools)
    passes, downstream, info, inst_rows, inst_service, inst_off, weights, current, member_info = [], [], [], [], [], [0], [], [], []
    for dp, factory in zip(pools["deployer"], pools["factory"]):
        lb_ = dp._load_balancer
        passes.append([[k, int(v)] for k, v in dp._health_pass_count.items()])
        downstream.append([s.name for s in dp.downstream_entities()])
        for s in factory.made[:dp._next_instance_id]:
            bi = type(lb_).get_backend_info(lb_, s)
            info.append(-1 if bi is None else int(bi.total_requests))              # (None for a removed instance)
            inst_rows.append([s.stats_accepted, s.stats_dropped, s._requests_completed, s._requests_rejected, s.depth, s.active_requests])
            inst_service.append(s._total_service_time)
        inst_off.append(len(inst_rows))
        member_info.append([[b.name, int(lb_._backends[b.name].total_requests), int(lb_._backends[b.name].weight)] for b in lb_.all_backends])
        st = lb_.strategy
        weights.append(sorted([k, int(v)] for k, v in getattr(st, "_weights", {}).items()))
        current.append(sorted([k, int(v)] for k, v in getattr(st, "_current_weights", {}).items()))
    out["rd_pass_count"], out["rd_downstream"] = passes, downstream
    out["rd_instance_total_requests"] = np.asarray(info, np.int64)
    out["rd_instance_stats"], out["rd_instance_off"] = np.asarray(inst_rows, np.int64).reshape(-1, 6), np.asarray(inst_off, np.int64)
    out["rd_instance_service_s"] = np.asarray(inst_service, np.float64)
    out["rd_member_info"] = member_info
    out["rd_strategy_weights"], out["rd_current_weights"] = weights, current
    return out


def results(spec, sim, pools):
    """Everything the recorder records for "deployer" except the trace, read off the product's objects after run()."""
    with tolerant(pools["lb"]):
        out = MX.results(spec, sim, pools)
        # (per backend the spec lists, as the recorder reads them; -1: it is no member any more)
        tot, off = [], [0]
        for j, lb_ in enumerate(pools["lb"]):
            tot.extend(lb_.get_backend_info(pools["server"][b]).total_requests for b in spec["lbs"][j]["backends"])
            off.append(len(tot))
    out["lb_backend_total_requests"], out["lb_backend_off"] = np.asarray(tot, np.int64), np.asarray(off, np.int64)
    out.update(deployer_results(spec, pools))
    out["autoscaler_by_kind"] = np.zeros(1, np.int64)
    out["deployer_by_kind"] = np.asarray(getattr(sim, "_deployer_by_kind", np.zeros(len(RD_EVENTS))), np.int64)
    return out


WINDOW_KEYS = {"window_rd_state", "window_rd_members", "window_rd_lists"}
NOT_COMPARED = MX.NOT_COMPARED | WINDOW_KEYS | {"python"}
BY_KIND_SLICES = MX.BY_KIND_SLICES + [("autoscaler_by_kind", EV_AS_EVAL + 1), ("deployer_by_kind", N_KINDS)]


def compare(name, got, ref):
    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    """family_checks.engine over build() above."""
    sim, pools = build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, bool(spec.get("auto")))   # (Infinity: a horizon nothing reaches)
    eng = GraphEngine(g.arrays, seed=spec["seed"], start_ns=start_ns, **caps)
    eng.add_faults(sim._general_faults(g))
    for entry in sched:
        eng.schedule(*entry)
    return sim, pools, g, eng, end_ns, start_ns, cancelled


def engine_run(spec, ends_s, **caps):
    """engine(spec), run to every end of `ends_s` in turn (None: the spec's own end); the results bound like Simulation.run() binds them."""
    sim, pools, g, eng, end_ns, start_ns, cancelled = engine(spec, **caps)
    with eng:
        for t in ends_s:
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    return sim, pools


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def traffic(rate=20.0, to=LB0, kind="poisson"):
    return [src(to, rate, kind)]


def fleet(name, dp, strategy="round_robin", n_init=3, mean=0.05, c=1, cap=None, svc="exp", sources=None, end_s=8.0, seed=11, **kw):
    """Source(s) -> LoadBalancer over `n_init` Servers, replaced by `dp` -> Sink."""
    kw.setdefault("deployers", [dp])
    return _g(name, servers=[srv(mean, c, cap, svc=svc) for _ in range(n_init)], lbs=[lb(strategy, range(n_init))],
              sources=traffic() if sources is None else sources, end_s=end_s, seed=seed, **kw)


def _fixtures():
    f = []
    # ---- batch sizes against the backend count; healthy_threshold 1 costs no failure, 2 costs one per instance
    f.append(fleet("batch_1_threshold_1_completes", deployer(batch=1, thr=1), traced=True))
    f.append(fleet("batch_1_threshold_2_one_failure_per_instance", deployer(batch=1, thr=2, fails=3), seed=12, traced=True))
    f.append(fleet("batch_2_threshold_1", deployer(batch=2, thr=1), seed=13, traced=True))
    f.append(fleet("batch_equal_to_the_backend_count", deployer(batch=3, thr=1), seed=14))
    f.append(fleet("batch_above_the_backend_count", deployer(batch=5, thr=1), seed=15, traced=True))
    # the reference's defaults but for the interval: two instances, one failure each in their first round, 2 > max_failures = 1
    f.append(fleet("default_settings_batch_2_rolls_back", deployer(batch=2, thr=2, fails=1), seed=16, traced=True))
    f.append(fleet("default_settings_batch_1_rolls_back_at_the_second_batch", deployer(batch=1, thr=2, fails=1), seed=17))
    # the rollback comes behind a second health check of the same nanosecond: its passes complete the batch (the whole fleet),
    # _replace_batch finds nothing left and the deployment ends "completed" behind "rolled_back"
    f.append(fleet("rollback_with_a_pass_in_flight_walks_on_to_completed", deployer(batch=3, thr=2, fails=1), seed=18, traced=True))
    f.append(fleet("rollback_then_the_batch_completes_and_stalls", deployer(batch=2, thr=2, fails=1), n_init=4, seed=19))
    # a second deployment resets _health_pass_count: pending timeouts of the first count as failures
    f.append(fleet("second_deploy_behind_the_first", deployer(batch=3, thr=1, deploys=(0.5, 4.0)), seed=20, traced=True))
    f.append(fleet("second_deploy_inside_the_first", deployer(batch=1, thr=1, deploys=(0.5, 1.25)), seed=21, traced=True))
    f.append(fleet("second_deploy_fails_the_pending_timeouts_of_the_first", deployer(batch=1, thr=1, fails=0, deploys=(0.5, 1.0)), n_init=2,
                   seed=22, traced=True))
    f.append(fleet("three_deploys", deployer(batch=2, thr=1, fails=2, deploys=(0.25, 1.0, 1.0)), n_init=2, seed=23))
    # the rollback takes the new instances, the passes in flight take the old ones: no member is left and every Request fails
    f.append(fleet("rollback_leaves_the_load_balancer_empty_under_traffic", deployer(batch=2, thr=2, fails=1), strategy="wrr", n_init=2,
                   seed=24, traced=True))
    f.append(fleet("second_deploy_over_a_single_backend_rolls_back", deployer(batch=1, thr=1, fails=0, deploys=(0.5, 1.5)), n_init=1, seed=31))
    f.append(fleet("no_backends_at_all", deployer(batch=1, thr=1), n_init=0, seed=25))
    # a full queue refuses the probe: it passes all the same
    f.append(fleet("full_queue_refuses_a_probe", deployer(batch=1, thr=2, fails=5, mean=0.4, cap=0, svc="const"), mean=0.4, svc="const",
                   sources=traffic(30.0, kind="constant"), seed=26, traced=True))
    f.append(fleet("crashed_deployer", deployer(batch=1, thr=2, fails=9), faults=[crash(D0, 1.1, 2.7)], seed=27, traced=True))
    f.append(fleet("paused_deployer", deployer(batch=1, thr=2, fails=9), faults=[pause(D0, 0.9, 2.2)], seed=28))
    f.append(fleet("crashed_new_instance_never_passes", deployer(batch=1, thr=1, fails=2), faults=[crash(["server", 0], 0.1, 0.2)], seed=29))
    f.append(_g("end_time_infinity_ends_with_the_deployment", servers=[srv(0.05), srv(0.05)], lbs=[lb("round_robin", [0, 1])], sources=[],
                schedule=plain(LB0, *[round(0.1 * k, 2) for k in range(30)]), deployers=[deployer(batch=1, thr=2, fails=4)], auto=True,
                end_s=60.0, seed=30, traced=True))
    # ---- the four strategies over a member list that loses its initial backends
    for k, strat in enumerate(STRATEGIES):
        f.append(fleet(f"{strat}_completes", deployer(batch=1 + k % 2, thr=1, c=1 + k % 2), strategy=strat, c=1 + k % 2, seed=40 + k,
                       traced=strat in ("wrr", "wlc")))
        f.append(fleet(f"{strat}_rolls_back", deployer(batch=2, thr=2, fails=1), strategy=strat, seed=44 + k))
        f.append(fleet(f"{strat}_two_deploys", deployer(batch=2, thr=1, fails=1, deploys=(0.5, 1.0)), strategy=strat, n_init=4, seed=48 + k))
    # ---- removed backends finish what they hold: slow initial Servers, removed with work in their queues
    f.append(fleet("removed_initial_backend_finishes_its_queue", deployer(batch=3, thr=1, iv=0.25, mean=0.02), mean=0.3, svc="const",
                   sources=traffic(12.0, kind="constant"), seed=52, traced=True))
    f.append(fleet("slow_interval_health_checks_multiply", deployer(batch=3, thr=3, fails=20, iv=0.4), seed=53))
    f.append(fleet("later_start_time", deployer(batch=2, thr=1), start_ns=5 * 10 ** 9, seed=54))
    f.append(_g("two_deployed_load_balancers", servers=[srv(0.05), srv(0.05), srv(0.04, c=2)], lbs=[lb("round_robin", [0, 1]), lb("wlc", [2])],
                sources=traffic() + traffic(15.0, LB1), deployers=[deployer(batch=1, thr=1), deployer(batch=1, thr=2, fails=1, lb=1, c=2)],
                end_s=6.0, seed=55))
    f.append(fleet("sixty_six_members_one_batch", deployer(batch=66, thr=1, iv=0.5, mean=0.3), strategy="least_conn", n_init=66, mean=0.3,
                   sources=traffic(100.0), end_s=2.0, seed=56))
    # ---- windows variants (the reference runs them in the same windows)
    by_name = {s["name"]: s for s in f}
    for base, windows in (("batch_1_threshold_2_one_failure_per_instance", [0.5, 1.0, 1.3, 2.5, 2.5, 4.0]),
                          ("second_deploy_fails_the_pending_timeouts_of_the_first", [0.75, 1.0, 1.5, 2.0]), ("wrr_two_deploys", [1.0, 2.0, 3.25])):
        f.append(dict(by_name[base], name=base + "_in_windows", traced=False, windows=windows))
    for s in f:
        s.setdefault("traced", False)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """One or two Sources -> a LoadBalancer of a drawn strategy over 1 .. 4 Servers, replaced by a drawn deployer -> Sink; every fourth
    spec has a fault on the deployer or on a backend, every third constant Sources."""
    rng = np.random.default_rng(311_000 + k)
    strat = STRATEGIES[int(rng.integers(0, 4))]
    n_init, c = int(rng.integers(1, 5)), int(rng.integers(1, 3))
    mean = float(np.round(rng.uniform(0.02, 0.12), 3))
    end = float(rng.choice([3.0, 4.0, 5.0]))
    n_deploys = 1 if rng.random() < 0.6 else 2
    deploys = sorted(float(np.round(rng.uniform(0.0, end * 0.6), 2)) for _ in range(n_deploys))
    dp = deployer(batch=int(rng.integers(1, 4)), iv=float(rng.choice([0.25, 0.5, 0.75])), thr=int(rng.integers(1, 4)), fails=int(rng.integers(0, 5)),
                  deploys=deploys, mean=mean, c=c, cap=None if rng.random() < 0.7 else int(rng.integers(0, 3)),
                  svc="const" if rng.random() < 0.2 else "exp")
    constant = k % 3 == 0
    sources = [src(LB0, float(rng.choice([10.0, 20.0, 30.0])), "constant" if constant else "poisson")]
    if rng.random() < 0.4:
        sources.append(src(LB0, float(rng.choice([2.0, 5.0])), "poisson"))
    faults = []
    if k % 4 == 1:
        on = D0 if rng.random() < 0.5 else ["server", int(rng.integers(0, n_init))]
        at = float(np.round(rng.uniform(0.2, end), 2))
        faults.append(crash(on, at, None if rng.random() < 0.3 else float(np.round(rng.uniform(at, end), 2))) if rng.random() < 0.6 else
                      pause(on, at, float(np.round(rng.uniform(at, end), 2))))
    return fleet(f"deployer_graph_{k}", dp, strategy=strat, n_init=n_init, mean=mean, c=c, sources=sources, faults=faults, end_s=end,
                 seed=int(rng.integers(1, 10_000)))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="deployer_groups", end_s=3.0):
    """`n_groups` disconnected Source -> deployed LoadBalancer -> Sink chains in ONE Simulation: the parts of hs_graph_run_parts (a pool
    belongs to the part of its LoadBalancer)."""
    servers, lbs, sources, deployers = [], [], [], []
    for g in range(n_groups):
        servers += [srv(0.04 + 0.01 * (g % 3), 1 + g % 2, out=["sink", g]), srv(0.05, 1, out=["sink", g])]
        lbs.append(lb(STRATEGIES[g % 4], [2 * g, 2 * g + 1]))
        sources.append(src(["lb", g], 15.0 + g % 7, "poisson"))
        deployers.append(deployer(batch=1 + g % 2, thr=1 + g % 2, fails=1 + g % 3, iv=0.25, deploys=(0.25 + 0.1 * (g % 4),), lb=g, mean=0.04,
                                  c=1 + g % 2, out=["sink", g]))
    return _g(name, servers=servers, lbs=lbs, sources=sources, n_sinks=n_groups, deployers=deployers, end_s=end_s, seed=61)


def recorded_specs():
    """Everything make_golden_deployers.py records: the fixtures, the random graphs and the groups."""
    return all_specs() + [groups_spec(16)]
