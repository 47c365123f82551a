"""Specs of the AutoScaler (happy_simulator_amd.entities; the reference's components/deployment/auto_scaler.py) over a LoadBalancer of
the single-heap loop.  The format is the mixed family's (tests/mixed_specs.py, tests/graph_family.py) with two additions:

  scalers = [dict(lb=j, policy=["tu", target] | ["step", [[threshold, adjustment], ...]] | ["qd", out, in], lo=, hi=, iv=, out_cd=,
                  in_cd=, starts=1, stop=False, inst=dict(mean=, c=, cap=, svc=, out=pool ref, qp=None | ["lifo", cap]))]
      AutoScaler(f"as{i}", LoadBalancer j, factory, policy, min_instances=lo, max_instances=hi, evaluation_interval=iv,
      scale_out_cooldown=out_cd, scale_in_cooldown=in_cd); the factory builds instance k = Server(f"as{i}_server_{k}") as `inst` says,
      with SERVICE stream base len(spec["servers"]) + k - 1.  The scalers stand behind every other entity in `entities=[...]`;
      behind the spec's own schedule every scaler is started `starts` times (sim.schedule(scaler.start())) and, with `stop`, stopped.
  scaler_probes = [[i, interval]]: Probe.on(scaler i, "current_count", interval), behind the spec's other probes.
  a fault may name ["scaler", i].

`build()` wires the product; tests/golden/make_golden_autoscaler.py hands the same functions the reference's classes and records every
spec listed here as family "autoscaler": what the "mixed" family records, one more by_kind row (39: `_autoscaler_evaluate`) and
scaler_results below.  AUTOSCALER reads the recordings back.  Every case has at most 10 s of simulated time and at most 20 000 Events.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded graphs: Source(s) -> scaled LoadBalancer of any of the four strategies -> Sink
  groups_spec(n)  n disconnected scaled chains: the parts of hs_graph_run_parts
"""
import numpy as np

import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import mixed_specs as MX
from happy_simulator_amd.graph_engine import GraphEngine
from recorded import Recorded

AUTOSCALER = Recorded("live_autoscaler", "autoscaler", "make_golden_autoscaler.py", part_bytes=640 * 1024, max_part_bytes=900 * 1024)
N_RANDOM = 100
EV_AS_EVAL = 39                                # the by_kind row of `_autoscaler_evaluate` (behind record_family.EV's 39)
crash, pause = MX.crash, MX.pause
src, plain, srv, link, bh, cl, fixed, gt, gate_events, lb = MX.src, MX.plain, MX.srv, MX.link, MX.bh, MX.cl, MX.fixed, MX.gt, MX.gate_events, MX.lb
SINK, LB0, LB1, C0, W0, F0, A0 = ["sink", 0], ["lb", 0], ["lb", 1], ["client", 0], ["wrapper", 0], ["flow", 0], ["scaler", 0]
STRATEGIES = ("round_robin", "wrr", "least_conn", "wlc")
ACTIONS = {None: 0, "scale_out": 1, "scale_in": 2}
_g = MX._g


def inst(mean=0.08, c=1, cap=None, svc="exp", out=SINK, qp=None):
    return dict(mean=mean, c=c, cap=cap, svc=svc, out=None if out is None else list(out), qp=qp)


def scaler(policy, lo=1, hi=4, iv=0.5, out_cd=0.0, in_cd=0.0, lb=0, starts=1, stop=False, **instance):  # noqa: A002
    return dict(lb=lb, policy=list(policy), lo=lo, hi=hi, iv=iv, out_cd=out_cd, in_cd=in_cd, starts=starts, stop=stop, inst=inst(**instance))


def make_policy(ns, pol):
    if pol[0] == "tu":
        return ns.TargetUtilization(target=pol[1])
    if pol[0] == "step":
        return ns.StepScaling([tuple(s) for s in pol[1]])
    if pol[0] == "qd":
        return ns.QueueDepthScaling(scale_out_threshold=pol[1], scale_in_threshold=pol[2])
    return None                                                  # (the constructor's default)


class ProductFactory:
    """`server_factory` of scaler i over the product's classes; `made`: every Server it built, in call order."""

    def __init__(self, spec, i, pools):
        self.spec, self.sc, self.pools, self.made = spec, spec["scalers"][i], pools, []

    def __call__(self, name):
        v = self.sc["inst"]
        out = None if v["out"] is None else self.pools[v["out"][0]][v["out"][1]]
        service = hs.ConstantLatency(v["mean"]) if v["svc"] == "const" else hs.ExponentialLatency(v["mean"])
        if v.get("qp"):
            server = hs.Server(name, concurrency=v["c"], queue_policy=hs.LIFOQueue() if v["qp"][1] is None else hs.LIFOQueue(capacity=v["qp"][1]),
                               service_time=service, downstream=out)
        else:
            server = hs.Server(name, concurrency=v["c"], queue_capacity=v["cap"], service_time=service, downstream=out)
        self.made.append(server)
        return server


def with_scalers(spec, pools, probes, entities, ns, factory_cls, probe_fn):
    """wire()'s probes and entity list with the spec's scalers (and the probes on them) behind them; pools["scaler"] holds the
    scalers, pools["factory"] their factories."""
    pools["factory"] = [factory_cls(spec, i, pools) for i in range(len(spec.get("scalers") or []))]
    pools["scaler"] = [ns.AutoScaler(f"as{i}", pools["lb"][sc["lb"]], pools["factory"][i], make_policy(ns, sc["policy"]), min_instances=sc["lo"],
                                     max_instances=sc["hi"], evaluation_interval=sc["iv"], scale_out_cooldown=sc["out_cd"],
                                     scale_in_cooldown=sc["in_cd"]) for i, sc in enumerate(spec.get("scalers") or [])]
    more = [probe_fn(pools["scaler"][i], "current_count", interval) for i, interval in spec.get("scaler_probes") or []]
    return probes + more, entities + pools["scaler"]


def schedule_scalers(spec, pools, sim):
    for sc, scaler_ in zip(spec.get("scalers") or [], pools["scaler"]):
        for _ in range(sc.get("starts", 1)):
            sim.schedule(scaler_.start())
        if sc.get("stop"):
            scaler_.stop()


def build(spec, seed=None, **sim_kw):
    """graph_family.build with the scalers among the entities and started behind the schedule."""
    pools, sources, probes, entities = GF.wire(spec, GF.Product, hs)
    probes, entities = with_scalers(spec, pools, probes, entities, hs, ProductFactory, GF.Product.probe)
    start_ns = int(spec.get("start_ns", 0))

    def at(t_s):
        return hs.Instant(start_ns + hs.Instant.from_seconds(t_s).nanoseconds)

    fs, handles = GF.make_schedule(hs, spec, pools)
    early = GF.early_starts(spec, pools)
    sim = hs.Simulation(sources=sources, entities=entities, seed=spec["seed"] if seed is None else seed, max_graph_events=400_000,
                        fault_schedule=fs, end_time=at(spec["end_s"]), **({"start_time": hs.Instant(start_ns)} if start_ns else {}),
                        **({"probes": [p for p, _ in probes]} if probes else {}), **sim_kw)
    GF.cancel_after(spec, handles)
    GF.schedule_all(spec, pools, sim, hs.Event, at, early)
    schedule_scalers(spec, pools, sim)
    pools["probes"] = probes
    pools["fault_schedule"], pools["handles"] = fs, handles
    return sim, pools


def scaler_state(pools):
    """The object state of every scaler and of its LoadBalancer's membership, as arrays."""
    rows, members = [], []
    for sc in pools["scaler"]:
        st = sc.stats
        rows.append([st.evaluations, st.scale_out_count, st.scale_in_count, st.instances_added, st.instances_removed, st.cooldown_blocks,
                     sc._next_instance_id, ACTIONS[sc._last_scale_action], -1 if sc._last_scale_time is None else sc._last_scale_time.nanoseconds,
                     int(sc.is_running), sc.current_count, len(sc._managed_servers), len(sc.scaling_history)])
        members.append([b.name for b in sc.load_balancer.all_backends])
    return dict(as_state=np.asarray(rows, np.int64).reshape(-1, 13), as_members=members)


def removal_times(history):
    """{instance id: the time in ns it left its LoadBalancer} of one scaler's history rows (time, action, from_count, to_count): a
    scale-out hands out the next ids, a scale-in takes the newest managed ones."""
    stack, next_id, out = [], 0, {}
    for t, action, c0, c1 in np.asarray(history).tolist():
        for _ in range(abs(c1 - c0)):
            if action == ACTIONS["scale_out"]:
                next_id += 1
                stack.append(next_id)
            else:
                out[stack.pop()] = t
    return out


def window_states(states):
    return dict(window_as_state=np.stack([s["as_state"] for s in states]), window_as_members=[s["as_members"] for s in states])


def scaler_results(spec, pools):
    """What both libraries' scalers, their LoadBalancers and the instances they activated show after a run."""
    out = scaler_state(pools)
    hist, hist_off, reasons, managed, downstream, info, inst_rows, inst_service, inst_off, weights, current = [], [0], [], [], [], [], [], [], [0], [], []
    for sc, factory in zip(pools["scaler"], pools["factory"]):
        lb_ = sc.load_balancer
        for ev in sc.scaling_history:
            hist.append([ev.time.nanoseconds, ACTIONS[ev.action], ev.from_count, ev.to_count])
            reasons.append(ev.reason)
        hist_off.append(len(hist))
        managed.append([s.name for s in sc._managed_servers])
        downstream.append([s.name for s in sc.downstream_entities()])
        activated = factory.made[:sc._next_instance_id]
        for s in activated:
            bi = lb_.get_backend_info(s)
            info.append(-1 if bi is None else int(bi.total_requests))              # (None for a removed instance)
            inst_rows.append([s.stats_accepted, s.stats_dropped, s._requests_completed, s._requests_rejected, s.depth, s.active_requests])
            inst_service.append(s._total_service_time)
        inst_off.append(len(inst_rows))
        st = lb_.strategy
        weights.append(sorted([k, int(v)] for k, v in getattr(st, "_weights", {}).items()))
        current.append([[k, int(v)] for k, v in getattr(st, "_current_weights", {}).items()])
    out["as_history"], out["as_history_off"], out["as_reasons"] = np.asarray(hist, np.int64).reshape(-1, 4), np.asarray(hist_off, np.int64), reasons
    out["as_managed"], out["as_downstream"] = managed, downstream
    out["as_instance_total_requests"] = np.asarray(info, np.int64)
    out["as_instance_stats"], out["as_instance_off"] = np.asarray(inst_rows, np.int64).reshape(-1, 6), np.asarray(inst_off, np.int64)
    out["as_instance_service_s"] = np.asarray(inst_service, np.float64)
    out["as_strategy_weights"], out["as_current_weights"] = weights, current
    return out


def results(spec, sim, pools):
    """Everything the recorder records for "autoscaler" except the trace, read off the product's objects after run()."""
    out = MX.results(spec, sim, pools)
    # (per backend the spec lists, as the recorder reads them: a scaled LoadBalancer's members beyond them are read by scaler_results)
    tot, off = [], [0]
    for j, lb_ in enumerate(pools["lb"]):
        tot.extend(lb_.get_backend_info(pools["server"][b]).total_requests for b in spec["lbs"][j]["backends"])
        off.append(len(tot))
    out["lb_backend_total_requests"], out["lb_backend_off"] = np.asarray(tot, np.int64), np.asarray(off, np.int64)
    out.update(scaler_results(spec, pools))
    out["autoscaler_by_kind"] = np.asarray(getattr(sim, "_autoscaler_by_kind", np.zeros(1)), np.int64)
    return out


WINDOW_KEYS = {"window_as_state", "window_as_members"}
NOT_COMPARED = MX.NOT_COMPARED | WINDOW_KEYS | {"python"}
BY_KIND_SLICES = MX.BY_KIND_SLICES + [("autoscaler_by_kind", EV_AS_EVAL + 1)]


def compare(name, got, ref):
    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    """family_checks.engine over build() above."""
    sim, pools = build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, False)
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
TU, STEP, QD = ["tu", 0.5], ["step", [[0.5, 1], [0.9, 2], [0.0, -1]]], ["qd", 3, 0]


def burst(rate=40.0, stop_s=2.0, low=4.0, to=LB0):
    """A constant Source that stops and a slow Poisson one: load that saturates the pool, then lets it drain."""
    return [src(to, rate, "constant", stop_s), src(to, low, "poisson")]


def pool(name, sc, strategy="round_robin", n_init=1, mean=0.08, c=1, cap=None, svc="exp", sources=None, end_s=5.0, seed=11, **kw):
    """Source(s) -> LoadBalancer over `n_init` Servers, scaled by `sc` -> Sink."""
    kw.setdefault("scalers", [sc])
    return _g(name, servers=[srv(mean, c, cap, svc=svc) for _ in range(n_init)], lbs=[lb(strategy, range(n_init))],
              sources=burst() if sources is None else sources, end_s=end_s, seed=seed, **kw)


def _fixtures():
    f = []
    # ---- each policy scales out under the burst and in again behind it
    f.append(pool("target_utilization_scales_out_and_in", scaler(TU, c=2), c=2, traced=True))
    f.append(pool("step_scaling_scales_out_and_in", scaler(STEP, hi=5), seed=12, traced=True))
    f.append(pool("queue_depth_scales_out_and_in", scaler(QD, mean=0.06), mean=0.06, seed=13, traced=True))
    # ---- the branches of _try_scale_out / _try_scale_in
    f.append(pool("cooldowns_block_scale_out_and_scale_in", scaler(TU, out_cd=1.0, in_cd=2.0, iv=0.25), seed=14, traced=True))
    # min_instances above max_instances: the policy asks for 3, the clamp leaves one to add, then `to_add <= 0`
    f.append(pool("min_above_max_clamps_then_adds_nothing", scaler(TU, lo=3, hi=2), seed=15))
    f.append(pool("initial_count_below_min_instances", scaler(QD, lo=3, hi=5), sources=[src(LB0, 5.0, "poisson")], seed=16))
    f.append(pool("scale_in_with_nothing_managed", scaler(["tu", 1.0], lo=1, hi=3, in_cd=1.0), n_init=3, sources=[src(LB0, 3.0, "poisson")], seed=17, traced=True))
    # a removed instance is in service (depth counts the queue alone): its completion and `_lb_response` come behind the removal
    f.append(pool("removed_instance_completes_work_afterwards", scaler(QD, mean=0.6, svc="const", hi=3), mean=0.6, svc="const",
                  sources=[src(LB0, 10.0, "constant", 1.0), src(LB0, 1.0, "poisson")], end_s=6.0, seed=19, traced=True))
    # out, in, out: the third instance gets a fresh id
    f.append(pool("fresh_id_after_a_scale_in", scaler(TU, hi=3), sources=burst(40.0, 1.5, 2.0), schedule=plain(LB0, *[round(3.0 + 0.01 * k, 2) for k in range(40)]),
                  seed=19, traced=True))
    f.append(pool("stopped_before_the_run", scaler(TU, stop=True), seed=20))
    f.append(pool("started_twice", scaler(TU, starts=2, out_cd=0.0, in_cd=0.5), seed=21, traced=True))
    f.append(pool("started_twice_with_cooldowns", scaler(STEP, starts=2, out_cd=0.5, in_cd=0.5, hi=5), seed=22))
    f.append(pool("crashed_scaler_never_ticks_again", scaler(TU), faults=[crash(A0, 1.1, 2.0)], seed=23, traced=True))
    f.append(pool("paused_scaler", scaler(QD), faults=[pause(A0, 0.9, 1.2)], seed=24))
    f.append(pool("crash_after_the_scale_out", scaler(TU), faults=[crash(A0, 2.6, None)], seed=25))
    # ---- the four strategies over a changing member list
    for k, strat in enumerate(STRATEGIES):
        for j, (pn, pol) in enumerate((("tu", TU), ("step", STEP), ("qd", QD))):
            f.append(pool(f"{strat}_{pn}", scaler(pol, hi=3 + j, c=1 + k % 2), strategy=strat, n_init=1 + (k + j) % 3, c=1 + k % 2, seed=30 + 3 * k + j,
                          traced=(strat, pn) in (("wrr", "tu"), ("wlc", "qd"))))
    # ---- the wide case: the depth sum and the selection cross a wavefront's width
    f.append(pool("sixty_six_members", scaler(QD, hi=68, mean=0.5, iv=0.5), strategy="least_conn", n_init=64, mean=0.5,
                  sources=[src(LB0, 400.0, "constant", 1.0), src(LB0, 20.0, "poisson")], end_s=3.0, seed=45))
    f.append(pool("sixty_five_members_target_utilization", scaler(["tu", 0.3], hi=66, mean=0.4), strategy="wrr", n_init=64, mean=0.4,
                  sources=[src(LB0, 300.0, "constant", 1.0), src(LB0, 10.0, "poisson")], end_s=3.0, seed=46))
    # ---- combinations
    f.append(_g("client_in_front_of_a_server_in_front_of_the_pool", clients=[cl(0, 0.3, fixed(2, 0.1))], servers=[srv(0.005, out=LB0, svc="const"), srv(0.08)],
                lbs=[lb("round_robin", [1])], sources=burst(40.0, 2.0, 4.0, C0), scalers=[scaler(TU)], end_s=5.0, seed=50, traced=True))
    f.append(_g("instances_in_front_of_a_bulkhead", wrappers=[bh(1, 2, 3, 0.2)], servers=[srv(0.05, out=W0), srv(0.02)], lbs=[lb("least_conn", [0])],
                sources=burst(), scalers=[scaler(TU, mean=0.05, out=W0)], end_s=5.0, seed=51))
    f.append(_g("gate_flush_in_front_of_the_pool", flows=[gt(LB0, [(1.0, 1.5), (2.5, 3.0)], False)], servers=[srv(0.06)], lbs=[lb("wlc", [0])],
                sources=[src(F0, 30.0)], schedule=[gate_events(0)], scalers=[scaler(QD, mean=0.06, iv=0.25)], end_s=5.0, seed=52, traced=True))
    f.append(pool("policied_instances", scaler(QD, qp=["lifo", None]), seed=53))
    f.append(pool("bounded_queue_instances", scaler(TU, cap=1, c=1), cap=2, seed=54))
    f.append(pool("probe_on_current_count", scaler(TU), scaler_probes=[[0, 0.25]], probes=[[["server", 0], "depth", 0.5]], seed=55, traced=True))
    f.append(pool("crashed_initial_backend", scaler(TU), strategy="least_conn", n_init=2, faults=[crash(["server", 0], 1.0, 2.5)], seed=56))
    f.append(pool("later_start_time", scaler(STEP, out_cd=0.5), sources=[src(LB0, 30.0, "poisson")], start_ns=5 * 10 ** 9, seed=57))
    f.append(_g("two_scaled_load_balancers", servers=[srv(0.08), srv(0.05, c=2)], lbs=[lb("round_robin", [0]), lb("least_conn", [1])],
                sources=burst() + burst(60.0, 1.5, 3.0, LB1), scalers=[scaler(TU), scaler(QD, lb=1, c=2, mean=0.05)], end_s=5.0, seed=58))
    f.append(pool("ten_seconds_with_default_like_cooldowns", scaler(TU, iv=1.0, out_cd=2.0, in_cd=2.0), sources=burst(30.0, 4.0), end_s=10.0, seed=59))
    # ---- windows variants (the reference runs them in the same windows; ends on evaluation nanoseconds among them)
    by_name = {s["name"]: s for s in f}
    for base, windows in (("target_utilization_scales_out_and_in", [0.5, 1.0, 1.3, 2.5, 2.5, 4.0]), ("fresh_id_after_a_scale_in", [0.75, 2.0, 3.0, 3.5]),
                          ("wrr_tu", [1.0, 2.0, 3.25])):
        f.append(dict(by_name[base], name=base + "_in_windows", traced=False, windows=windows))
    for s in f:
        s.setdefault("traced", False)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """One or two Sources -> a LoadBalancer of a drawn strategy over 1 .. 3 Servers, scaled by a drawn policy -> Sink; every fourth
    spec has a fault on the scaler or on a backend, every third constant Sources."""
    rng = np.random.default_rng(211_000 + k)
    strat = STRATEGIES[int(rng.integers(0, 4))]
    n_init, c = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    mean = float(np.round(rng.uniform(0.03, 0.15), 3))
    end = float(rng.choice([3.0, 4.0, 5.0]))
    which = int(rng.integers(0, 3))
    if which == 0:
        pol = ["tu", float(rng.choice([0.3, 0.5, 0.7, 1.0]))]
    elif which == 1:
        steps = [[float(rng.choice([0.2, 0.5, 0.5, 0.8, 1.0])), int(rng.integers(1, 3))] for _ in range(int(rng.integers(1, 4)))]
        pol = ["step", steps + [[0.0, -int(rng.integers(1, 3))]]]
    else:
        lo_thr = int(rng.integers(0, 2))
        pol = ["qd", lo_thr + int(rng.integers(1, 5)), lo_thr]
    lo, hi = int(rng.integers(1, 3)), int(rng.integers(2, 6))
    sc = scaler(pol, lo=lo, hi=hi, iv=float(rng.choice([0.25, 0.5, 1.0])), out_cd=float(rng.choice([0.0, 0.0, 0.5, 1.0, 2.0])),
                in_cd=float(rng.choice([0.0, 0.5, 1.0, 2.0])), starts=2 if rng.random() < 0.1 else 1, mean=mean, c=c,
                cap=None if rng.random() < 0.7 else int(rng.integers(0, 4)), svc="const" if rng.random() < 0.2 else "exp")
    constant = k % 3 == 0
    rate = float(rng.choice([10.0, 20.0, 40.0]))
    sources = [src(LB0, rate, "constant", float(rng.choice([1.0, 1.5, 2.0])))]
    sources.append(src(LB0, float(rng.choice([2.0, 5.0, 10.0])), "constant" if constant else "poisson"))
    faults = []
    if k % 4 == 1:
        on = A0 if rng.random() < 0.5 else ["server", int(rng.integers(0, n_init))]
        at = float(np.round(rng.uniform(0.2, end), 2))
        faults.append(crash(on, at, None if rng.random() < 0.3 else float(np.round(rng.uniform(at, end), 2))) if rng.random() < 0.6 else
                      pause(on, at, float(np.round(rng.uniform(at, end), 2))))
    return pool(f"autoscaler_graph_{k}", sc, strategy=strat, n_init=n_init, mean=mean, c=c, sources=sources, faults=faults, end_s=end,
                seed=int(rng.integers(1, 10_000)))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups, name="autoscaler_groups", end_s=3.0):
    """`n_groups` disconnected Source -> scaled LoadBalancer -> Sink chains in ONE Simulation: the parts of hs_graph_run_parts (a pool
    belongs to the part of its LoadBalancer)."""
    servers, lbs, sources, scalers = [], [], [], []
    for g in range(n_groups):
        servers.append(srv(0.06 + 0.01 * (g % 3), 1 + g % 2, out=["sink", g]))
        lbs.append(lb(STRATEGIES[g % 4], [g]))
        sources.append(src(["lb", g], 25.0 + g % 7, "poisson"))
        scalers.append(scaler((TU, STEP, QD)[g % 3], hi=3 + g % 2, lb=g, iv=0.5, in_cd=0.5 * (g % 2), mean=0.06, c=1 + g % 2, out=["sink", g]))
    return _g(name, servers=servers, lbs=lbs, sources=sources, n_sinks=n_groups, scalers=scalers, end_s=end_s, seed=61)


def recorded_specs():
    """Everything make_golden_autoscaler.py records: the fixtures, the random graphs and the groups."""
    return all_specs() + [groups_spec(16)]
