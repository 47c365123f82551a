#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for a CanaryDeployer over a LoadBalancer -- the yardstick of
tests/test_canary_host.py and tests/test_gpu_canary.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_canary.py          # writes tests/golden/live_canary/part_*.npz

Recorded (tests/canary_specs.py CANARY reads them back): every spec of canary_specs.recorded_specs() through
record_family.run_case(spec, "canary"), and the two evaluators' `is_healthy` over enumerated inputs.  The family is registered on
record_family's and graph_family's objects here, at run time, as tests/golden/make_golden_deployers.py registers the rolling deployer's:
the canary deployer's six Events are kinds 47 .. 52 at the deployer's node, the canary Server is numbered like the product numbers its
pool of one.  The reference's handlers run unchanged.  The interpreter's `sum` over the baseline's figures is part of what is recorded:
the recorder asserts CPython < 3.12 (a plain left-to-right sum, which the device restates) and records the version.  The recorder first
asserts that the product's host-side lowering takes every spec; after the run it asserts what each named fixture is there to show.
"""
from __future__ import annotations

import sys

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import deployer_specs as DS  # noqa: E402
import canary_specs as CS  # noqa: E402
from happysimulator.components.deployment.canary_deployer import (CanaryDeployer, CanaryStage, ErrorRateEvaluator,  # noqa: E402
                                                                  LatencyEvaluator)

EV = RF.EV
EV["as_eval"] = len(EV)
for _name in DS.RD_EVENTS + CS.CN_EVENTS:
    EV[_name] = len(EV)
assert EV[CS.CN_EVENTS[0]] == CS.EV_CN_FIRST and len(EV) == CS.N_KINDS
RF.REF_NS.CanaryDeployer, RF.REF_NS.CanaryStage, RF.REF_NS.ErrorRateEvaluator, RF.REF_NS.LatencyEvaluator = (
    CanaryDeployer, CanaryStage, ErrorRateEvaluator, LatencyEvaluator)
RF._OWN_KINDS[CanaryDeployer] = {name: EV[name] for name in CS.CN_EVENTS}
_cur = {}


class ReferenceFactory:
    """`server_factory` of canary deployer i over the reference's classes; `made`: every Server it built."""

    def __init__(self, spec, i, pools):
        self.spec, self.i, self.cn, self.pools, self.made = spec, i, spec["canaries"][i], pools, []

    def __call__(self, name):
        v = self.cn["inst"]
        assert name == f"cn{self.i}_canary" and not self.made
        out = None if v["out"] is None else self.pools[v["out"][0]][v["out"][1]]
        service = (RF.ConstantLatency(v["mean"]) if v["svc"] == "const" else
                   RF.MG.PhiloxExponentialLatency(v["mean"], RF.hs.Stream(self.spec["seed"], len(self.spec["servers"]), RF.hs.STREAM_SERVICE)))
        server = RF.Server(name, concurrency=v["c"], queue_capacity=v["cap"], service_time=service, downstream=out)
        self.made.append(server)
        node = _cur["pool_node"].get((self.i, 1), -1)          # the node the product lowers the canary to
        for part in (server, server._queue, server._driver, server._worker):
            _cur["part_node"][id(part)] = node
        return server


_wire, _schedule_all, _classify, _run_sim_windows = GF.wire, GF.schedule_all, RF.classify, RF.MG.run_sim_windows


def wire(spec, F, ns):
    pools, sources, probes, entities = _wire(spec, F, ns)
    if ns is RF.REF_NS:
        entities = CS.with_canaries(spec, pools, entities, ns, ReferenceFactory)
        DS.tolerate_removed(pools["lb"])
        _cur.update(spec=spec, pools=pools, part_node={}, window_states=[])
    return pools, sources, probes, entities


def schedule_all(spec, pools, sim, event_cls, at, early_events):
    _schedule_all(spec, pools, sim, event_cls, at, early_events)
    if "factory" in pools and pools["factory"] and isinstance(pools["factory"][0], ReferenceFactory):
        CS.schedule_canaries(spec, pools, sim, at)


def classify(e, node_of, by_name):
    node = _cur["part_node"].get(id(e.target))
    if node is not None:
        node_of[id(e.target)] = node
    return _classify(e, node_of, by_name)


def run_sim_windows(sim, spec):
    if not spec.get("windows"):
        return _run_sim_windows(sim, spec)
    for t in list(spec["windows"]) + [spec["end_s"]]:
        sim._run_window(RF.MG._at(spec, t))
        _cur["window_states"].append(CS.canary_state(_cur["pools"]))
    sim._is_running = False
    return sim._build_summary()


def _section(c):
    out = CS.canary_results(c.spec, c.pools)
    if c.spec.get("windows"):
        out.update(CS.window_states(_cur["window_states"]))
    return out


GF.wire, GF.schedule_all, RF.classify, RF.MG.run_sim_windows = wire, schedule_all, classify, run_sim_windows
RF._SECTION["canary"] = _section
RF.SECTIONS["canary"] = RF.SECTIONS["mixed"] + ("canary",)
RF.N_KINDS["canary"] = len(EV)


class _Stats:
    def __init__(self, completed, rejected):
        self.requests_completed, self.requests_rejected = completed, rejected


class _Backend:
    def __init__(self, completed, rejected, latency):
        self.stats, self.average_service_time = _Stats(completed, rejected), latency


def evaluator_inputs():
    """Enumerated inputs of the two evaluators' `is_healthy`: (evaluator spec, canary, [baseline, ...]) with a backend as (completed,
    rejected, average_service_time)."""
    rows = []
    backends = [(0, 0, 0.0), (10, 0, 0.1), (9, 1, 0.15), (90, 10, 0.15000000000000002), (1, 1, 0.30000000000000004), (3, 0, 0.1 + 0.2), (7, 3, 1.0)]
    baselines = ([], [(10, 0, 0.1)], [(9, 1, 0.1)] * 3, [(10, 0, 0.1), (5, 5, 0.2), (99, 1, 0.3)], [(0, 0, 0.0)] * 2, [(9, 1, 0.1), (8, 2, 0.1), (7, 3, 0.1)])
    for ev in (["error", 0.05, 2.0], ["error", 0.5, 1.0], ["error", 0.0, 2.0], ["latency", 1.0, 1.5], ["latency", 0.15, 1.0], ["latency", 0.2, 3.0]):
        for cn in backends:
            for base in baselines:
                rows.append((ev, cn, base))
    return rows


def record_evaluators(ns):
    return np.array([CS.make_evaluator(ns, ev).is_healthy(_Backend(*cn), [_Backend(*b) for b in base]) for ev, cn, base in evaluator_inputs()], np.int64)


def main():
    assert sys.version_info < (3, 12), "from CPython 3.12 on `sum` over floats is compensated: the device's plain sum would have to follow"
    import happy_simulator_amd as product

    cases = {}
    for spec in CS.recorded_specs():
        sim, _pools = CS.build(spec)
        g = sim.lowered()                                  # the product takes this graph (host-side lowering; raises otherwise)
        sim._general_prepare(g, bool(spec.get("auto")))
        assert g.arrays.has_canaries
        index = {g.node_of[id(d)]: i for i, d in enumerate(_pools["canary"])}
        _cur.clear()
        _cur["pool_node"] = {(index[dn], k): node for node, (dn, k) in g.dpool_of.items()}
        res = cases[CS.CANARY.key("case", spec)] = RF.run_case(spec, "canary", want_trace=spec["name"] in CS.TRACED)
        res["python"] = list(sys.version_info[:3])
        assert res["total_events"] <= 20_000, (spec["name"], res["total_events"])
        assert len(res["by_kind"]) == CS.N_KINDS and not res["by_kind"][DS.EV_AS_EVAL:CS.EV_CN_FIRST].any()
        print(spec["name"], res["total_events"], res["by_kind"][CS.EV_CN_FIRST:].tolist(), res["cn_state"].tolist(), res["cn_members"],
              res["cn_weights"], flush=True)
    cases[CS.CANARY.key("evaluators")] = dict(healthy=record_evaluators(RF.REF_NS))
    CS.CANARY.write(cases)
    assert record_evaluators(product).tolist() == cases[CS.CANARY.key("evaluators")]["healthy"].tolist()
    get = lambda name: cases[CS.CANARY.key("case", CS.FIXTURES[name])]  # noqa: E731
    st = lambda name: dict(zip(("started", "completed", "rolled_back", "stages", "performed", "passed", "failed", "status", "stage", "total",  # noqa: E731
                                "has_canary", "stage_start"), get(name)["cn_state"][0].tolist()))
    done, back = CS.STATUS["completed"], CS.STATUS["rolled_back"]
    # ---- what each fixture is there to show
    for name in ("default_stages_to_promotion_wrr", "default_stages_to_promotion_wlc", "quick_stages_to_promotion_wrr", "quick_stages_to_promotion_wlc"):
        s, r = st(name), get(name)
        assert s["status"] == done and s["stages"] == 4 and s["completed"] == 1 and r["cn_members"][0] == ["cn0_canary"], (name, s)
        assert all(w == 1 for _k, w in r["cn_weights"][0]) and len(r["cn_weights"][0]) == 4
    r = get("quick_stages_to_promotion_wrr_in_windows")
    seen = {tuple(map(tuple, w[0])) for w in r["window_cn_weights"]}
    assert len(seen) >= 4 and any(dict(w)["cn0_canary"] == 25 and dict(w)["srv0"] == 25 for w in seen) and any(dict(w)["srv0"] == 33 for w in seen), seen
    for name in ("round_robin_weights_are_a_no_op", "least_conn_weights_are_a_no_op"):
        assert st(name)["status"] == done and get(name)["cn_weights"][0] == [], name
    s = st("latency_evaluator_rolls_a_slow_canary_back")
    assert s["status"] == back and s["failed"] == 1 and s["rolled_back"] == 1 and get("latency_evaluator_rolls_a_slow_canary_back")["cn_members"][0] == [
        "srv0", "srv1", "srv2"], s
    s = st("latency_evaluator_passes_a_like_canary")
    assert s["failed"] == 0 and s["status"] == done and s["performed"] == 8, s
    s = st("latency_above_max_latency")
    assert s["status"] == back and s["failed"] == 1 and s["passed"] == 2, s             # its own limit, once the canary has served at all
    s, r = st("latency_within_an_ulp_of_the_threshold"), get("latency_within_an_ulp_of_the_threshold")
    assert s["performed"] == 8 and s["failed"] == 0 and s["status"] == done, s
    # the canary's average (n x 0.15 / n) and the threshold (average of the baseline's m x 0.1 / m, times 1.5) differ by rounding
    # alone: a few ulps of 0.15 (here by the counts at the end of the run), so every evaluation was decided by the order of the roundings
    n_c, ms = int(r["cn_instance_stats"][0, 0]), r["accepted"][:3].tolist()
    avg = lambda v, k: sum([v] * k) / k  # noqa: E731
    x, thr = avg(0.15, n_c), sum(avg(0.1, m) for m in ms) / 3 * 1.5
    assert n_c > 3 and abs(x - thr) <= 16 * np.spacing(0.15), (x, thr)
    s = st("error_rate_evaluator_strict")
    assert s["performed"] > 0 and get("error_rate_evaluator_strict")["rejected"].sum() >= 0
    s = st("period_shorter_than_the_interval")
    assert s["stages"] == 2 and s["performed"] == 2 and s["status"] == done, s          # one evaluation ends a stage
    s = st("period_no_multiple_of_the_interval")
    assert s["stages"] == 3 and s["performed"] == 2 + 3 + 1 and s["status"] == done, s  # 0.7 s: two evaluations; 1.1 s: three; 0 s: one
    assert st("never_deployed")["started"] == 0 and st("never_deployed")["has_canary"] == 0
    assert st("no_baseline_at_all")["status"] == done and get("no_baseline_at_all")["cn_members"][0] == ["cn0_canary"]
    assert st("crashed_canary_deployer")["status"] == CS.STATUS["in_progress"]
    r = get("end_time_infinity_ends_with_the_promotion")
    assert st("end_time_infinity_ends_with_the_promotion")["status"] == done and r["pending_events"] == 0
    r = get("removed_baseline_finishes_its_queue")
    assert (r["lb_backend_total_requests"] == -1).all() and r["completed"][:3].sum() == r["accepted"][:3].sum() > 0
    assert st("sixty_six_baselines_promoted")["status"] == done and get("sixty_six_baselines_promoted")["cn_members"][0] == ["cn0_canary"]
    for name in CS.FIXTURES:
        if name.endswith("_in_windows"):
            a, b = get(name[:-len("_in_windows")]), get(name)
            for k in a:
                if k not in ("trace", "python") and isinstance(a[k], np.ndarray):
                    assert a[k].tobytes() == b[k].tobytes(), (name, k)
    assert 3 * len(CS.TRACED) >= len(CS.FIXTURES) and CS.N_RANDOM >= 100


if __name__ == "__main__":
    main()
