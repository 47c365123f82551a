#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for an AutoScaler over a LoadBalancer -- the yardstick of
tests/test_autoscaler_host.py and tests/test_gpu_autoscaler.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_autoscaler.py          # writes tests/golden/live_autoscaler/part_*.npz

Recorded (tests/autoscaler_specs.py AUTOSCALER reads them back): every spec of autoscaler_specs.recorded_specs() through
record_family.run_case(spec, "autoscaler"), and the three policies' `evaluate` over enumerated inputs.  The family is registered on
record_family's and graph_family's objects here, at run time: graph_family.wire puts the spec's scalers (and the probes on them) behind
the other entities, graph_family.schedule_all starts them behind the spec's schedule, record_family.classify counts an
`_autoscaler_evaluate` Event as kind 39 at the scaler's node and numbers an instance the factory made like the product numbers its
pool (behind all of the Simulation's own nodes).  The factory builds instance k with SERVICE stream base len(spec["servers"]) + k - 1
and keeps every Server it made, so that a removed instance can still be read.  The reference's handlers run unchanged.  The recorder
first asserts that the product's host-side lowering takes every spec; after the run it asserts what each named fixture is there to
show.  The interpreter's `sum` over the utilizations is part of what is recorded: the recorder asserts CPython < 3.12 (a plain
left-to-right sum, which the device restates) and records the version.
"""
from __future__ import annotations

import sys

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import autoscaler_specs as AS  # noqa: E402
from happysimulator.components.deployment import AutoScaler, QueueDepthScaling, StepScaling, TargetUtilization  # noqa: E402
from happysimulator.components.queue_policy import LIFOQueue  # noqa: E402

EV = RF.EV
EV["as_eval"] = len(EV)
assert EV["as_eval"] == AS.EV_AS_EVAL
RF.REF_NS.AutoScaler, RF.REF_NS.TargetUtilization, RF.REF_NS.StepScaling, RF.REF_NS.QueueDepthScaling = (
    AutoScaler, TargetUtilization, StepScaling, QueueDepthScaling)
RF._OWN_KINDS[AutoScaler] = {"_autoscaler_evaluate": EV["as_eval"]}
RF.REF_METRIC["current_count"] = "current_count"
_cur = {}          # of the case that is running: spec, pools, the node of every part of every instance, the states behind the windows


class ReferenceFactory:
    """`server_factory` of scaler i over the reference's classes; `made`: every Server it built, in call order."""

    def __init__(self, spec, i, pools):
        self.spec, self.i, self.sc, self.pools, self.made = spec, i, spec["scalers"][i], pools, []

    def __call__(self, name):
        v = self.sc["inst"]
        k = int(name.rsplit("_", 1)[1])
        assert name == f"as{self.i}_server_{k}" and k == len(self.made) + 1
        out = None if v["out"] is None else self.pools[v["out"][0]][v["out"][1]]
        service = (RF.ConstantLatency(v["mean"]) if v["svc"] == "const" else
                   RF.MG.PhiloxExponentialLatency(v["mean"], RF.hs.Stream(self.spec["seed"], len(self.spec["servers"]) + k - 1, RF.hs.STREAM_SERVICE)))
        if v.get("qp"):
            server = RF.Server(name, concurrency=v["c"], queue_policy=LIFOQueue() if v["qp"][1] is None else LIFOQueue(capacity=v["qp"][1]),
                               service_time=service, downstream=out)
        else:
            server = RF.Server(name, concurrency=v["c"], queue_capacity=v["cap"], service_time=service, downstream=out)
        self.made.append(server)
        node = _cur["pool_node"].get((self.i, k), -1)          # the node the product lowers instance k to
        for part in (server, server._queue, server._driver, server._worker):
            _cur["part_node"][id(part)] = node
        return server


_wire, _schedule_all, _classify, _run_sim_windows = GF.wire, GF.schedule_all, RF.classify, RF.MG.run_sim_windows


def wire(spec, F, ns):
    pools, sources, probes, entities = _wire(spec, F, ns)
    if ns is RF.REF_NS:
        probes, entities = AS.with_scalers(spec, pools, probes, entities, ns, ReferenceFactory,
                                           lambda target, metric, interval: F.probe(target, metric, interval))
        _cur.update(spec=spec, pools=pools, part_node={}, window_states=[])
    return pools, sources, probes, entities


def schedule_all(spec, pools, sim, event_cls, at, early_events):
    _schedule_all(spec, pools, sim, event_cls, at, early_events)
    if "factory" in pools and pools["factory"] and isinstance(pools["factory"][0], ReferenceFactory):
        AS.schedule_scalers(spec, pools, sim)


def classify(e, node_of, by_name):
    node = _cur["part_node"].get(id(e.target))
    if node is not None:
        node_of[id(e.target)] = node
    return _classify(e, node_of, by_name)


def run_sim_windows(sim, spec):
    """make_golden.run_sim_windows, with the scalers' object state read behind every window of a windowed spec."""
    if not spec.get("windows"):
        return _run_sim_windows(sim, spec)
    for t in list(spec["windows"]) + [spec["end_s"]]:
        sim._run_window(RF.MG._at(spec, t))
        _cur["window_states"].append(AS.scaler_state(_cur["pools"]))
    sim._is_running = False
    return sim._build_summary()


def _section(c):
    out = AS.scaler_results(c.spec, c.pools)
    if c.spec.get("windows"):
        out.update(AS.window_states(_cur["window_states"]))
    return out


GF.wire, GF.schedule_all, RF.classify, RF.MG.run_sim_windows = wire, schedule_all, classify, run_sim_windows
RF._SECTION["autoscaler"] = _section
RF.SECTIONS["autoscaler"] = RF.SECTIONS["mixed"] + ("autoscaler",)
RF.N_KINDS["autoscaler"] = len(EV)


def run_case(spec, want_trace=False):
    return RF.run_case(spec, "autoscaler", want_trace=want_trace)


class _Backend:
    def __init__(self, active, limit, depth):
        self.utilization, self.depth = active / limit, depth


def policy_inputs():
    """Enumerated inputs of the three policies' `evaluate`: (policy spec, [(active, limit, depth), ...], current, min, max)."""
    rows = []
    loads = ([], [(0, 1, 0)], [(1, 1, 3)], [(1, 2, 0), (2, 2, 5)], [(1, 3, 0), (2, 3, 1), (3, 3, 9)], [(1, 3, 0)] * 7, [(2, 3, 2)] * 10 + [(1, 7, 0)] * 3)
    for pol in (["tu", 0.7], ["tu", 0.3], ["tu", 1.0], ["step", [[0.5, 1], [0.9, 2], [0.0, -1]]], ["step", [[0.8, 3]]], ["step", []], ["qd", 3, 0],
                ["qd", 100, 10], ["qd", 1, 1]):
        for load in loads:
            for lo, hi in ((1, 10), (2, 3), (3, 2), (1, 1)):
                rows.append((pol, load, len(load), lo, hi))
    return rows


def record_policies(ns):
    return np.array([AS.make_policy(ns, pol).evaluate([_Backend(*b) for b in load], cur, lo, hi) for pol, load, cur, lo, hi in policy_inputs()], np.int64)


def main():
    assert sys.version_info < (3, 12), "from CPython 3.12 on `sum` over floats is compensated: the device's plain sum would have to follow"
    cases = {}
    import happy_simulator_amd as product

    for spec in AS.recorded_specs():
        sim, _pools = AS.build(spec)
        g = sim.lowered()                                  # the product takes this graph (host-side lowering; raises otherwise)
        sim._general_prepare(g, False)                     # ... every scheduled Event of it
        assert spec["end_s"] <= 10.0 and g.arrays.has_scalers
        scaler_index = {node: i for i, node in enumerate(sorted({sn for sn, _k in g.pool_of.values()} | {g.node_of[id(s)] for s in _pools["scaler"]}))}
        assert [g.node_of[id(s)] for s in _pools["scaler"]] == sorted(scaler_index)
        _cur.clear()
        _cur["pool_node"] = {(scaler_index[sn], k): node for node, (sn, k) in g.pool_of.items()}
        res = cases[AS.AUTOSCALER.key("case", spec)] = run_case(spec, want_trace=spec["name"] in AS.TRACED)
        sizes = [sum(1 for (i, _k) in _cur["pool_node"] if i == j) for j in range(len(spec["scalers"]))]
        assert (res["as_state"][:, 6] <= np.array(sizes)).all(), (spec["name"], "the reference created an instance beyond the product's pool", sizes)
        res["python"] = list(sys.version_info[:3])
        assert res["total_events"] <= 20_000, (spec["name"], res["total_events"])
        assert len(res["by_kind"]) == 40
        print(spec["name"], res["total_events"], int(res["by_kind"][39]), res["as_state"].tolist(), flush=True)
    get = lambda name: cases[AS.AUTOSCALER.key("case", AS.FIXTURES[name])]  # noqa: E731
    st = lambda name: dict(zip(("evaluations", "outs", "ins", "added", "removed", "blocks", "next_id", "last_action", "last_ns", "running", "count",  # noqa: E731
                                "managed", "history"), get(name)["as_state"][0].tolist()))
    # ---- what each fixture is there to show
    for name in ("target_utilization_scales_out_and_in", "step_scaling_scales_out_and_in", "queue_depth_scales_out_and_in"):
        s = st(name)
        assert s["outs"] > 0 and s["ins"] > 0 and s["added"] > 0 and s["removed"] > 0, (name, s)
    s = st("cooldowns_block_scale_out_and_scale_in")
    h = get("cooldowns_block_scale_out_and_scale_in")["as_history"]
    assert s["blocks"] > 0 and s["outs"] > 0 and s["ins"] > 0, s
    spec = AS.FIXTURES["cooldowns_block_scale_out_and_scale_in"]
    blocked_out = run_case(dict(spec, name="blocks_before_the_first_scale_in", end_s=float(h[h[:, 1] == 2][0, 0]) / 1e9 - 0.01))["as_state"][0]
    assert blocked_out[5] > 0 and blocked_out[2] == 0                      # a scale-out blocked by cooldown
    assert s["blocks"] > blocked_out[5]                                    # ... and later blocks, behind the first scale-in
    r = get("min_above_max_clamps_then_adds_nothing")
    s = st("min_above_max_clamps_then_adds_nothing")
    assert r["as_history"].tolist()[0][1:] == [1, 1, 2] and r["as_reasons"][0] == "Added 1 instances"   # the policy wanted 3: clamped at max
    assert s["outs"] == 1 and s["evaluations"] > 3 and s["blocks"] == 0 and s["count"] == 2              # every later evaluation: to_add <= 0
    s = st("initial_count_below_min_instances")
    assert get("initial_count_below_min_instances")["as_history"][0].tolist()[1:] == [1, 1, 3] and s["count"] >= 3
    r, s = get("scale_in_with_nothing_managed"), st("scale_in_with_nothing_managed")
    assert s["ins"] > 0 and s["removed"] > 0 and s["managed"] == 0 and s["next_id"] == 0 and s["count"] == 3
    assert all(row[1] == 2 and row[2] == row[3] == 3 for row in r["as_history"].tolist()) and s["blocks"] > 0   # (the cooldown starts all the same)
    r, s = get("removed_instance_completes_work_afterwards"), st("removed_instance_completes_work_afterwards")
    assert s["removed"] > 0 and (r["as_instance_total_requests"] == -1).any()
    sim, pools_ = AS.build(AS.FIXTURES["removed_instance_completes_work_afterwards"])
    g = sim.lowered()
    tr = r["trace"]
    late = [k for k, t in AS.removal_times(r["as_history"]).items()
            if ((tr[:, 2] == next(n for n, (_sn, kk) in g.pool_of.items() if kk == k)) & (tr[:, 1] == EV["continuation"]) & (tr[:, 0] > t)).any()]
    assert late, "no completion behind a removal"
    r, s = get("fresh_id_after_a_scale_in"), st("fresh_id_after_a_scale_in")
    acts = r["as_history"][:, 1].tolist()
    assert 2 in acts and 1 in acts[acts.index(2):] and s["next_id"] > s["managed"] and s["next_id"] == s["added"], (acts, s)
    left = AS.removal_times(r["as_history"])
    assert left and max(left) < s["next_id"] or max(left) == s["next_id"] and min(left) < max(left)     # an id handed out behind a removal
    s = st("stopped_before_the_run")
    assert s["evaluations"] == 0 and s["running"] == 0 and get("stopped_before_the_run")["by_kind"][39] == 1
    one, two = get("target_utilization_scales_out_and_in"), get("started_twice")
    assert st("started_twice")["evaluations"] >= 2 * 9 and two["by_kind"][39] == st("started_twice")["evaluations"]
    assert one["by_kind"][39] == st("target_utilization_scales_out_and_in")["evaluations"]
    s = st("crashed_scaler_never_ticks_again")
    assert s["evaluations"] == 3 and get("crashed_scaler_never_ticks_again")["by_kind"][39] == 4, s     # 0, 0.5, 1.0 s; the Event of 1.5 s is dropped
    assert st("paused_scaler")["evaluations"] == 2
    for strat in AS.STRATEGIES:
        assert sum(st(f"{strat}_{pn}")["outs"] > 0 for pn in ("tu", "step", "qd")) >= 2, strat
        assert all(st(f"{strat}_{pn}")["ins"] > 0 for pn in ("tu", "step", "qd")), strat
    assert st("sixty_six_members")["count"] >= 64 and st("sixty_six_members")["outs"] > 0
    assert len(get("probe_on_current_count")["probe_v"]) > 10 and len(set(get("probe_on_current_count")["probe_v"].tolist())) > 2
    assert get("policied_instances")["as_instance_stats"][:, 2].sum() > 0 and get("bounded_queue_instances")["as_instance_stats"][:, 0].sum() > 0
    for name in AS.FIXTURES:
        if name.endswith("_in_windows"):
            a, b = get(name[:-len("_in_windows")]), get(name)
            for k in a:
                if k not in ("trace", "python") and isinstance(a[k], np.ndarray):
                    assert a[k].tobytes() == b[k].tobytes(), (name, k)
            assert len(set(b["window_as_state"][:, 0, 10].tolist())) > 1           # current_count changed between two windows
    assert len(AS.FIXTURES) >= 30 and len(AS.TRACED) >= 8 and AS.N_RANDOM >= 100
    # ---- the policies on their own, over enumerated inputs (tests/test_autoscaler_host.py evaluates the product's on the same)
    cases[AS.AUTOSCALER.key("policies")] = dict(desired=record_policies(RF.REF_NS))
    assert record_policies(product).tolist() == cases[AS.AUTOSCALER.key("policies")]["desired"].tolist()
    AS.AUTOSCALER.write(cases)


if __name__ == "__main__":
    main()
