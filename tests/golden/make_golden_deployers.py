#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for a RollingDeployer over a LoadBalancer -- the yardstick of
tests/test_deployers_host.py and tests/test_gpu_deployers.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_deployers.py          # writes tests/golden/live_deployers/part_*.npz

Recorded (tests/deployer_specs.py DEPLOYERS reads them back): every spec of deployer_specs.recorded_specs() through
record_family.run_case(spec, "deployer").  The family is registered on record_family's and graph_family's objects here, at run time:
graph_family.wire puts the spec's deployers behind the other entities, graph_family.schedule_all schedules their deploy() Events behind
the spec's schedule, record_family.classify counts the deployer's seven Events as kinds 40 .. 46 at the deployer's node and numbers an
instance the factory made like the product numbers its pool (behind all of the Simulation's own nodes).  The factory builds instance
k with SERVICE stream base len(spec["servers"]) + k - 1 and keeps every Server it made, so that a removed instance can still be read.
The reference's handlers run unchanged.  The recorder first asserts that the product's host-side lowering takes every spec and that no
run outgrew the product's pool; after the run it asserts what each named fixture is there to show.
"""
from __future__ import annotations

import sys

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import deployer_specs as DS  # noqa: E402
from happysimulator.components.deployment import RollingDeployer  # noqa: E402

EV = RF.EV
EV["as_eval"] = len(EV)
assert EV["as_eval"] == DS.EV_AS_EVAL
for _name in DS.RD_EVENTS:
    EV[_name] = len(EV)
assert EV[DS.RD_EVENTS[0]] == DS.EV_RD_FIRST and len(EV) == DS.N_KINDS
RF.REF_NS.RollingDeployer = RollingDeployer
RF._OWN_KINDS[RollingDeployer] = {name: EV[name] for name in DS.RD_EVENTS}
_cur = {}          # of the case that is running: spec, pools, the node of every part of every instance, the states behind the windows


class ReferenceFactory:
    """`server_factory` of deployer i over the reference's classes; `made`: every Server it built, in call order."""

    def __init__(self, spec, i, pools):
        self.spec, self.i, self.dp, self.pools, self.made = spec, i, spec["deployers"][i], pools, []

    def __call__(self, name):
        v = self.dp["inst"]
        k = int(name.rsplit("_", 1)[1])
        assert name == f"rd{self.i}_v2_{k}" and k == len(self.made) + 1
        out = None if v["out"] is None else self.pools[v["out"][0]][v["out"][1]]
        service = (RF.ConstantLatency(v["mean"]) if v["svc"] == "const" else
                   RF.MG.PhiloxExponentialLatency(v["mean"], RF.hs.Stream(self.spec["seed"], len(self.spec["servers"]) + k - 1, RF.hs.STREAM_SERVICE)))
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
        entities = DS.with_deployers(spec, pools, entities, ns, ReferenceFactory)
        DS.tolerate_removed(pools["lb"])                   # (the other families' sections read every listed backend's BackendInfo)
        _cur.update(spec=spec, pools=pools, part_node={}, window_states=[])
    return pools, sources, probes, entities


def schedule_all(spec, pools, sim, event_cls, at, early_events):
    _schedule_all(spec, pools, sim, event_cls, at, early_events)
    if "factory" in pools and pools["factory"] and isinstance(pools["factory"][0], ReferenceFactory):
        DS.schedule_deployers(spec, pools, sim, at)


def classify(e, node_of, by_name):
    node = _cur["part_node"].get(id(e.target))
    if node is not None:
        node_of[id(e.target)] = node
    return _classify(e, node_of, by_name)


def run_sim_windows(sim, spec):
    """make_golden.run_sim_windows, with the deployers' object state read behind every window of a windowed spec."""
    if not spec.get("windows"):
        return _run_sim_windows(sim, spec)
    for t in list(spec["windows"]) + [spec["end_s"]]:
        sim._run_window(RF.MG._at(spec, t))
        _cur["window_states"].append(DS.deployer_state(_cur["pools"]))
    sim._is_running = False
    return sim._build_summary()


def _section(c):
    out = DS.deployer_results(c.spec, c.pools)
    if c.spec.get("windows"):
        out.update(DS.window_states(_cur["window_states"]))
    return out


GF.wire, GF.schedule_all, RF.classify, RF.MG.run_sim_windows = wire, schedule_all, classify, run_sim_windows
RF._SECTION["deployer"] = _section
RF.SECTIONS["deployer"] = RF.SECTIONS["mixed"] + ("deployer",)
RF.N_KINDS["deployer"] = len(EV)


def run_case(spec, want_trace=False):
    return RF.run_case(spec, "deployer", want_trace=want_trace)


def main():
    cases = {}
    for spec in DS.recorded_specs():
        sim, _pools = DS.build(spec)
        g = sim.lowered()                                  # the product takes this graph (host-side lowering; raises otherwise)
        sim._general_prepare(g, False)                     # ... every scheduled Event of it
        assert g.arrays.has_deployers
        index = {g.node_of[id(d)]: i for i, d in enumerate(_pools["deployer"])}
        _cur.clear()
        _cur["pool_node"] = {(index[dn], k): node for node, (dn, k) in g.dpool_of.items()}
        res = cases[DS.DEPLOYERS.key("case", spec)] = run_case(spec, want_trace=spec["name"] in DS.TRACED)
        sizes = [sum(1 for (i, _k) in _cur["pool_node"] if i == j) for j in range(len(spec["deployers"]))]
        assert (res["rd_state"][:, 12] <= np.array(sizes)).all(), (spec["name"], "the reference created an instance beyond the product's pool", sizes)
        res["python"] = list(sys.version_info[:3])
        assert res["total_events"] <= 20_000, (spec["name"], res["total_events"])
        assert len(res["by_kind"]) == DS.N_KINDS and res["by_kind"][DS.EV_AS_EVAL] == 0
        print(spec["name"], res["total_events"], res["by_kind"][DS.EV_RD_FIRST:].tolist(), res["rd_state"].tolist(), res["rd_members"], flush=True)
    DS.DEPLOYERS.write(cases)
    get = lambda name: cases[DS.DEPLOYERS.key("case", DS.FIXTURES[name])]  # noqa: E731
    st = lambda name: dict(zip(("started", "completed", "rolled_back", "replaced", "performed", "passed", "failed", "status", "total",  # noqa: E731
                                "state_replaced", "state_failed", "batch", "next_id", "fail_count"), get(name)["rd_state"][0].tolist()))
    done, back = DS.STATUS["completed"], DS.STATUS["rolled_back"]
    # ---- what each fixture is there to show
    for name, batches in (("batch_1_threshold_1_completes", 3), ("batch_equal_to_the_backend_count", 1), ("batch_above_the_backend_count", 1)):
        s = st(name)
        assert s["status"] == done and s["failed"] == 0 and s["replaced"] == 3 and s["batch"] == batches and s["rolled_back"] == 0, (name, s)
        assert s["completed"] == 1 and get(name)["rd_members"][0] == [f"rd0_v2_{k}" for k in (1, 2, 3)]
    # two instances per batch: the first pass schedules one more health check, so the checks multiply -- the batch completes twice
    s = st("batch_2_threshold_1")
    assert s["completed"] == 2 and s["state_replaced"] == 4 > s["total"] and s["failed"] == 0 and s["status"] == done, s
    s = st("batch_1_threshold_2_one_failure_per_instance")
    assert s["status"] == done and s["failed"] == 3 and s["replaced"] == 3 and s["next_id"] == 3, s   # one failure per new instance, in its first round
    s = st("default_settings_batch_2_rolls_back")
    assert s["rolled_back"] == 1 and s["state_failed"] == 2 and s["fail_count"] == 2, s
    s = st("default_settings_batch_1_rolls_back_at_the_second_batch")
    assert s["rolled_back"] == 1 and s["status"] == back and s["completed"] == 0 and s["batch"] == 3, s
    r, s = get("rollback_with_a_pass_in_flight_walks_on_to_completed"), st("rollback_with_a_pass_in_flight_walks_on_to_completed")
    assert s["rolled_back"] >= 1 and s["completed"] >= 1 and s["status"] == done, s
    tr = r["trace"]
    first_back = np.nonzero(tr[:, 1] == EV["_rolling_rollback"])[0][0]
    assert (tr[first_back:, 1] == EV["_rolling_health_pass"]).any() and (tr[first_back:, 1] == EV["_rolling_complete"]).any()
    assert r["rd_members"][0] == [] and r["lb_stats"][0, 3] > 0                     # the rollback took the new ones, the passes the old ones
    r = get("rollback_leaves_the_load_balancer_empty_under_traffic")
    assert r["rd_members"][0] == [] and r["lb_stats"][0, 3] > 100 and r["lb_stats"][0, 2] == r["lb_stats"][0, 3], r["lb_stats"].tolist()
    s = st("second_deploy_fails_the_pending_timeouts_of_the_first")
    assert s["started"] == 2 and s["rolled_back"] == 1 and s["status"] == back and s["state_failed"] == 1, s
    s = st("second_deploy_inside_the_first")
    assert s["started"] == 2 and s["next_id"] == 6 and s["total"] == 4, s                 # the second start saw a new instance among the members
    assert st("second_deploy_behind_the_first")["next_id"] == 6 and st("three_deploys")["started"] == 3
    r = get("full_queue_refuses_a_probe")
    assert r["probe_drops"] > 0 and st("full_queue_refuses_a_probe")["passed"] == st("full_queue_refuses_a_probe")["performed"], r["probe_drops"]
    s = st("crashed_deployer")
    assert s["status"] == DS.STATUS["in_progress"] and s["passed"] == 1 and get("crashed_deployer")["by_kind"][DS.EV_RD_FIRST + 2] > s["performed"], s
    assert st("paused_deployer")["status"] == DS.STATUS["in_progress"] and st("paused_deployer")["performed"] == 0
    r = get("end_time_infinity_ends_with_the_deployment")
    assert st("end_time_infinity_ends_with_the_deployment")["status"] == done and r["pending_events"] == 0
    assert st("no_backends_at_all")["status"] == done and st("no_backends_at_all")["next_id"] == 0
    r = get("removed_initial_backend_finishes_its_queue")
    assert (r["lb_backend_total_requests"] == -1).all() and r["completed"][:3].sum() == r["accepted"][:3].sum() > 0
    tr = r["trace"]
    gone = tr[tr[:, 1] == EV["_rolling_replace_batch"]][-1, 0]
    assert ((tr[:, 1] == EV["continuation"]) & (tr[:, 0] > gone) & (tr[:, 2] < 3 + tr[:, 2].min())).any(), "no completion of an old backend behind its removal"
    s = st("slow_interval_health_checks_multiply")
    assert s["performed"] == 12 > 3 * 3 and s["completed"] == 4, s
    for strat in DS.STRATEGIES:
        assert st(f"{strat}_completes")["completed"] >= 1 and st(f"{strat}_rolls_back")["rolled_back"] == 1, strat
        assert st(f"{strat}_two_deploys")["started"] == 2
    assert st("sixty_six_members_one_batch")["replaced"] == 66
    for name in DS.FIXTURES:
        if name.endswith("_in_windows"):
            a, b = get(name[:-len("_in_windows")]), get(name)
            for k in a:
                if k not in ("trace", "python") and isinstance(a[k], np.ndarray):
                    assert a[k].tobytes() == b[k].tobytes(), (name, k)
            assert len({tuple(m[0]) for m in b["window_rd_members"]}) > 1             # the members changed between two windows
    assert len(DS.FIXTURES) >= 30 and 3 * len(DS.TRACED) >= len(DS.FIXTURES) and DS.N_RANDOM >= 100


if __name__ == "__main__":
    main()
