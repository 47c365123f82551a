#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for Servers whose queue is a LIFOQueue, an AdaptiveLIFO or a CoDelQueue -- the
yardstick of tests/test_queues_host.py and tests/test_gpu_queues.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_queues.py          # writes tests/golden/live_queues/part_*.npz

Recorded (tests/queue_specs.py QUEUES reads them back): every spec of queue_specs.recorded_specs() through
record_family.run_case(spec, "queues").  The family and its section are registered on record_family's dicts here, at run time: what
the "mixed" family records, then `q_state` (queue_specs.queue_results: every stats field and every private state variable of every
policy object, len(policy) and server.depth) and `codel_branches` (how often each branch of `_codel_dequeue` was taken, counted by
the wrapper below -- the reference's method itself runs unchanged).  `_Reference` is subclassed so that a server dict's `qp` becomes
the reference's policy; its CoDelQueue reads the Server's clock.  The recorder first asserts that the product's host-side lowering
takes every spec with `has_queue_policies` set; after the run it asserts that every distinguishing branch is taken by a fixture.
Running it again rewrites the parts byte for byte.
"""
from __future__ import annotations

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import queue_specs as QS  # noqa: E402
from happysimulator.components.queue_policies.adaptive_lifo import AdaptiveLIFO  # noqa: E402
from happysimulator.components.queue_policies.codel import CoDelQueue  # noqa: E402
from happysimulator.components.queue_policy import LIFOQueue  # noqa: E402

import types  # noqa: E402

REF_POLICIES = types.SimpleNamespace(LIFOQueue=LIFOQueue, AdaptiveLIFO=AdaptiveLIFO, CoDelQueue=CoDelQueue)
_branches = np.zeros(len(QS.BRANCHES), np.int64)        # of the case that is running


def _counted_codel_dequeue(self, now, sojourn_time, _orig=CoDelQueue._codel_dequeue):
    """CoDelQueue._codel_dequeue, unchanged, with the branch it took read off the state before and behind it."""
    dropping, count, last, drop_next, dropped = self._dropping, self._count, self._last_count, self._drop_next, self._dropped
    _orig(self, now, sojourn_time)
    if not dropping and self._dropping:
        delta = count - last
        if delta < 1:
            _branches[0] += 1
        elif (now - drop_next).to_seconds() < self._interval:
            assert self._count == 1
            _branches[2] += 1
        else:
            assert self._count == delta
            _branches[1] += delta > 1
    if dropping and not self._dropping:
        _branches[3] += 1
    if self._dropped - dropped >= 2:
        _branches[4] += 1


CoDelQueue._codel_dequeue = _counted_codel_dequeue


class _QueueReference(RF._Reference):
    """record_family._Reference whose Servers read `qp`."""

    def server(self, i, sv):
        if sv.get("qp") is None:
            return super().server(i, sv)
        pol = QS.make_policy(REF_POLICIES, sv["qp"])
        server = RF.Server(f"srv{i}", concurrency=sv.get("c", 1), queue_policy=pol,
                           service_time=(RF.ConstantLatency(sv["mean"]) if sv.get("svc") == "const" else
                                         RF.MG.PhiloxExponentialLatency(sv["mean"], RF.hs.Stream(self.seed, i, RF.hs.STREAM_SERVICE))))
        if isinstance(pol, CoDelQueue):
            pol.set_clock(lambda: server.now)
        return server


RF._Reference = _QueueReference
RF._SECTION["queues"] = lambda c: dict(QS.queue_results(c.pools), codel_branches=_branches.copy())
RF.SECTIONS["queues"] = RF.SECTIONS["mixed"] + ("queues",)
RF.N_KINDS["queues"] = len(RF.EV)


def run_case(spec, want_trace=False):
    _branches[:] = 0
    return RF.run_case(spec, "queues", want_trace=want_trace)


def _same(a, b, but=()):
    assert set(a) == set(b)
    for k in a:
        if k in but:
            continue
        x, y = a[k], b[k]
        ok = (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y
        assert ok, k


def main():
    cases = {}
    for spec in QS.recorded_specs():
        sim, _pools = QS.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        policied = any(sv.get("qp") for sv in spec["servers"])
        assert bool(sim._graph.arrays.has_queue_policies) == policied, spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[QS.QUEUES.key("case", spec)] = run_case(spec, want_trace=spec["name"] in QS.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        assert spec.get("auto") or spec["end_s"] <= 20.0
        assert len(res["by_kind"]) == 39                   # no new Event kinds
        print(spec["name"], res["total_events"], res["q_state"][:, :12].tolist(), res["codel_branches"].tolist(), flush=True)
    get = lambda name: cases[QS.QUEUES.key("case", QS.FIXTURES[name])]  # noqa: E731
    # ---- every distinguishing branch is taken
    r = get("lifo_unbounded_overloaded")
    fifo = run_case(QS.without_policies(QS.FIXTURES["lifo_unbounded_overloaded"]))
    assert len(r["sink_latency_s"]) > 20 and r["sink_latency_s"].tobytes() != fifo["sink_latency_s"].tobytes()
    r = get("alifo_threshold_3_switches_modes")["q_state"][0]
    assert r[8] >= 3 and r[5] > 0 and r[6] > 0, r                      # mode_switches, dequeued_fifo, dequeued_lifo
    r = get("alifo_threshold_1_is_always_congested")["q_state"][0]
    assert r[5] == 0 and r[6] > 20 and r[8] == 1, r
    for name in ("alifo_threshold_above_its_capacity_is_a_fifo", "alifo_unbounded_huge_threshold_is_a_fifo", "codel_target_never_reached_is_a_fifo"):
        r = get(name)
        fifo = run_case(QS.without_policies(QS.FIXTURES[name]))
        _same(r, fifo, but=("q_state", "codel_branches"))
        assert r["total_events"] > 300 and (r["q_state"][0, 6] == 0 if r["q_state"][0, 1] == 2 else r["q_state"][0, 6] == 0), name
    r = get("alifo_threshold_above_its_capacity_is_a_fifo")
    assert r["dropped"][0] > 0 and r["q_state"][0, 7] == r["dropped"][0]
    b = get("codel_c2_enters_leaves_and_re_enters")["codel_branches"]
    assert (b[:4] > 0).all(), b                                        # the first four CoDel branches in one fixture
    b = get("codel_c2_short_interval")["codel_branches"]
    assert b[0] > 0 and b[1] > 0 and b[3] > 0, b
    r = get("codel_one_nanosecond_interval_drains_the_queue")
    assert r["codel_branches"][4] > 0 and r["q_state"][0, 6] > r["q_state"][0, 8], (r["codel_branches"], r["q_state"])
    total = sum(c["codel_branches"] for c in cases.values())
    assert (total > 0).all(), total
    r = get("codel_checked_backend")                                   # probes wait in the CoDel queues; something is dropped behind a pop
    assert r["by_kind"][RF.EV["hc_cycle"]] > 0 and r["q_state"][:, 6].sum() > 0
    for nm in ("lifo", "alifo", "codel"):
        assert get(f"{nm}_crashed_and_restarted")["dropped"][0] == 0 and get(f"{nm}_under_a_probe_on_depth")["probe_v"].max() >= 3
        assert get(f"{nm}_behind_a_client_with_fixed_retry")["cl_stats"][0, 3] > 0          # retries
        assert get(f"{nm}_behind_a_gate_flush")["flow_stats"][0, 3] == 2
    assert len(QS.FIXTURES) >= 36 and len(QS.TRACED) >= 6 and QS.N_RANDOM >= 120
    cases[QS.QUEUES.key("defaults")] = QS.policy_defaults(REF_POLICIES)
    QS.QUEUES.write(cases)


if __name__ == "__main__":
    main()
