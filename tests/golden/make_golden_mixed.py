#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for graphs that mix the entity families of the single-heap loop -- limiters,
HealthCheckers, Bulkhead / TimeoutWrapper, Clients, BatchProcessor / ConveyorBelt / GateController, faults over all of them -- the
yardstick of tests/test_mixed_host.py and tests/test_gpu_mixed.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_mixed.py          # writes tests/golden/live_mixed/part_*.npz

Recorded (tests/mixed_specs.py MIXED reads them back): every spec of mixed_specs.recorded_specs() through
record_family.run_case(spec, "mixed"): what the Client family records plus the flow entities' section, all 39 kinds in by_kind and in
the traces of mixed_specs.TRACED.  The recorder first asserts that the product's host-side lowering takes the spec and every
scheduled Event of it (no device needed), and that `has_flows` is set where a flow entity is present: no case is left out.  Running it
again rewrites the parts byte for byte.

events_cancelled: the reference counts every popped Event whose `cancelled` flag is set, whoever set it.  In these recordings that
is a BatchProcessor's `_BatchTimeout` (cancelled by the batch that starts), a send_request() Event cancelled by its caller and the
Events of a fault whose handle was cancelled (`cancelled_events_of_three_origins` holds all three); no wrapper, Client, checker or
limiter cancels an Event of its own.

time_travel: an Event that lies before the Simulation's start is popped and skipped and counts nowhere.  A gate's start_events()
and a FaultSchedule's Events hold absolute times and `checker.start()` called before the Simulation exists holds time 0: under a
later start_time they lie in the past (`gate_events_and_an_early_checker_before_a_later_start_time`, every eighth random graph).
"""
from __future__ import annotations

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import mixed_specs as MX  # noqa: E402

EV = RF.EV


def main():
    cases = {}
    for spec in MX.recorded_specs():
        sim, _pools = MX.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert bool(sim._graph.arrays.has_flows) == bool(spec["flows"]), spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[MX.MIXED.key("case", spec)] = RF.run_case(spec, "mixed", want_trace=spec["name"] in MX.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        assert spec.get("auto") or spec["end_s"] <= 20.0
        bk = res["by_kind"]
        print(spec["name"], res["total_events"], "lim", bk[15:17].tolist(), "hc", bk[19:22].tolist(), "bh", bk[22:25].tolist(), "tw", bk[25:28].tolist(),
              "cl", bk[28:31].tolist(), "flow", bk[31:].tolist(), res["flow_stats"].tolist(), res["events_cancelled"], res["time_travel"], flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[MX.MIXED.key("case", MX.FIXTURES[name])]  # noqa: E731
    kinds = lambda r, a, b: r["by_kind"][EV[a]:EV[b] + 1].tolist()  # noqa: E731
    r = get("gate_flush_into_a_client_fixed_retry")
    assert r["total_events"] == 304 and kinds(r, "cl_req", "cl_timeout") == [25, 25, 25] and kinds(r, "gt_item", "gt_close") == [30, 2, 2], r["by_kind"]
    assert r["flow_stats"].tolist() == [[25, 20, 0, 2, 0, 5]] and r["events_cancelled"] == 0, r["flow_stats"]
    r = get("gate_flush_into_a_small_bulkhead")
    assert r["total_events"] == 161 and kinds(r, "bh_req", "bh_timeout") == [15, 10, 3] and kinds(r, "gt_item", "gt_close") == [30, 1, 1], r["by_kind"]
    assert r["flow_stats"].tolist() == [[15, 25, 0, 1, 0, 15]] and r["events_cancelled"] == 0, r["flow_stats"]
    r = get("client_server_batch_processor")
    assert r["total_events"] == 501 and kinds(r, "cl_req", "cl_timeout") == [41, 41, 39] and kinds(r, "bp_item", "bp_cont") == [38, 4, 11], r["by_kind"]
    assert r["flow_stats"][0, :4].tolist() == [11, 38, 4, 0] and r["events_cancelled"] == 7, r["flow_stats"]
    r = get("batch_into_a_timeout_wrapper_link_server")
    assert r["total_events"] == 613 and kinds(r, "tw_req", "tw_timeout") == [43, 78, 39] and kinds(r, "bp_item", "bp_cont") == [44, 3, 10], r["by_kind"]
    assert r["flow_stats"][0, :4].tolist() == [10, 43, 3, 1] and r["events_cancelled"] == 7, r["flow_stats"]
    r = get("cancelled_events_of_three_origins")
    assert r["events_cancelled"] > r["flow_stats"][0, 0] - r["flow_stats"][0, 2] >= 1, (r["events_cancelled"], r["flow_stats"])
    r = get("gate_events_and_an_early_checker_before_a_later_start_time")         # the `_GateOpen` of 1 s and the checker's first cycle of 0 s
    assert r["time_travel"] == 2 and kinds(r, "hc_cycle", "hc_timeout") == [0, 0, 0] and kinds(r, "gt_open", "gt_close") == [1, 2], r["by_kind"]
    assert sum(1 for c in cases.values() if c["time_travel"] > 0) >= 10
    assert len(MX.FIXTURES) >= 24 and len(MX.TRACED) >= 8 and MX.N_RANDOM >= 150
    MX.MIXED.write(cases)


if __name__ == "__main__":
    main()
