#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for Bulkhead and TimeoutWrapper (components/resilience/bulkhead.py, timeout.py)
-- the yardstick of tests/test_resilience_host.py and tests/test_gpu_resilience.py.  Run by hand where the reference is installed
(refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_resilience.py          # writes tests/golden/live_resilience/part_*.npz

Recorded (tests/recorded.py RESILIENCE reads them back; record_family.run_case is the run):
  * constructor defaults, properties, stats objects and the ValueError texts of both classes;
  * every spec of resilience_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs
    of make_golden.py choosing the random numbers -- everything the faults family records, what the health family records about
    LoadBalancers and checkers, plus per wrapper its statistics, its ids in flight
    and the ids of its wait queue, and the wrappers' Events processed (kinds 22 / 23 / 24 = a Request at a Bulkhead, its `_bh_response`,
    its `_bh_timeout`; 25 / 26 / 27 = the same of a TimeoutWrapper, in by_kind and in the trace); the fixtures of
    resilience_specs.TRACED with their full trace.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed): no case is left out.
"""
from __future__ import annotations

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import resilience_specs as XS  # noqa: E402
from happysimulator import Sink  # noqa: E402
from happysimulator.components.resilience import Bulkhead, TimeoutWrapper  # noqa: E402
from happysimulator.components.resilience.bulkhead import BulkheadStats  # noqa: E402
from happysimulator.components.resilience.timeout import TimeoutStats  # noqa: E402
from recorded import RESILIENCE as XR  # noqa: E402

EV_BH_REQ, EV_BH_RESP = RF.EV["bh_req"], RF.EV["bh_resp"]


def defaults():
    """Constructor state, properties, stats objects and error texts."""
    k = Sink("k")
    b, t = Bulkhead("b", k, max_concurrent=3), TimeoutWrapper("t", k, timeout=2.5)
    out = {}
    sb, st = b.stats, t.stats
    out["bulkhead"] = dict(fields=[b.max_concurrent, b.max_wait_queue, b.max_wait_time, b.active_count, b.queue_depth, b.available_permits,
                                   b._next_request_id, len(b._in_flight)], target_is=b.target is k,
                           downstream=[x.name for x in b.downstream_entities()], stats_type=type(sb).__name__,
                           stats_fields=[f for f in BulkheadStats.__dataclass_fields__],
                           stats=[getattr(sb, f) for f in BulkheadStats.__dataclass_fields__])
    out["timeout"] = dict(fields=[t.timeout, t.in_flight_count, t._next_request_id], target_is=t.target is k,
                          downstream=[x.name for x in t.downstream_entities()], stats_type=type(st).__name__,
                          stats_fields=[f for f in TimeoutStats.__dataclass_fields__], stats=[getattr(st, f) for f in TimeoutStats.__dataclass_fields__])
    for key, obj, attr in (("bulkhead", sb, "total_requests"), ("timeout", st, "total_requests")):
        try:
            setattr(obj, attr, 1)
            out[key]["stats_frozen"] = False
        except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
            out[key]["stats_frozen"] = type(e).__name__
    errors = []
    for kw in (dict(max_concurrent=0), dict(max_concurrent=-2), dict(max_concurrent=1, max_wait_queue=-1), dict(max_concurrent=1, max_wait_time=0),
               dict(max_concurrent=1, max_wait_time=-0.5), dict(max_concurrent=0, max_wait_queue=-1), dict(max_concurrent=1, max_wait_queue=0, max_wait_time=None)):
        try:
            Bulkhead("x", k, **kw)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["bulkhead"]["errors"] = errors
    errors = []
    for timeout in (0, -1.5, 0.0, 1e-9):
        try:
            TimeoutWrapper("x", k, timeout=timeout)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["timeout"]["errors"] = errors
    return out


def main():
    cases = {XR.key("defaults"): defaults()}
    for spec in XS.all_specs():
        sim, _pools = GF.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_wrappers, spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[XR.key("case", spec)] = RF.run_case(spec, "resilience", want_trace=spec["name"] in XS.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        print(spec["name"], res["total_events"], res["by_kind"][EV_BH_REQ:].tolist(), res["wrap_stats"][:, :5].tolist(), res["crashed"].sum(), flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[XR.key("case", XS.FIXTURES[name])]  # noqa: E731
    r = get("bulkhead_link_twenty_requests")              # 20 Requests through Bulkhead -> NetworkLink -> Server: 38 `_bh_response` Events
    assert r["by_kind"][EV_BH_REQ] == 20 and r["by_kind"][EV_BH_RESP] == 38, r["by_kind"][EV_BH_REQ:]
    r = get("paused_server_leaks_permits")                # every permit leaked during the pause: active_count == 4 and 3 queued at 10 s,
    assert r["wrap_stats"][0, 7] == 4 and r["wrap_stats"][0, 8] == 3 and r["wrap_stats"][0, 2] > 200, r["wrap_stats"]     # the rest rejected
    r = get("bulkhead_server_burst")
    assert r["wrap_stats"][0, 5] > 1                      # peak_concurrent above 1 in front of a Server
    r = get("timeout_response_after_the_wrappers_restart")
    assert r["wrap_stats"][0, 1] > 0 and r["wrap_stats"][0, 2] > 0
    r = get("timeout_wrapper_crash_without_restart")
    assert r["wrap_stats"][0, 3] > 0                      # entries stay in flight for ever
    r = get("expired_entries_skipped_after_a_wrapper_crash")
    assert r["wrap_stats"][0, 3] > 0
    assert len(XS.FIXTURES) >= 40 and len(XS.TRACED) == 6 and XS.N_RANDOM >= 120
    XR.write(cases)


if __name__ == "__main__":
    main()
