#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for Client and its retry policies (components/client/client.py, retry.py) -- the
yardstick of tests/test_client_host.py and tests/test_gpu_client.py.  Run by hand where the reference is installed (refshim.py:
HS_REFERENCE_ROOT):

    python tests/golden/make_golden_client.py          # writes tests/golden/live_client/part_*.npz

Recorded (tests/recorded.py CLIENT reads them back; record_family.run_case is the run):
  * constructor defaults, properties, stats objects and the ValueError texts of Client and the four policies, and
    get_delay(1 .. max_attempts) of FixedRetry and ExponentialBackoff over a parameter grid that includes the max_delay cap;
  * every spec of client_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream plugs of
    make_golden.py choosing the random numbers -- everything the resilience family records, plus per Client its statistics, its keys in flight and its response times, and the Clients' Events processed
    (kinds 28 / 29 / 30 = a request at a Client, its `_client_response`, its `_client_timeout`, in by_kind and in the trace); the
    fixtures of client_specs.TRACED with their full trace.
The recorder asserts that every spec is one the product accepts (its host-side lowering, no device needed): no case is left out.
"""
from __future__ import annotations

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import client_specs as CS  # noqa: E402
import graph_family as GF  # noqa: E402
import happysimulator.components.client as ref_client  # noqa: E402
from happysimulator import Sink  # noqa: E402
from happysimulator.components.client import Client, DecorrelatedJitter, ExponentialBackoff, FixedRetry, NoRetry  # noqa: E402
from happysimulator.components.client.client import ClientStats  # noqa: E402
from happysimulator.core.temporal import Duration  # noqa: E402
from recorded import CLIENT as CR  # noqa: E402

EV_CL_REQ, EV_CL_RESP = RF.EV["cl_req"], RF.EV["cl_resp"]
FIXED_GRID = [(1, 0.0), (3, 0.25), (5, 0), (2, 1), (4, 1e-9)]
EXP_GRID = [(6, 0.1, 1.0, 2.0), (1, 0.1, 0.1, 2.0), (5, 0.05, 0.05, 3.0), (8, 0.001, 10.0, 10.0), (4, 0.3, 0.5, 1.0), (6, 0.1, 0.25, 2.0), (12, 1, 60, 1.5)]
CLIENT_ERRORS = (dict(timeout=-1), dict(timeout=-0.5), dict(timeout=0), dict(timeout=None), dict(timeout=0.0))
POLICY_ERRORS = (("fixed", (0, 0.1)), ("fixed", (1, -0.1)), ("fixed", (-1, -1)), ("fixed", (1, 0)),
                 ("exp", (0, 0.1, 1.0)), ("exp", (1, 0, 1.0)), ("exp", (1, 0.5, 0.1)), ("exp", (1, 0.1, 1.0, 0.5)), ("exp", (1, 0.1, 1.0, 2.0, -0.1)),
                 ("exp", (1, 0.1, 0.1)), ("jitter", (0, 0.1, 1.0)), ("jitter", (1, 0, 1.0)), ("jitter", (1, 0.5, 0.1)), ("jitter", (1, 0.1, 0.1)))


def policy_error(ns, kind, args):
    cls = {"fixed": ns.FixedRetry, "exp": ns.ExponentialBackoff, "jitter": ns.DecorrelatedJitter}[kind]
    try:
        cls(*args)
        return None
    except ValueError as e:
        return str(e)


def defaults():
    """Constructor state, properties, stats objects, error texts and delay tables."""
    k = Sink("k")
    c = Client("c", k)
    st = c.stats
    out = dict(fields=[c.timeout, type(c.retry_policy).__name__, c.in_flight_count, c.average_response_time, c._next_request_id,
                       c.get_response_time_percentile(0.5), len(c._response_times)],
               target_is=c.target is k, downstream=[x.name for x in c.downstream_entities()], stats_type=type(st).__name__,
               stats_fields=[f for f in ClientStats.__dataclass_fields__], stats=[getattr(st, f) for f in ClientStats.__dataclass_fields__])
    try:
        st.timeouts = 1
        out["stats_frozen"] = False
    except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
        out["stats_frozen"] = type(e).__name__
    errors = []
    for kw in CLIENT_ERRORS:
        try:
            Client("x", k, **kw)
            errors.append(None)
        except ValueError as e:
            errors.append(str(e))
    out["errors"] = errors
    out["policy_errors"] = [policy_error(ref_client, kind, args) for kind, args in POLICY_ERRORS]
    # send_request: the ids, the metadata and the time without a clock
    ev1, ev2 = c.send_request(), c.send_request(payload={"a": 1}, event_type="get")
    out["send_request"] = dict(ids=[ev1.context["metadata"]["request_id"], ev2.context["metadata"]["request_id"]], next_id=c._next_request_id,
                               metadata_keys=sorted(ev1.context["metadata"]), attempt=ev1.context["metadata"]["attempt"],
                               client_name=ev1.context["metadata"]["client_name"], payload=ev2.context["metadata"]["payload"]["a"],
                               types=[ev1.event_type, ev2.event_type], time_ns=ev1.time.nanoseconds, target_is=ev1.target is c)
    n, f, e, j = NoRetry(), FixedRetry(3, 0.25), ExponentialBackoff(4, 0.1, 1.0), DecorrelatedJitter(3, 0.1, 1.0)
    out["policies"] = dict(no_retry=[n.should_retry(1), n.should_retry(100), n.get_delay(1), n.get_delay(7)],
                           fixed=[f.max_attempts, f.delay, [f.should_retry(a) for a in range(1, 5)]],
                           exp=[e.max_attempts, e.initial_delay, e.max_delay, e.multiplier, e.jitter, [e.should_retry(a) for a in range(1, 6)]],
                           jitter=[j.max_attempts, j.base_delay, j.max_delay, [j.should_retry(a) for a in range(1, 5)], j._previous_delay])
    out["fixed_delays"] = [[FixedRetry(m, d).get_delay(a) for a in range(1, m + 1)] for m, d in FIXED_GRID]
    out["exp_delays"] = [[ExponentialBackoff(*g).get_delay(a) for a in range(1, g[0] + 1)] for g in EXP_GRID]
    # Duration.from_seconds of every delay: what the timeout handler adds to `now`
    out["fixed_delays_ns"] = [[Duration.from_seconds(x).nanoseconds for x in row] for row in out["fixed_delays"]]
    out["exp_delays_ns"] = [[Duration.from_seconds(x).nanoseconds for x in row] for row in out["exp_delays"]]
    return out


def main():
    cases = {CR.key("defaults"): defaults()}
    for spec in CS.all_specs():
        sim, _pools = GF.build(spec)
        sim.lowered()                                      # the product takes this graph (host-side lowering; raises otherwise)
        assert sim._graph.arrays.has_clients, spec["name"]
        sim._general_prepare(sim._graph, bool(spec.get("auto")))     # ... and every scheduled Event of it
        res = cases[CR.key("case", spec)] = RF.run_case(spec, "client", want_trace=spec["name"] in CS.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        print(spec["name"], res["total_events"], res["by_kind"][EV_CL_REQ:].tolist(), res["cl_stats"].tolist(), res["crashed"].sum(), flush=True)
    # what the issue states about the reference, pinned on the recordings
    get = lambda name: cases[CR.key("case", CS.FIXTURES[name])]  # noqa: E731
    d = cases[CR.key("defaults")]
    assert d["exp_delays"][0] == [0.1, 0.1, 0.2, 0.4, 0.8, 1.0], d["exp_delays"][0]
    assert d["errors"] == ["timeout must be >= 0, got -1", "timeout must be >= 0, got -0.5", None, None, None]      # timeout = 0 is legal
    r = get("keyless_ten_plain_events")                    # 10 plain Events at 0.0 .. 0.9 s, timeout 0.5, the Server paused over [0.25, 0.55)
    assert r["cl_stats"][0].tolist() == [10, 3, 5, 0, 5, 0, 0], r["cl_stats"]
    r = get("link_double_response_twenty_requests")        # Client(0.02, FixedRetry(2, 0.05)) -> NetworkLink(0.03) -> Server(0.01) -> Sink
    assert r["cl_stats"][0, :5].tolist() == [40, 0, 40, 20, 20] and r["by_kind"][EV_CL_RESP] == 80 and r["received"][0] == 40, (r["cl_stats"], r["by_kind"])
    assert np.array_equal(r["sink_latency_s"], np.full(40, 0.04)), r["sink_latency_s"]       # created_at is the send time of the attempt
    r = get("timeout_zero_sink")                           # the timeout was constructed before the response and pops first
    assert r["cl_stats"][0, :5].tolist() == [15, 0, 15, 10, 5] and r["received"][0] == 15, r["cl_stats"]
    r = get("retry_lands_after_the_restart")
    assert r["cl_stats"][0, :5].tolist() == [3, 1, 2, 2, 0], r["cl_stats"]
    r = get("late_response_of_attempt_one")
    assert r["cl_stats"][0, :5].tolist() == [6, 0, 6, 3, 3] and r["by_kind"][EV_CL_RESP] == 12, (r["cl_stats"], r["by_kind"])    # every response (two per attempt: link and Sink) is late: a no-op
    r = get("client_crash_without_restart")
    assert r["cl_stats"][0, 5] > 0                         # entries stay in flight for ever
    r = get("source_plain_and_send_request_mixed")
    assert r["cl_stats"][0, 6] == 4
    assert len(CS.FIXTURES) >= 40 and len(CS.TRACED) == 6 and CS.N_RANDOM >= 120
    CR.write(cases)


if __name__ == "__main__":
    main()
