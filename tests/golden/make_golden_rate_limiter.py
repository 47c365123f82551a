#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for RateLimitedEntity and the Token/Leaky bucket and Sliding/Fixed window
policies (components/rate_limiter/) -- the yardstick of tests/test_rate_limiter_host.py and tests/test_gpu_rate_limiter.py.  Run by
hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_rate_limiter.py          # writes tests/golden/live_rate_limiter/part_*.npz

Recorded (tests/recorded.py RATE_LIMITER reads them back; record_family.run_case is the run):
  * constructor defaults, properties and ValueError texts of the classes;
  * per policy, call sequences (now_ns, method) -> (result, state) (rate_limiter_specs.policy_calls);
  * every spec of rate_limiter_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream
    plugs of make_golden.py choosing the random numbers -- every Sink record, per-entity statistics, the limiters' counters, queue
    depth, time series and final policy state, probe samples, event totals by kind (the limiters' two handlers as kinds 15 and 16,
    and per limiter), the first event beyond the end, how often `time_until_available` returned Duration(1); the named fixtures
    with their full trace;
  * per policy, the first seeded guard_spec whose run meets the 1-ns guard (or the number of tries that found none).
"""
from __future__ import annotations

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import rate_limiter_specs as RS  # noqa: E402
from happysimulator import Instant, Sink  # noqa: E402
from happysimulator.components.rate_limiter import policy as ref_policy  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from recorded import RATE_LIMITER as RR  # noqa: E402

def defaults():
    """Constructor state, properties and error texts."""
    out = {}
    tb, lb, sw, fw = ref_policy.TokenBucketPolicy(), ref_policy.LeakyBucketPolicy(), ref_policy.SlidingWindowPolicy(), ref_policy.FixedWindowPolicy(7)
    out["token"] = dict(capacity=tb.capacity, refill_rate=tb.refill_rate, tokens=tb.tokens, state=RS.policy_state(tb),
                        initial=ref_policy.TokenBucketPolicy(4, 2, 0.5).tokens, types=[type(tb.capacity).__name__, type(tb.refill_rate).__name__])
    out["leaky"] = dict(leak_rate=lb.leak_rate, interval=lb._leak_interval, state=RS.policy_state(lb),
                        zero_interval=ref_policy.LeakyBucketPolicy(0)._leak_interval)
    out["sliding"] = dict(window_size_seconds=sw.window_size_seconds, max_requests=sw.max_requests, state=RS.policy_state(sw))
    out["fixed"] = dict(requests_per_window=fw.requests_per_window, window_size=fw.window_size, state=RS.policy_state(fw))
    errors = []
    for args in ((0, 1.0), (-2, 1.0), (3, 0), (3, -0.5)):
        try:
            ref_policy.FixedWindowPolicy(*args)
        except ValueError as e:
            errors.append(str(e))
    out["fixed"]["errors"] = errors
    k = Sink("k")
    ent = RateLimitedEntity("lim", k, tb)
    s = ent.stats
    out["entity"] = dict(queue_capacity=ent._queue.capacity, queue_depth=ent.queue_depth, stats=[s.received, s.forwarded, s.queued, s.dropped],
                         stats_type=type(s).__name__, downstream_is=ent.downstream is k, policy_is=ent.policy is tb,
                         downstream_entities=[x.name for x in ent.downstream_entities()],
                         series=[ent.received_times, ent.forwarded_times, ent.dropped_times], poll_scheduled=ent._poll_scheduled)
    try:
        s.received = 1
        out["entity"]["stats_frozen"] = False
    except Exception as e:  # noqa: BLE001 -- dataclasses.FrozenInstanceError
        out["entity"]["stats_frozen"] = type(e).__name__
    return out


def policy_calls(kind, j):
    pol, calls = RS.policy_calls(kind, j)
    RS.replay.instant = Instant
    return dict(policy=pol, calls=np.array([[t, m == "try_acquire"] for t, m in calls], np.int64),
                results=np.array(RS.replay(RS.make_policy(ref_policy, pol), calls), np.float64))


def find_guard(kind):
    """The first try of rate_limiter_specs.guard_spec(kind, j) whose run meets the guard, as (j, result); (-tries, None) if none does."""
    for j in range(RS.GUARD_TRIES):
        res = RF.run_case(RS.guard_spec(kind, j), "rate_limiter")
        if int(res["lim_guard_hits"].sum()) > 0:
            return j, res
    return -RS.GUARD_TRIES, None


def main():
    cases = {RR.key("defaults"): defaults()}
    for kind in RS.POLICIES:
        for j in range(RS.N_POLICY_CALLS):
            cases[RR.key("policy_calls", kind, j)] = policy_calls(kind, j)
    covered = set()
    for spec in RS.all_specs():
        fixture = spec["name"] in RS.FIXTURES
        res = cases[RR.key("case", spec)] = RF.run_case(spec, "rate_limiter", want_trace=fixture and len(spec["servers"]) <= 16)
        for lm, up in zip(spec["limiters"], spec.get("limiter_upstreams") or []):
            covered.add((lm["policy"][0], up))
        print(spec["name"], res["total_events"], res["lim_stats"][:2].tolist(), int(res["lim_guard_hits"].sum()), flush=True)
    missing = [(p, u) for p in RS.POLICIES for u in RS.UPSTREAMS if (p, u) not in covered]
    assert not missing, f"the random graphs never put these policies behind these upstreams: {missing}"
    for kind, (rec, fwd, qd, dr, ev) in RS.ISSUE_VALUES.items():
        res = cases[RR.key("case", RS.FIXTURES[f"{kind}_constant"])]
        assert res["lim_stats"][0, :4].tolist() == [rec, fwd, qd, dr] and res["total_events"] == ev, (kind, res["lim_stats"], res["total_events"])
    for kind in RS.POLICIES:
        j, res = find_guard(kind)
        cases[RR.key("guard", kind)] = dict(tries=j, result=res)
        print("guard", kind, j, flush=True)
    RR.write(cases)


if __name__ == "__main__":
    main()
