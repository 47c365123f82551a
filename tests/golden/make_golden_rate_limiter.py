#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for RateLimitedEntity and the Token/Leaky bucket and Sliding/Fixed window
policies (components/rate_limiter/) -- the yardstick of tests/test_rate_limiter_host.py and tests/test_gpu_rate_limiter.py.  Run by
hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_rate_limiter.py          # writes tests/golden/live_rate_limiter/part_*.npz

Recorded (tests/rate_limiter_reference.py reads them back):
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

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import rate_limiter_specs as RS  # noqa: E402
import strategy_specs as SS  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the reference's import path; the stream plugs and the trace classifier)
import make_golden_strategies as MGS  # noqa: E402
import hs_streams_py as hs  # noqa: E402
from happysimulator import ConstantLatency, Instant, Server, Simulation, Sink, Source  # noqa: E402
from happysimulator.components.load_balancer.load_balancer import LoadBalancer  # noqa: E402
from happysimulator.components.network.link import NetworkLink  # noqa: E402
from happysimulator.components.rate_limiter import policy as ref_policy  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from happysimulator.core.event import Event  # noqa: E402
from happysimulator.core.temporal import Duration  # noqa: E402
from happysimulator.instrumentation.probe import Probe  # noqa: E402
from happysimulator.load.profile import ConstantRateProfile  # noqa: E402
from happysimulator.load.providers.constant_arrival import ConstantArrivalTimeProvider  # noqa: E402
from happysimulator.load.source import SimpleEventProvider  # noqa: E402

EV_LIM_REQUEST, EV_LIM_POLL = len(MG.EV), len(MG.EV) + 1
REF_METRIC = dict({k: v[1] for k, v in MG.PROBE_METRICS.items()}, queue_depth="queue_depth")


MAX_EVENTS = 60_000


class Livelock(RuntimeError):
    pass


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


class _Reference:
    """rate_limiter_specs.wire's factory over the reference's classes (streams: Source k ARRIVAL / KEY base k, Server s SERVICE base
    s, link l LINK / LOSS base l, router r ROUTE base r)."""

    def __init__(self, spec):
        self.spec, self.seed = spec, spec["seed"]
        self.probe_data = []

    def sink(self, j):
        return Sink(f"sink{j}")

    def server(self, i, sv):
        return Server(f"srv{i}", concurrency=sv.get("c", 1), queue_capacity=sv.get("cap"),
                      service_time=(ConstantLatency(sv["mean"]) if sv.get("svc") == "const" else
                                    MG.PhiloxExponentialLatency(sv["mean"], hs.Stream(self.seed, i, hs.STREAM_SERVICE))))

    def limiter(self, i, lm):
        ent = RateLimitedEntity(f"lim{i}", None, RS.make_policy(ref_policy, lm["policy"]), queue_capacity=lm["cap"])
        ent._guard_hits = 0
        orig = ent.policy.time_until_available

        def counted(now, _orig=orig, _ent=ent):
            w = _orig(now)
            if w == Duration(1):
                _ent._guard_hits += 1
            return w

        ent.policy.time_until_available = counted
        return ent

    def link(self, l, lk):
        jit = None
        if lk.get("jm") is not None and lk.get("jk") == "exp":
            jit = MG.PhiloxExponentialLatency(lk["jm"], hs.Stream(self.seed, l, hs.STREAM_LINK))
        elif lk.get("jm") is not None and lk.get("jk") == "const":
            jit = ConstantLatency(lk["jm"])
        link = NetworkLink(f"link{l}", latency=ConstantLatency(lk["lat"]), jitter=jit, packet_loss_rate=lk.get("loss", 0.0), egress=None)
        link._loss_stream = hs.Stream(self.seed, l, hs.STREAM_LOSS)
        return link

    def lb(self, j, lb, backends):
        return SS.make_lb(LoadBalancer, j, lb, backends, MGS._strategy(lb))

    def router(self, r, targets):
        return MG.PhiloxRandomRouter(f"router{r}", targets=targets, stream=hs.Stream(self.seed, r, hs.STREAM_ROUTE))

    def source(self, k, sc, to):
        prof = ConstantRateProfile(rate=sc["rate"])
        prov = (MG.PhiloxPoissonArrival(prof, Instant.Epoch, hs.Stream(self.seed, k, hs.STREAM_ARRIVAL)) if sc["kind"] == "poisson"
                else ConstantArrivalTimeProvider(prof, start_time=Instant.Epoch))
        ep = (MG.PhiloxClientProvider(to, sc["n_clients"], hs.Stream(self.seed, k, hs.STREAM_KEY)) if sc.get("n_clients")
              else SimpleEventProvider(to, "Request", None))
        return Source(f"src{k}", ep, prov)

    def probe(self, target, metric, interval):
        probe, data = Probe.on(target, REF_METRIC[metric], interval=interval)
        data._ns = []

        def add_stat(value, time, _orig=data.add_stat, _d=data):
            _d._ns.append((time.nanoseconds, value))
            _orig(value, time)

        data.add_stat = add_stat
        self.probe_data.append(data)
        return probe


def run_case(spec, want_trace=False):
    """The reference's run of one spec.  Trace nodes: Sources, Probes, then the entities (servers + lbs + routers + links + limiters
    + sinks); trace kinds: make_golden.EV, then 15 = a Request at a limiter, 16 = a limiter's poll."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    F = _Reference(spec)
    pools, sources, probes, entities = RS.wire(spec, F)
    servers, sinks, links, routers, lbs, lims = (pools[k] for k in ("server", "sink", "link", "router", "lb", "limiter"))
    sim = Simulation(start_time=MG._start(spec), sources=sources, entities=entities,
                     **({} if spec.get("auto") else {"end_time": MG._at(spec, spec["end_s"])}), **({"probes": probes} if probes else {}))
    node_of = {}
    for i, x in enumerate(sources + probes):
        node_of[id(x)] = i
    first = len(sources) + len(probes)
    lim_index = {}
    for i, x in enumerate(entities):
        node_of[id(x)] = first + i
        if isinstance(x, Server):
            for part in (x._queue, x._driver, x._worker):
                node_of[id(part)] = first + i
        if isinstance(x, RateLimitedEntity):
            lim_index[id(x)] = len(lim_index)
    cb_probe = {id(p._event_provider.data_sink): len(sources) + j for j, p in enumerate(probes)}
    by_kind = np.zeros(EV_LIM_POLL + 1, np.int64)
    lim_events = np.zeros((len(lims), 2), np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop

    def pop():
        e = orig_pop()
        if by_kind.sum() >= MAX_EVENTS:
            # FixedWindowPolicy.time_until_available answers Duration.ZERO when `remaining <= 0`; where the float floor division puts a
            # window's last nanosecond + 1 into the OLD window (0.3 // 0.1 == 2.0), the poll at that boundary finds the window still
            # full and is rescheduled for the same nanosecond for ever.  The reference never returns from such a run: not recordable.
            raise Livelock(spec["name"])
        if isinstance(e.target, RateLimitedEntity):
            poll = e.event_type == f"rate_limit_poll::{e.target.name}"
            k, nd = (EV_LIM_POLL if poll else EV_LIM_REQUEST), node_of[id(e.target)]
            lim_events[lim_index[id(e.target)], int(poll)] += 1
        else:
            k, nd = MG.classify(e, node_of)
        if k == MG.EV["probe"]:
            fn = e.target._fn if hasattr(e.target, "_fn") else e.target.fn
            cells = {id(cell.cell_contents) for cell in (fn.__closure__ or ())}
            nd = next(c for key, c in cb_probe.items() if key in cells)
        by_kind[k] += 1
        if want_trace:
            trace.append((e.time.nanoseconds, k, nd, e._sort_index))
        return e

    heap.pop = pop
    for (kind, idx), t_s in spec.get("schedule") or []:
        sim.schedule(Event(time=MG._at(spec, t_s), event_type="Request", target=pools[kind][idx]))
    summary = MG.run_sim_windows(sim, spec)
    out = dict(total_events=int(summary.total_events_processed), final_ns=int(sim._current_time.nanoseconds), by_kind=by_kind)
    assert int(by_kind.sum()) == out["total_events"], "every popped event was processed (no time travel, nothing cancelled)"
    out["pending_events"] = int(heap.size())
    out["generated"] = np.array([s.generated_count for s in sources], np.int64)
    out["accepted"] = np.array([s.stats_accepted for s in servers], np.int64)
    out["dropped"] = np.array([s.stats_dropped for s in servers], np.int64)
    out["completed"] = np.array([s._requests_completed for s in servers], np.int64)
    out["rejected"] = np.array([s._requests_rejected for s in servers], np.int64)
    out["depth"] = np.array([s.depth for s in servers], np.int64)
    out["active"] = np.array([s.active_requests for s in servers], np.int64)
    out["total_service_s"] = np.array([s._total_service_time for s in servers], np.float64)
    out["received"] = np.array([k.events_received for k in sinks], np.int64)
    out["routed"] = np.array([r.stats_routed for r in routers], np.int64)
    out["packets_sent"] = np.array([l.packets_sent for l in links], np.int64)
    out["packets_dropped"] = np.array([l.packets_dropped for l in links], np.int64)
    out["lb_stats"] = np.array([[lb.stats.requests_received, lb.stats.requests_forwarded, lb.stats.requests_failed,
                                 lb.stats.no_backend_available, len(lb._in_flight)] for lb in lbs], np.int64).reshape(-1, 5)
    tot, toff, index = [], [0], []
    for j, lb in enumerate(lbs):
        tot.extend(lb.get_backend_info(servers[b]).total_requests for b in spec["lbs"][j]["backends"])
        toff.append(len(tot))
        st = lb.strategy
        index.append(st._fallback._index if hasattr(st, "_fallback") else getattr(st, "_index", -1))
    out["lb_backend_total_requests"] = np.asarray(tot, np.int64)
    out["lb_backend_off"] = np.asarray(toff, np.int64)
    out["lb_rr_index"] = np.asarray(index, np.int64)
    sink_t, sink_lat, off = [], [], [0]
    for k in sinks:
        sink_t.extend(t.nanoseconds for t in k.completion_times)
        sink_lat.extend(k.latencies_s)
        off.append(len(sink_t))
    out["sink_t_ns"] = np.asarray(sink_t, np.int64)
    out["sink_latency_s"] = np.asarray(sink_lat, np.float64)
    out["sink_off"] = np.asarray(off, np.int64)
    pt, pv, poff = [], [], [0]
    for d in F.probe_data:
        pt.extend(t for t, _ in d._ns)
        pv.extend(int(v) for _, v in d._ns)
        poff.append(len(pt))
    out["probe_t_ns"], out["probe_v"], out["probe_off"] = np.asarray(pt, np.int64), np.asarray(pv, np.int64), np.asarray(poff, np.int64)
    out.update(RS.limiter_results(lims))
    out["lim_events"] = lim_events
    out["lim_guard_hits"] = np.array([x._guard_hits for x in lims], np.int64)
    es = summary.entities
    out["entity_summaries"] = {x.name: [es[x.name].entity_type, int(es[x.name].events_handled), es[x.name].queue_stats is None] for x in lims}
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out


def find_guard(kind):
    """The first try of rate_limiter_specs.guard_spec(kind, j) whose run meets the guard, as (j, result); (-tries, None) if none does."""
    for j in range(RS.GUARD_TRIES):
        res = run_case(RS.guard_spec(kind, j))
        if int(res["lim_guard_hits"].sum()) > 0:
            return j, res
    return -RS.GUARD_TRIES, None


def main():
    import rate_limiter_reference as RR

    cases = {RR.key("defaults"): defaults()}
    for kind in RS.POLICIES:
        for j in range(RS.N_POLICY_CALLS):
            cases[RR.key("policy_calls", kind, j)] = policy_calls(kind, j)
    covered = set()
    for spec in RS.all_specs():
        fixture = spec["name"] in RS.FIXTURES
        res = cases[RR.key("case", spec)] = run_case(spec, want_trace=fixture and len(spec["servers"]) <= 16)
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
