"""The one run of the LIVE upstream reference behind tests/golden/make_golden_{rate_limiter,faults,health,resilience,client,flow,mixed}.py: the
reference's own event loop over its own components, wired by tests/graph_family.py's wire() like the product's, with the Philox
stream plugs of make_golden.py choosing the random numbers.  Importing this module puts tests/, tests/golden/ and the repository
root (the product: the recorders assert that it takes every spec) on sys.path, so a recorder starts from a clean shell.

`run_case(spec, family)` records a common core -- event totals by kind, the first event beyond the end -- and the family's SECTIONS
in their order (a recorded dict keeps its insertion order in the file).  Trace rows: (time ns, kind, node, sort index) of every
processed Event; nodes: Sources, Probes, then the entities in wire()'s order; kinds: EV below.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import client_specs as CS  # noqa: E402
import fault_specs as FS  # noqa: E402
import flow_specs as FL  # noqa: E402
import graph_family as GF  # noqa: E402
import health_specs as HS  # noqa: E402
import rate_limiter_specs as RS  # noqa: E402
import resilience_specs as XS  # noqa: E402
import strategy_specs as SS  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the reference's import path; the stream plugs and the trace classifier)
import hs_streams_py as hs  # noqa: E402
import happysimulator.components.client as ref_client  # noqa: E402
import happysimulator.components.industrial.batch_processor as ref_bp  # noqa: E402
import happysimulator.components.industrial.conveyor as ref_cv  # noqa: E402
import happysimulator.components.industrial.gate_controller as ref_gt  # noqa: E402
import happysimulator.faults as ref_faults  # noqa: E402
from happysimulator import ConstantLatency, Instant, Server, Simulation, Sink, Source  # noqa: E402
from happysimulator.components.load_balancer import HealthChecker  # noqa: E402
from happysimulator.components.load_balancer import strategies as ref_strategies  # noqa: E402
from happysimulator.components.load_balancer.load_balancer import LoadBalancer  # noqa: E402
from happysimulator.components.network.link import NetworkLink  # noqa: E402
from happysimulator.components.rate_limiter import policy as ref_policy  # noqa: E402
from happysimulator.components.rate_limiter.rate_limited_entity import RateLimitedEntity  # noqa: E402
from happysimulator.components.resilience import Bulkhead, TimeoutWrapper  # noqa: E402
from happysimulator.core.event import Event, ProcessContinuation  # noqa: E402
from happysimulator.core.temporal import Duration  # noqa: E402
from happysimulator.instrumentation.probe import Probe  # noqa: E402
from happysimulator.load.profile import ConstantRateProfile  # noqa: E402
from happysimulator.load.providers.constant_arrival import ConstantArrivalTimeProvider  # noqa: E402
from happysimulator.load.source import SimpleEventProvider  # noqa: E402

BatchProcessor, ConveyorBelt, GateController = ref_bp.BatchProcessor, ref_cv.ConveyorBelt, ref_gt.GateController
# trace / by_kind kinds: make_golden.EV (0 .. 14), then what each family added
EV = dict(MG.EV)
for _name in ("lim_request", "lim_poll",                                   # 15, 16: a Request at a limiter, a limiter's poll
              "fault_on", "fault_off",                                     # 17, 18: a crash / pause, a restart / resume
              "hc_cycle", "hc_resp", "hc_timeout",                         # 19 .. 21: a checker's cycle / response / timeout
              "bh_req", "bh_resp", "bh_timeout",                           # 22 .. 24: a Request at a Bulkhead, its response, its timeout
              "tw_req", "tw_resp", "tw_timeout",                           # 25 .. 27: the same of a TimeoutWrapper
              "cl_req", "cl_resp", "cl_timeout",                           # 28 .. 30: the same of a Client
              *FL.EV_FLOW):                                                # 31 .. 38: a Request at a BatchProcessor, its `_BatchTimeout`, the
    EV[_name] = len(EV)                                                    # continuation of a batch; a Request at a ConveyorBelt, the continuation
assert EV["lim_request"] == 15 and EV["cl_req"] == 28                      # of its transit; a Request at a GateController, `_GateOpen`, `_GateClose`
assert EV["bp_item"] == FL.EV_FLOW_FIRST and len(EV) == 39
N_KINDS = dict(rate_limiter=EV["lim_poll"] + 1, faults=EV["fault_off"] + 1, health=EV["hc_timeout"] + 1, resilience=EV["tw_timeout"] + 1,
               client=EV["cl_timeout"] + 1, flow=len(EV), mixed=len(EV))
_FAULT_ON = ("fault.crash:", "fault.pause:")
_FAULT_OFF = ("fault.restart:", "fault.resume:")
# event_type -> kind of the Events an entity sends itself; any other Event at it is a request
_OWN_KINDS = {HealthChecker: {"_health_check_cycle": EV["hc_cycle"], "_health_check_response": EV["hc_resp"], "_health_check_timeout": EV["hc_timeout"]},
              Bulkhead: {"_bh_response": EV["bh_resp"], "_bh_timeout": EV["bh_timeout"], None: EV["bh_req"]},
              TimeoutWrapper: {"_tw_response": EV["tw_resp"], "_tw_timeout": EV["tw_timeout"], None: EV["tw_req"]},
              ref_client.Client: {"_client_response": EV["cl_resp"], "_client_timeout": EV["cl_timeout"], None: EV["cl_req"]}}
# a Probe's metric -> the reference attribute it reads (the limiters', wrappers' and Clients' metrics go by their own names)
REF_METRIC = dict({k: v[1] for k, v in MG.PROBE_METRICS.items()}, queue_depth="queue_depth", active_count="active_count",
                  available_permits="available_permits", in_flight_count="in_flight_count", buffer_depth="buffer_depth",
                  items_in_transit="items_in_transit")
REF_STRATEGY = {"wrr": "WeightedRoundRobin", "ip_hash": "IPHash", "least_conn": "LeastConnections", "wlc": "WeightedLeastConnections",
                "round_robin": "RoundRobin", "chash": "ConsistentHash", "random": "Random"}
# where wire() and make_schedule() find the reference's classes
REF_NS = types.SimpleNamespace(Bulkhead=Bulkhead, TimeoutWrapper=TimeoutWrapper, HealthChecker=HealthChecker, Client=ref_client.Client,
                               FixedRetry=ref_client.FixedRetry, ExponentialBackoff=ref_client.ExponentialBackoff,
                               FaultSchedule=ref_faults.FaultSchedule, CrashNode=ref_faults.CrashNode, PauseNode=ref_faults.PauseNode,
                               BatchProcessor=BatchProcessor, ConveyorBelt=ConveyorBelt, GateController=GateController)
MAX_EVENTS = 60_000


class Livelock(RuntimeError):
    pass


def ref_strategy(lb):
    """The reference's strategy object of a spec's LoadBalancer."""
    kind = lb["strategy"]
    if kind == "chash":
        return ref_strategies.ConsistentHash(virtual_nodes=lb["vnodes"])
    if kind == "random":
        ref_strategies.random = MG._PerRequestChoice
        return ref_strategies.Random()
    return getattr(ref_strategies, REF_STRATEGY[kind])()


def recording_probe(target, attr, interval):
    """(Probe, its data) of the reference with every sample kept as (time ns, value) in `data._ns`."""
    probe, data = Probe.on(target, attr, interval=interval)
    data._ns = []

    def add_stat(value, time, _orig=data.add_stat, _d=data):
        _d._ns.append((time.nanoseconds, value))
        _orig(value, time)

    data.add_stat = add_stat
    return probe, data


class _Reference:
    """graph_family.wire's factory over the reference's classes (streams: Source k ARRIVAL / KEY base k, Server s SERVICE base
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
        return SS.make_lb(LoadBalancer, j, lb, backends, ref_strategy(lb))

    def router(self, r, targets):
        return MG.PhiloxRandomRouter(f"router{r}", targets=targets, stream=hs.Stream(self.seed, r, hs.STREAM_ROUTE))

    def source(self, k, sc, to):
        prof = ConstantRateProfile(rate=sc["rate"])
        prov = (MG.PhiloxPoissonArrival(prof, Instant.Epoch, hs.Stream(self.seed, k, hs.STREAM_ARRIVAL)) if sc["kind"] == "poisson"
                else ConstantArrivalTimeProvider(prof, start_time=Instant.Epoch))
        if sc.get("stop_s") is not None:                   # (a Source that stops handing out Requests: tests/flow_specs.py)
            assert sc["kind"] == "constant" and not sc.get("n_clients")
        ep = (MG.PhiloxClientProvider(to, sc["n_clients"], hs.Stream(self.seed, k, hs.STREAM_KEY)) if sc.get("n_clients")
              else SimpleEventProvider(to, "Request", None if sc.get("stop_s") is None else MG._at(self.spec, sc["stop_s"])))
        return Source(f"src{k}", ep, prov)

    def probe(self, target, metric, interval):
        probe, data = recording_probe(target, REF_METRIC[metric], interval)
        self.probe_data.append(data)
        return probe


def classify(e, node_of, by_name):
    """(kind, node) of a popped Event; a fault Event's node is the entity it names (the schedule's own dict order: the last of a
    name wins)."""
    et = e.event_type
    if et.startswith(_FAULT_ON) or et.startswith(_FAULT_OFF):
        return (EV["fault_on"] if et.startswith(_FAULT_ON) else EV["fault_off"]), by_name[et.split(":", 1)[1]]
    t = e.target
    if isinstance(t, BatchProcessor):
        return (EV["bp_cont"] if isinstance(e, ProcessContinuation) else EV["bp_timeout"] if et == "_BatchTimeout" else EV["bp_item"]), node_of[id(t)]
    if isinstance(t, ConveyorBelt):
        return (EV["cv_cont"] if isinstance(e, ProcessContinuation) else EV["cv_item"]), node_of[id(t)]
    if isinstance(t, GateController):
        return (EV["gt_open"] if et == "_GateOpen" else EV["gt_close"] if et == "_GateClose" else EV["gt_item"]), node_of[id(t)]
    own = _OWN_KINDS.get(type(e.target))
    if own is not None:
        return own[et if et in own else None], node_of[id(e.target)]
    if isinstance(e.target, RateLimitedEntity):
        return (EV["lim_poll"] if et == f"rate_limit_poll::{e.target.name}" else EV["lim_request"]), node_of[id(e.target)]
    return MG.classify(e, node_of)


# ---- what a family records after the common core, in its order ---------------------------------------------------------------------
def _stats(c):
    spec, sources, servers, sinks, links, routers, lbs = (c.spec, c.sources, *(c.pools[k] for k in ("server", "sink", "link", "router", "lb")))
    out = {}
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
    return out


def _probes(c):
    pt, pv, poff = [], [], [0]
    for d in c.F.probe_data:
        pt.extend(t for t, _ in d._ns)
        pv.extend(int(v) for _, v in d._ns)
        poff.append(len(pt))
    return dict(probe_t_ns=np.asarray(pt, np.int64), probe_v=np.asarray(pv, np.int64), probe_off=np.asarray(poff, np.int64))


def _guard_hits(c):
    lims, es = c.pools["limiter"], c.summary.entities
    return dict(lim_guard_hits=np.array([x._guard_hits for x in lims], np.int64),
                entity_summaries={x.name: [es[x.name].entity_type, int(es[x.name].events_handled), es[x.name].queue_stats is None] for x in lims})


_SECTION = dict(
    time_travel=lambda c: dict(time_travel=int(c.skipped)),
    stats=_stats,
    probes=_probes,
    limiters=lambda c: dict(RS.limiter_results(c.pools["limiter"]), lim_events=c.lim_events),
    guard_hits=_guard_hits,
    faults=lambda c: FS.fault_results(c.fs, GF.fault_targets(c.pools)),
    health=lambda c: HS.health_results(c.spec, c.pools),
    # probe_drops: probes a full bounded queue refused (their checks pass all the same)
    health_events=lambda c: dict(health_events=c.by_kind[EV["hc_cycle"]:].copy(), probe_drops=int(c.probe_drops)),
    probe_drops=lambda c: dict(probe_drops=int(c.probe_drops)),
    wrappers=lambda c: XS.wrapper_results(c.pools),
    clients=lambda c: CS.client_results(c.pools),
    flows=lambda c: FL.flow_results(c.pools),
    fault_events=lambda c: dict(fault_events=int(c.by_kind[EV["fault_on"]] + c.by_kind[EV["fault_off"]])),
    cancelled=lambda c: dict(events_cancelled=int(c.summary.events_cancelled)),
)
SECTIONS = dict(
    rate_limiter=("stats", "probes", "limiters", "guard_hits"),
    faults=("time_travel", "stats", "probes", "limiters", "faults", "fault_events", "cancelled"),
    health=("time_travel", "stats", "faults", "health", "health_events", "cancelled"),
    resilience=("time_travel", "stats", "probes", "limiters", "faults", "health", "wrappers", "fault_events", "cancelled"),
    client=("time_travel", "stats", "probes", "limiters", "faults", "health", "wrappers", "clients", "fault_events", "cancelled"),
    flow=("time_travel", "stats", "probes", "limiters", "faults", "flows", "fault_events", "cancelled"),
    mixed=("time_travel", "stats", "probes", "limiters", "faults", "health", "probe_drops", "wrappers", "clients", "flows", "fault_events", "cancelled"),
)


def run_case(spec, family, want_trace=False):
    """The reference's run of one spec as `family` records it."""
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    c = types.SimpleNamespace(spec=spec, F=_Reference(spec), skipped=0, probe_drops=0)
    c.pools, c.sources, probes, entities = GF.wire(spec, c.F, REF_NS)
    c.fs, handles = GF.make_schedule(REF_NS, spec, c.pools)
    early = GF.early_starts(spec, c.pools)
    sim = Simulation(start_time=MG._start(spec), sources=c.sources, entities=entities,
                     **({"fault_schedule": c.fs} if "faults" in SECTIONS[family] else {}),
                     **({} if spec.get("auto") else {"end_time": MG._at(spec, spec["end_s"])}), **({"probes": probes} if probes else {}))
    GF.cancel_after(spec, handles)
    node_of = {}
    for i, x in enumerate(c.sources + probes):
        node_of[id(x)] = i
    first = len(c.sources) + len(probes)
    lim_index = {}
    for i, x in enumerate(entities):
        node_of[id(x)] = first + i
        if isinstance(x, Server):
            for part in (x._queue, x._driver, x._worker):
                node_of[id(part)] = first + i
        if isinstance(x, RateLimitedEntity):
            lim_index[id(x)] = len(lim_index)
    by_name = {x.name: node_of[id(x)] for x in entities + c.sources + probes}
    cb_probe = {id(p._event_provider.data_sink): len(c.sources) + j for j, p in enumerate(probes)}
    c.by_kind = by_kind = np.zeros(N_KINDS[family], np.int64)
    c.lim_events = np.zeros((len(lim_index), 2), np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop
    state = dict(cur=sim._start_time, cancelled=0, probe=None)

    def settle_probe():
        # the Event handled since the last pop was a checker's probe at a live Server: did its queue refuse it?
        if state["probe"] is not None:
            srv, before = state["probe"]
            c.probe_drops += int(srv.stats_dropped > before)
            state["probe"] = None

    def pop():
        settle_probe()
        e = orig_pop()
        if by_kind.sum() >= MAX_EVENTS:
            # FixedWindowPolicy.time_until_available answers Duration.ZERO when `remaining <= 0`; where the float floor division puts a
            # window's last nanosecond + 1 into the OLD window (0.3 // 0.1 == 2.0), the poll at that boundary finds the window still
            # full and is rescheduled for the same nanosecond for ever.  The reference never returns from such a run: not recordable.
            raise Livelock(spec["name"])
        if e.cancelled:                                   # skipped, counted in events_cancelled (core/simulation.py:475-477)
            state["cancelled"] += 1
            return e
        if e.time < state["cur"]:                         # time travel: skipped, not counted (:480-489)
            c.skipped += 1
            return e
        state["cur"] = e.time
        k, nd = classify(e, node_of, by_name)
        live = not getattr(e.target, "_crashed", False)   # (an Event at a crashed target is popped and counted, but its handler never runs: core/event.py:261)
        if isinstance(e.target, RateLimitedEntity) and live:
            c.lim_events[lim_index[id(e.target)], k - EV["lim_request"]] += 1
        if k == EV["probe"]:
            fn = e.target._fn if hasattr(e.target, "_fn") else e.target.fn
            cells = {id(cell.cell_contents) for cell in (fn.__closure__ or ())}
            nd = next(node for key, node in cb_probe.items() if key in cells)
        by_kind[k] += 1
        if e.event_type == "health_check" and isinstance(e.target, Server) and live:
            state["probe"] = (e.target, e.target.stats_dropped)
        if want_trace:
            trace.append((e.time.nanoseconds, k, nd, e._sort_index))
        return e

    heap.pop = pop
    GF.schedule_all(spec, c.pools, sim, Event, lambda t_s: MG._at(spec, t_s), early)
    c.summary = MG.run_sim_windows(sim, spec)
    settle_probe()
    out = dict(total_events=int(c.summary.total_events_processed), final_ns=int(sim._current_time.nanoseconds), by_kind=by_kind)
    assert int(by_kind.sum()) == out["total_events"], (spec["name"], int(by_kind.sum()), out["total_events"])
    assert state["cancelled"] == int(sim._events_cancelled)
    if "time_travel" not in SECTIONS[family]:
        assert state["cancelled"] == c.skipped == 0, "every popped event was processed (no time travel, nothing cancelled)"
    out["pending_events"] = int(heap.size())
    for name in SECTIONS[family]:
        out.update(_SECTION[name](c))
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out
