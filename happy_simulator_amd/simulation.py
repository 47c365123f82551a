"""`Simulation` -- host-side mirror of happysimulator/core/simulation.py:66-288 whose `run()` executes on the
MI355X engine instead of the Python heap loop.  Same constructor, same `SimulationSummary`."""
from __future__ import annotations

import time as _time

import warnings

import numpy as np

from . import _native as N
from .core.event import Event
from .core.temporal import Instant
from .engine import StationEngine
from .graph_engine import (DEFAULT_MAX_EVENTS, MAX_PARTS, GeneralGraph, GraphEngine, PartRun, keyless_hazard, lower_general, split_parts,
                           write_back_general)
from .entities import CanaryDeployer, RollingDeployer, AutoScaler, BatchProcessor, Bulkhead, Client, ConveyorBelt, Entity, Fallback, GateController, HealthChecker, Hedge, InventoryBuffer, LoadBalancer, Network, PooledCycleResource, Server, TimeoutWrapper
from .faults import FaultSchedule, LinkFaultEvent
from .lowering import (LazyRecords, LbGraph, LoweredGraph, UnsupportedTopology, attach_lb_probes, attach_probes, find_load_balancer, lower,
                       plain_probe_arrays, write_back_plain_probes,
                       lower_lb, write_back, write_back_lb, write_back_plain, write_back_probes, write_back_shared_sink_probes)
from .lowering import _plain_chains as plain_chains
from .summary import EntitySummary, LazyEntities, QueueStats, SimulationSummary

_DEFAULT_SEED = 42


LAZY_PROBES_MIN = 256      # plain-chain runs with more Probes than this leave the samples on the device until a Data is read


# Entity families only the single-heap loop follows, in the order their refusals win: (classes, whether a Source's target counts
# next to the listed entities, the station engines' refusal).  Backends that join and leave, completion hooks and per-request ids,
# retries, stations that hold Requests back and release them together.
_NOT_ON_STATIONS = "the station, network and pipeline engines do not lower "
_SINGLE_HEAP_ONLY = (
    ((PooledCycleResource, InventoryBuffer), True, _NOT_ON_STATIONS + "PooledCycleResource or InventoryBuffer"),
    ((Hedge, Fallback), True, _NOT_ON_STATIONS + "Hedge or Fallback"),
    ((RollingDeployer, CanaryDeployer), False, _NOT_ON_STATIONS + "a RollingDeployer or a CanaryDeployer"),
    (AutoScaler, False, _NOT_ON_STATIONS + "an AutoScaler"),
    ((BatchProcessor, ConveyorBelt, GateController), True, _NOT_ON_STATIONS + "BatchProcessor, ConveyorBelt or GateController"),
    (Client, True, _NOT_ON_STATIONS + "a Client"),
    ((Bulkhead, TimeoutWrapper), True, _NOT_ON_STATIONS + "Bulkhead or TimeoutWrapper"),
)

# The internal Event kinds of the families (events_processed counts them, events_by_kind does not), like the limiters' and the
# faults': (GraphArrays flags of which one is set, the Simulation's attribute, the engine's reader of the counts by kind).
_BY_KIND = (
    (("has_health",), "_health_by_kind", "health_events"),                   # the checkers' cycle / response / timeout Events
    (("has_wrappers",), "_resilience_by_kind", "wrapper_events"),            # Bulkhead and TimeoutWrapper request / response / timeout
    (("has_clients",), "_client_by_kind", "client_events"),                  # the Clients' request / response / timeout Events
    (("has_scalers",), "_autoscaler_by_kind", "scaler_events"),              # the one `_autoscaler_evaluate` kind
    (("has_deployers", "has_canaries"), "_deployer_by_kind", "deployer_events"),   # the deployers' seven kinds
    (("has_deployers", "has_canaries"), "_canary_by_kind", "canary_events"),
    (("has_hedges",), "_hedge_by_kind", "hedge_events"),                     # Hedge request / response / send-hedge, Fallback's four
    (("has_stock",), "_stock_by_kind", "stock_events"),                      # a pool's Request / cycle end, a buffer's consume / replenish
)


def seed(value: int) -> None:
    """Default Philox key for Simulations created afterwards (the reference's idiom is `random.seed(42)`)."""
    global _DEFAULT_SEED
    _DEFAULT_SEED = int(value)


class Simulation:
    def __init__(self, start_time: Instant | None = None, end_time: Instant | None = None, sources=None,
                 entities=None, probes=None, trace_recorder=None, fault_schedule=None, duration: float | None = None,
                 *, seed: int | None = None, device: int = 0, log_capacity: int | None = None,
                 bag_capacity: int | None = None, msg_capacity: int | None = None, max_graph_events: int | None = None):
        if duration is not None and end_time is not None:
            raise ValueError("Cannot specify both 'duration' and 'end_time'")        # core/simulation.py:79-80
        self._start_time = start_time if start_time is not None else Instant.Epoch
        if duration is not None:
            self._end_time = self._start_time + duration
        elif end_time is not None:
            self._end_time = end_time
        else:
            self._end_time = Instant.Infinity
        self._sources = list(sources or [])
        self._entities = list(entities or [])
        self._probes = list(probes or [])
        if trace_recorder is not None:
            raise UnsupportedTopology("trace recorders force the reference's slow loop; profile with rocprofv3 instead")
        # FaultSchedule.start (core/simulation.py:162-169): the fault Events come into being HERE, behind the Sources' and the
        # Probes' first Events -- names resolve now (KeyError), a handle cancelled from now on cancels them
        self._fault_schedule = fault_schedule
        if fault_schedule is not None and not isinstance(fault_schedule, FaultSchedule):
            raise UnsupportedTopology(f"fault schedule {type(fault_schedule).__name__} is not a lowered FaultSchedule")
        self._faults = fault_schedule._start(self) if fault_schedule is not None else []
        for ent in self._entities:                 # the clock every listed entity is handed (core/simulation.py:118-135): a
            if isinstance(ent, (HealthChecker, AutoScaler, RollingDeployer, CanaryDeployer)):     # checker's (a scaler's) start(), a deployer's deploy() read `now` from it
                ent._sim_start = self._start_time
            if isinstance(ent, Client):            # ... and a Client's send_request()
                ent._sim = self
        self._seed = _DEFAULT_SEED if seed is None else int(seed)
        self._device = device
        # engine capacities (records per station log / in-flight messages per station / messages per exchange row); None =
        # derived from the rates.  An HS_E_OVERFLOW names the one to raise.
        self._log_capacity, self._bag_capacity, self._msg_capacity = log_capacity, bag_capacity, msg_capacity
        # a graph outside the station shape runs on the single-heap loop (graph_engine.py): events it may cost before it is refused
        self._max_graph_events = DEFAULT_MAX_EVENTS if max_graph_events is None else int(max_graph_events)
        self._summary: SimulationSummary | None = None
        self._graph: LoweredGraph | None = None
        self._events_processed = 0
        self._events_cancelled = 0
        self._current_time = self._start_time
        self._engine_summary = None
        self._scheduled: list[Event] = []

    def schedule(self, events) -> None:
        """Inject Events from outside the event loop, before run() (core/simulation.py:195-206).  Lowered: Requests for a
        Server of this Simulation; they enter the Server's queue at their time like a Source's payload would, with
        context["created_at"] = their own time.  An Event built before run() precedes run-time events of the same ns."""
        if self._summary is not None:
            raise UnsupportedTopology("schedule() after run(): the engine run is over (build a new Simulation)")
        for ev in (events if isinstance(events, list) else [events]):
            if not isinstance(ev, Event):
                raise TypeError(f"schedule() takes Event objects, got {type(ev).__name__}")
            self._scheduled.append(ev)

    def _schedule_arrays(self, g: LoweredGraph, arrays) -> list[int]:
        """Scheduled Events -> per-station ascending time lists (stable in call order).  Returns the times of the
        cancelled ones."""
        if not self._scheduled:
            return []
        station_of = {id(st.server): i for i, st in enumerate(g.stations) if st.server is not None}
        per: list[list[tuple[int, int]]] = [[] for _ in g.stations]
        cancelled: list[int] = []
        start_ns = self._start_time.nanoseconds
        for rank, ev in enumerate(self._scheduled):     # rank: the Event's position among everything the caller constructed
            if ev.cancelled:                       # lazy deletion: skipped when popped, counted (simulation.py:475-477)
                cancelled.append(ev.time.nanoseconds)
                continue
            i = station_of.get(id(ev.target))
            if i is None:
                raise UnsupportedTopology(
                    f"scheduled event {ev!r}: only Requests for a Server of this Simulation are lowered")
            if ev.on_complete:
                raise UnsupportedTopology(f"scheduled event {ev!r}: completion hooks are host Python (not lowered)")
            if ev.context.get("created_at") != ev.time:
                raise UnsupportedTopology(f"scheduled event {ev!r}: a custom created_at is not lowered")
            if ev.time.nanoseconds < start_ns:     # "time travel": the loop skips it without counting (simulation.py:480-489)
                warnings.warn(f"Time travel detected: {ev!r} lies before the simulation start; skipping event", stacklevel=3)
                continue
            per[i].append((ev.time.nanoseconds, rank))
        # Same-nanosecond order against run-time events is the reference's: the engine replays the first constructions of
        # the run in exact heap order (csrc/hs_exact.hpp) from the construction ranks handed over here.
        off = np.zeros(len(g.stations) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in per])
        flat = [tr for p in per for tr in sorted(p)]                         # ascending time, ties in construction order
        arrays.sched_off = off
        arrays.sched_time_ns = np.array([t for t, _ in flat], np.int64)
        arrays.sched_rank = np.array([r for _, r in flat], np.int64)
        return cancelled

    @property
    def summary(self) -> SimulationSummary | None:
        return self._summary

    def _has_health(self) -> bool:
        """A HealthChecker among the entities, or a LoadBalancer with a backend marked unhealthy: the backend list changes (or is
        not the full one), which only the single-heap loop follows."""
        return any(isinstance(e, HealthChecker) or (isinstance(e, LoadBalancer) and e.unhealthy_backends) for e in self._entities)

    def _scaler_starts(self) -> int:
        """The most `_autoscaler_evaluate` Events scheduled for one scaler: every one begins a chain of evaluations."""
        per: dict[int, int] = {}
        for ev in self._scheduled:
            if isinstance(ev.target, AutoScaler) and not ev.cancelled:
                per[id(ev.target)] = per.get(id(ev.target), 0) + 1
        return max(per.values(), default=1)

    def _deploys(self) -> dict:
        """id(deployer) -> its scheduled deploy() Events: what its instance pool is sized by."""
        per: dict[int, int] = {}
        for ev in self._scheduled:
            if isinstance(ev.target, (RollingDeployer, CanaryDeployer)) and not ev.cancelled:
                per[id(ev.target)] = per.get(id(ev.target), 0) + 1
        return per

    def _lower_general(self) -> GeneralGraph:
        """lower_general over this Simulation, with the horizon and the scheduled start() Events its AutoScalers' pools are sized by."""
        end_ns = None if self._end_time == Instant.Infinity else self._end_time.nanoseconds
        return lower_general(self._sources, self._entities, self._probes, start_ns=self._start_time.nanoseconds, end_ns=end_ns,
                             scaler_starts=self._scaler_starts(), deploys=self._deploys())

    def _single_heap_only(self) -> str | None:
        """What of this Simulation only the single-heap loop follows, as the station engines' refusal of it (None: nothing)."""
        firsts = [getattr(getattr(s, "_event_provider", None), "_target", None) for s in self._sources]
        for classes, aimed_at, refusal in _SINGLE_HEAP_ONLY:
            if any(isinstance(e, classes) for e in (self._entities + firsts if aimed_at else self._entities)):
                return refusal
        if self._faults:                               # (node faults run where every Event is popped one by one)
            return _NOT_ON_STATIONS + "fault schedules"
        return _NOT_ON_STATIONS + "health checks or unhealthy backends" if self._has_health() else None

    def lowered(self) -> "LoweredGraph | LbGraph | GeneralGraph":
        if self._graph is None:
            refusal = self._single_heap_only()
            if refusal is not None:
                self._graph = self._lower_general()
                self._station_refusal = refusal
        if self._graph is None:
            plain = plain_chains(self._sources, self._entities)      # (n plain chains: no LoadBalancer among them, one pass less)
            if plain is not None:
                self._graph = LoweredGraph(plain)
                lb = None
            else:
                lb = None
                try:
                    lb = find_load_balancer(self._sources, self._entities)
                    self._graph = lower_lb(self._sources, self._entities, lb) if lb is not None else lower(self._sources,
                                                                                                            self._entities)
                except UnsupportedTopology as station_shape:
                    # not the shape the station engines take: the single-heap loop (csrc/hs_graph.hip) runs what the same entity
                    # classes can be wired into otherwise -- exactly, at ~2.4 us per event and heap (several LoadBalancers, a LoadBalancer
                    # behind Servers ... included)
                    try:
                        self._graph = self._lower_general()
                    except UnsupportedTopology as general:
                        raise UnsupportedTopology(f"{station_shape}; and not on the single-heap path either: {general}") from None
                    self._station_refusal = str(station_shape)
                    return self._graph
            if self._probes:
                try:
                    if lb is not None:
                        attach_lb_probes(self._graph, self._probes)
                    elif plain is not None and not self._scheduled:
                        self._plain_probes_pending = True     # (_run puts them into the arrays without a Station per chain)
                    else:
                        attach_probes(self._graph, self._probes)
                except UnsupportedTopology as station_shape:
                    # (more than four probes on a station, a further Source of a Server sampled, a probe on the LoadBalancer's
                    # Source with stop_after ...: the single heap samples anything)
                    try:
                        self._graph = self._lower_general()
                    except UnsupportedTopology:
                        raise station_shape from None
                    self._station_refusal = str(station_shape)
        return self._graph

    def _run_lb(self, g: LbGraph, wall0: float) -> SimulationSummary:
        """Sources -> LoadBalancer(ConsistentHash) -> Servers -> Sink(s): the pipeline engine (csrc/hs_lb.hip)."""
        from .lb_engine import LoadBalancerEngine

        end_ns = self._end_time.nanoseconds
        src, be = g.engine_arrays()
        from .entities import ConsistentHash, IPHash, RoundRobin, WeightedRoundRobin

        strat = g.lb.strategy
        code = (N.LB_CONSISTENT_HASH if isinstance(strat, ConsistentHash) else N.LB_ROUND_ROBIN if isinstance(strat, RoundRobin)
                else N.LB_IP_HASH if isinstance(strat, IPHash) else N.LB_WEIGHTED_ROUND_ROBIN if isinstance(strat, WeightedRoundRobin)
                else N.LB_RANDOM)
        with LoadBalancerEngine(src, be, virtual_nodes=getattr(strat, "virtual_nodes", 1), horizon_ns=end_ns,
                                shared_sink=g.shared_sink, start_ns=self._start_time.nanoseconds, seed=self._seed,
                                device=self._device, strategy=code) as eng:
            if g.probes:
                eng.set_probes(*g.probe_arrays())
            if isinstance(strat, WeightedRoundRobin):
                eng.set_weights([strat.get_weight(b) for b in g.backends])
            eng.run(end_ns)
            es = eng.summary()
            write_back_lb(g, eng.stats(), eng)
        return self._finish(es, _time.monotonic() - wall0)

    def __del__(self):
        try:                       # results this run has not bound to its entities yet (entities._PENDING) outlive the Simulation
            from .entities import _flush_pending
            _flush_pending()
        except Exception:          # noqa: BLE001 -- interpreter shutdown
            pass

    def run(self) -> SimulationSummary:
        auto = self._end_time == Instant.Infinity
        if auto:
            # Auto-termination (core/simulation.py:311-322): the loop ends when no PRIMARY event is pending
            # (core/event_heap.py:102-104).  A Source's ticks are primary and never stop -- with any Source the reference
            # itself never returns -- so the lowered case is a Simulation driven by schedule()d Requests only: it ends with
            # the last completion, nothing beyond it is processed.  (Probe ticks are daemon events: where the run stops
            # relative to them is decided pop by pop -- not lowered.)
            if self._sources:
                raise UnsupportedTopology("end_time = Infinity with Sources never terminates (their ticks are primary events, in "
                                          "the reference too); pass end_time/duration")
            if any(isinstance(e, HealthChecker) and e.is_running for e in self._entities):
                # the cycle Event is no daemon (health_check.py:266-271): a running checker keeps the primary count above zero for ever
                raise UnsupportedTopology("end_time = Infinity with a running HealthChecker never terminates (its cycle Events are primary "
                                          "events, in the reference too); pass end_time/duration")
            if self._probes:
                # a Probe IS a Source (instrumentation/probe.py:81): its ticks are SourceEvents built with daemon=False
                # (load/source.py:136,171; load/source_event.py:27) -- only the probe_event samples are daemons -- so they keep
                # the primary count above zero for ever, exactly like a Source's
                raise UnsupportedTopology("end_time = Infinity with Probes never terminates either (a Probe's ticks are primary events: "
                                          "only its probe_event samples are daemons, load/source_event.py:27); pass end_time/duration")
        if self._start_time.nanoseconds < 0:
            # the reference accepts it; every engine keeps its Sinks' records and its links' packed bounds as non-negative times
            raise UnsupportedTopology(f"start_time {self._start_time!r} is negative: not lowered (the engines refuse it too)")
        wall0 = _time.monotonic()
        import gc

        gc_was = gc.isenabled()
        gc.disable()        # lowering and write-back touch every entity once: generational collections over 10^5 live objects cost more than the run
        try:
            return self._run(auto, wall0)
        finally:
            if gc_was:
                gc.enable()

    def _run(self, auto: bool, wall0: float) -> SimulationSummary:
        g = self.lowered()
        if not isinstance(g, GeneralGraph):
            try:
                return self._run_station(g, auto, wall0)
            except UnsupportedTopology as station_shape:
                # refused on the way (a probe the station slots do not hold, a tick on the nanosecond of a shared Sink's record ...):
                # the single-heap loop takes it if the graph is its kind; otherwise the station engines' refusal stands
                try:
                    g = self._lower_general()
                except UnsupportedTopology:
                    raise station_shape from None
                self._station_refusal = str(station_shape)
                self._graph = g
        try:
            return self._run_general(g, auto, wall0)
        except UnsupportedTopology as general:
            raise UnsupportedTopology(f"{self._station_refusal}; and not on the single-heap path either: {general}") from None

    def _run_station(self, g, auto: bool, wall0: float) -> SimulationSummary:
        if isinstance(g, LbGraph):
            if self._scheduled:
                raise UnsupportedTopology("schedule() is not lowered for load-balancer topologies yet")
            return self._run_lb(g, wall0)
        if auto and g.is_network:
            # the network engines run to a horizon; the single-heap loop ends with its heap, as the reference's does
            # (core/simulation.py:304-322: no Sources here, so every pending event is primary and the run drains)
            raise UnsupportedTopology("auto-terminating runs of station networks are not lowered on the network engines")
        # auto-termination: a horizon nothing reaches (the station kernel stops when no event is pending)
        end_ns = self._end_time.nanoseconds if not auto else (1 << 61)
        net = g.network_arrays(self._bag_capacity or 0) if g.is_network else None
        horizon_s = (end_ns - self._start_time.nanoseconds) / 1e9
        arrays = g.arrays()
        if getattr(self, "_plain_probes_pending", False):
            self._plain_probes_pending = False
            fast = not self._scheduled and g.plain is not None and g._stations is None      # (`arrays` is PlainChains.arrays)
            where = plain_probe_arrays(g.plain, self._probes, arrays) if fast else None
            if where is not None:
                return self._run_plain(g, arrays, end_ns, wall0, where)
            attach_probes(g, self._probes)                # (a probe the fast path does not cover: Station objects after all)
            arrays = g.arrays()
        elif g.plain is not None and not self._probes and not self._scheduled:
            return self._run_plain(g, arrays, end_ns, wall0)
        # the order in which Simulation.__init__ constructs the first SourceEvents / probe ticks (core/simulation.py:145-160)
        st_of = {id(st.source): (i, 0) for i, st in enumerate(g.stations) if st.source is not None}
        st_of.update({id(x): (i, 1 + k) for i, st in enumerate(g.stations) for k, x in enumerate(st.more_sources)})
        arrays.source_order = np.array([st_of[id(s)][0] for s in self._sources], np.int32)
        if any(st.more_sources for st in g.stations):
            arrays.source_slot_order = np.array([st_of[id(s)][1] for s in self._sources], np.uint8)
        if self._probes:
            where = {id(pr): (i, slot) for i, st in enumerate(g.stations) for slot, pr in enumerate(st.probes)}
            arrays.probe_order = np.array([where[id(p)][0] for p in self._probes], np.int32)
            arrays.probe_slot_order = np.array([where[id(p)][1] for p in self._probes], np.uint8)
        cancelled_ns = self._schedule_arrays(g, arrays)
        if net is not None and arrays.n > self._resident_stations():
            return self._run_time_shared(g, arrays, net, end_ns, horizon_s, wall0, cancelled_ns)
        with StationEngine(arrays, mode=N.MODE_SINGLE, horizon_ns=end_ns, start_ns=self._start_time.nanoseconds,
                           seed=self._seed, device=self._device, network=net,
                           log_capacity=self._log_cap(g, horizon_s, arrays, net is not None)) as eng:
            eng.run_until(end_ns)
            es = eng.summary()
            stats = eng.lp_stats()
            if arrays.src_more_kind is not None:
                stats["generated_more"] = [eng.source_generated(1 + k) for k in range(3)]
            counts, t_ns, created_ns = eng.read_sinks()
            net_stats = eng.net_stats() if net is not None else None
            if self._probes:
                write_back_probes(g, eng)
        write_back(g, stats, counts, t_ns, created_ns, net_stats, device=self._device)
        write_back_shared_sink_probes(g)
        # a cancelled event is counted when the loop pops it: everything up to the last processed event, or the whole
        # heap when the run ended with nothing left beyond end_time (core/simulation.py:472-477)
        drained = es.final_time_ns <= end_ns
        self._events_cancelled = sum(1 for t in cancelled_ns if drained or t <= es.final_time_ns)
        return self._finish(es, _time.monotonic() - wall0)

    def _run_general(self, g: GeneralGraph, auto: bool, wall0: float) -> SimulationSummary:
        """A graph outside the station shape (graph_lowering.lower_general) on the device's single-heap loop."""
        end_ns, start_ns, sched, cancelled_ns = self._general_prepare(g, auto)
        # (one component per heap while there are at most MAX_PARTS: components that SHARE a heap are checked as one -- two Probes of one
        #  interval, two constant Sources of one rate in different components then look like a mixed timestamp group: undecided)
        # an auto-terminating run with limiters ends when no PRIMARY event is pending anywhere (their polls are daemons,
        # core/simulation.py:311-322): a part cannot know that of the others, so such a run stays on one heap
        daemons = auto and bool((g.arrays.kind == N.NODE_RATE_LIMITER).any() or self._faults or any(len(e) > 3 for e in sched))   # (... or gate Events)
        faults = self._general_faults(g)
        # (a cancelled fault Event stays in its heap, as in the reference's: it is no candidate for the one Event beyond the end)
        parts = None if cancelled_ns or daemons or any(f[3] for f in faults) else split_parts(g.arrays, MAX_PARTS)
        try:
            self._refuse_long_run(1 if parts is None else len(parts))
        except UnsupportedTopology:
            if parts is None:
                raise
            parts = None                                           # (uneven parts: the one heap's own estimate decides)
            self._refuse_long_run(1)
        if parts is not None:
            # the graph falls into parts no Request can cross: one heap each, side by side (hs_graph_run_parts) -- exact unless a
            # timestamp group turns out to be ordered by ALL of the Simulation's events; then the one heap below decides
            part_of = np.empty(g.arrays.n, np.int64)
            local = np.empty(g.arrays.n, np.int64)
            for p, (ids, _pos, _b) in enumerate(parts):
                part_of[ids] = p
                local[ids] = np.arange(len(ids))
            engines = []
            try:
                for p, (ids, _pos, b) in enumerate(parts):
                    engines.append(GraphEngine(b, seed=self._seed, start_ns=start_ns, device=self._device, max_events=self._max_graph_events,
                                               record_capacity=4096))
                for node, *rest in faults:                         # (a fault Event lives in the part of the entity or link it names)
                    engines[int(part_of[node])].add_faults([(int(local[node]), *rest)])
                for node, t, *rid in sched:                        # (call order: each part keeps the order of its own)
                    engines[int(part_of[node])].schedule(int(local[node]), t, *rid)
                run = PartRun(g.arrays, parts, engines)
                if run.run(end_ns):
                    self._graph_parts = len(parts)
                    return self._general_finish(g, run, end_ns, cancelled_ns, _time.monotonic() - wall0)
            finally:
                for e in engines:
                    e.close()
        self._graph_parts = 1
        self._refuse_long_run(1)
        with self._general_engine(g, start_ns, sched) as eng:
            eng.run_until(end_ns)
            return self._general_finish(g, eng, end_ns, cancelled_ns, _time.monotonic() - wall0)

    def _refuse_long_run(self, heaps: int = 1) -> None:
        """(after _general_prepare) refuse up front what would keep one lane busy for minutes; `heaps`: the heaps the run is spread over."""
        est = self._general_est / max(heaps, 1)
        if self._max_graph_events > 0 and est > 4.0 * self._max_graph_events:
            raise UnsupportedTopology(
                f"the single-heap path (one lane, ~2 us per event) would need ~{est:.2g} events per heap for this run "
                f"(limit {self._max_graph_events}: Simulation(max_graph_events=...))")

    def _general_prepare(self, g: GeneralGraph, auto: bool):
        """What the single-heap engine is created with: (end ns, start ns, the schedule()d Requests as (node, ns), the cancelled
        Events' times) -- or the refusal of a run it does not take."""
        end_ns = self._end_time.nanoseconds if not auto else (1 << 61)
        start_ns = self._start_time.nanoseconds
        a = g.arrays
        if auto and any(isinstance(e, HealthChecker) and e.is_running for e in g.nodes):
            raise UnsupportedTopology("end_time = Infinity with a running HealthChecker never terminates (its cycle Events are primary "
                                      "events, in the reference too); pass end_time/duration")
        # ~8 reference events per Request that is served and ~2 per hop: refuse up front what would take the one lane minutes
        horizon_s = 0.0 if auto else (end_ns - start_ns) / 1e9
        self._general_est = 12.0 * float(a.src_rate[a.kind == N.NODE_SOURCE].sum()) * horizon_s
        cancelled_ns: list[int] = []
        sched: list[tuple[int, int]] = []
        n_starts: dict[int, int] = {}
        for ev in self._scheduled:
            if ev.cancelled:                       # lazy deletion: skipped when popped, counted (simulation.py:475-477)
                cancelled_ns.append(ev.time.nanoseconds)
                continue
            i = g.node_of.get(id(ev.target))
            if isinstance(ev.target, Network):
                raise UnsupportedTopology(f"scheduled event {ev!r}: an Event aimed at the Network '{ev.target.name}' is not lowered (a Network "
                                          "is a registry of links here: send to the link itself)")
            if i is not None and a.kind[i] == N.NODE_HEALTH_CHECKER and ev.event_type != "_health_check_cycle":
                raise UnsupportedTopology(f"scheduled event {ev!r}: only the Event start() returns is lowered for a HealthChecker")
            if i is None or a.kind[i] == N.NODE_SOURCE:
                raise UnsupportedTopology(f"scheduled event {ev!r}: only Requests for a Server / Sink / NetworkLink / RandomRouter / "
                                          "RateLimitedEntity of this Simulation are lowered")
            if ev.on_complete:
                raise UnsupportedTopology(f"scheduled event {ev!r}: completion hooks are host Python (not lowered)")
            if a.has_stock and (ev.event_type == "_InventoryReplenish" or "quantity" in ev.context):
                # (an event_type and a context travel on with the Event: either may reach a buffer from anywhere)
                raise UnsupportedTopology(f"scheduled event {ev!r}: a hand-made '_InventoryReplenish' Event and a 'quantity' in an Event's "
                                          "context are not lowered next to an InventoryBuffer (a consume takes one item)")
            rid = None
            if a.kind[i] == N.NODE_AUTO_SCALER:
                # the Event AutoScaler.start() returns: a daemon without a Request, at the Simulation's start
                if ev.event_type != "_autoscaler_evaluate" or not ev.daemon or ev.time.nanoseconds != start_ns:
                    raise UnsupportedTopology(f"scheduled event {ev!r}: only the daemon Event start() returns, at the Simulation's start, is "
                                              "lowered for an AutoScaler")
                if cancelled_ns:
                    raise UnsupportedTopology("cancelled Events in front of live ones are not lowered on the single-heap path")
                n_starts[i] = n_starts.get(i, 0) + 1
                if n_starts[i] > g.scaler_starts:
                    raise UnsupportedTopology(f"scheduled event {ev!r}: start() Events scheduled after the graph was lowered (the scaler's "
                                              "instance pool was sized for fewer): schedule them before lowered()")
                sched.append((i, ev.time.nanoseconds))
                continue
            if a.kind[i] in (N.NODE_ROLLING_DEPLOYER, N.NODE_CANARY_DEPLOYER):
                # the Event deploy() returns: no daemon, no Request, at any time the caller set
                rolling = a.kind[i] == N.NODE_ROLLING_DEPLOYER
                if ev.event_type != ("_rolling_deploy_start" if rolling else "_canary_deploy_start") or ev.daemon:
                    raise UnsupportedTopology(f"scheduled event {ev!r}: only the Event deploy() returns is lowered for a "
                                              f"{'RollingDeployer' if rolling else 'CanaryDeployer'}")
                if cancelled_ns:
                    raise UnsupportedTopology("cancelled Events in front of live ones are not lowered on the single-heap path")
                n_starts[i] = n_starts.get(i, 0) + 1
                if n_starts[i] > g.deploys.get(i, 0):
                    raise UnsupportedTopology(f"scheduled event {ev!r}: deploy() Events scheduled after the graph was lowered (the deployer's "
                                              "instance pool was sized for fewer): schedule them before lowered()")
                sched.append((i, ev.time.nanoseconds))
                continue
            if a.kind[i] == N.NODE_GATE and ev.event_type in ("_GateOpen", "_GateClose"):
                # one Event of GateController.start_events(): a daemon without a Request
                if not ev.daemon:
                    raise UnsupportedTopology(f"scheduled event {ev!r}: only the daemon Events start_events() returns are lowered for a "
                                              "GateController")
                if cancelled_ns:
                    raise UnsupportedTopology("cancelled Events in front of live ones are not lowered on the single-heap path")
                if ev.time.nanoseconds < start_ns:
                    warnings.warn(f"Time travel detected: {ev!r} lies before the simulation start; skipping event", stacklevel=3)
                    continue
                sched.append((i, ev.time.nanoseconds, None, ev.event_type == "_GateOpen"))
                continue
            if a.kind[i] == N.NODE_BATCH_PROCESSOR and ev.event_type == "_BatchTimeout":
                raise UnsupportedTopology(f"scheduled event {ev!r}: a BatchProcessor's own '_BatchTimeout' Event is not lowered")
            if a.kind[i] == N.NODE_CLIENT:
                # Client.send_request's Event or a plain one: the Client reads metadata request_id / attempt and never passes
                # created_at on (client.py:233-282)
                md = ev.context.get("metadata") or {}
                if ev.event_type in ("_client_timeout", "_client_response"):
                    raise UnsupportedTopology(f"scheduled event {ev!r}: a Client's own '{ev.event_type}' Event is not lowered")
                if ev.context.get("_on_success") is not None or ev.context.get("_on_failure") is not None:
                    raise UnsupportedTopology(f"scheduled event {ev!r}: on_success= / on_failure= are host callables (not lowered)")
                if md.get("attempt", 1) != 1 or isinstance(md.get("attempt", 1), bool):
                    raise UnsupportedTopology(f"scheduled event {ev!r}: attempt = {md.get('attempt')!r} is not lowered (a scheduled request is "
                                              "attempt 1)")
                rid = md.get("request_id")
                if rid is not None and (type(rid) is not int or not 0 < rid < Client.MAX_REQUEST_ID):
                    raise UnsupportedTopology(f"scheduled event {ev!r}: request_id = {rid!r} is not lowered (None or a positive int below "
                                              "2^30)")
                rid = 0 if rid is None else rid
            elif ev.context.get("created_at") != ev.time:
                raise UnsupportedTopology(f"scheduled event {ev!r}: a custom created_at is not lowered")
            lb_name = None if a.kind[i] == N.NODE_HEALTH_CHECKER else keyless_hazard(g, ev.target)
            if lb_name is not None:
                raise UnsupportedTopology(f"scheduled event {ev!r} carries no client id and can reach the Random LoadBalancer "
                                          f"'{lb_name}' (the reference would ask the process-wide random generator): not lowered")
            if cancelled_ns:
                # a cancelled Event keeps its place in the process-wide counter: the ones behind it would need the gap
                raise UnsupportedTopology("cancelled Events in front of live ones are not lowered on the single-heap path")
            if ev.time.nanoseconds < start_ns:     # "time travel": the loop skips it without counting (simulation.py:480-489)
                warnings.warn(f"Time travel detected: {ev!r} lies before the simulation start; skipping event", stacklevel=3)
                continue
            sched.append((i, ev.time.nanoseconds) if rid is None else (i, ev.time.nanoseconds, rid))
        return end_ns, start_ns, sched, cancelled_ns

    def _general_engine(self, g: GeneralGraph, start_ns: int, sched, record_capacity: int = 0) -> GraphEngine:
        eng = GraphEngine(g.arrays, seed=self._seed, start_ns=start_ns, device=self._device, max_events=self._max_graph_events,
                          record_capacity=record_capacity)
        try:
            eng.add_faults(self._general_faults(g))
            for node, t, *rid in sched:
                eng.schedule(node, t, *rid)
        except BaseException:
            eng.close()
            raise
        return eng

    def _general_faults(self, g: GeneralGraph) -> list[tuple]:
        """The fault Events as (node, ns, on, cancelled by now) -- a link fault's: (link node, ns, on, cancelled by now, its
        LinkFaultEvent) --, in the order Simulation.__init__ constructed them."""
        out = []
        for f in self._faults:
            if isinstance(f, LinkFaultEvent):
                node = g.node_of.get(id(f.link))
                if node is None:
                    raise UnsupportedTopology(f"link '{f.link.name}' is named by a link fault but is no entity of this Simulation: nothing "
                                              "sends to it and `entities` does not list it (not lowered)")
                out.append((node, f.event.time.nanoseconds, f.on, f.event.cancelled, f))
            else:
                ent, ev, on = f
                out.append((g.node_of[id(ent)], ev.time.nanoseconds, on, ev.cancelled))
        return out

    def _general_finish(self, g: GeneralGraph, eng: GraphEngine, end_ns: int, cancelled_ns, wall_s: float) -> SimulationSummary:
        """The run's results off the engine onto the user's objects (the engine may have run alone or in a batch)."""
        es = eng.summary()
        stats = eng.stats()
        rec = eng.records()
        a = g.arrays
        write_back_general(g, stats, *rec, device=self._device, engine=eng)
        drained = es.final_time_ns <= end_ns
        self._events_cancelled = sum(1 for t in cancelled_ns if drained or t <= es.final_time_ns)
        for flags, attr, reader in _BY_KIND:
            if any(getattr(a, f) for f in flags):
                setattr(self, attr, np.atleast_1d(getattr(eng, reader)()))       # (scaler_events is the one count itself)
        if a.has_flows:
            # the flow entities' eight kinds and, last, the `_BatchTimeout` Events popped after their batch had started: those were
            # cancelled (core/simulation.py:326-329)
            fe = eng.flow_events()
            self._flow_by_kind = fe[:N.FLOW_KINDS]
            self._events_cancelled += int(fe[N.FLOW_KINDS])
        if (a.has_health or a.has_wrappers or a.has_clients or a.has_flows or a.has_queue_policies or a.has_hedges or a.has_stock) and not self._faults:
            self._internal_by_kind = eng.faults()[1]
        if self._faults:
            crashed, internal, popped_cancelled = eng.faults()
            self._internal_by_kind = internal                      # (limiter Requests, limiter polls, fault set, fault clear)
            self._fault_events_processed = int(internal[2] + internal[3])
            self._events_cancelled += popped_cancelled
            for f in self._faults:                                 # the flag every named entity is left with (faults/node_faults.py:46-62)
                if not isinstance(f, LinkFaultEvent):
                    f[0]._crashed = bool(crashed[g.node_of[id(f[0])]])
            link_events = [f for f in self._faults if isinstance(f, LinkFaultEvent)]
            if link_events:
                # what the fault in force leaves on its link (faults/network_faults.py:83-100,159-176): the _CompoundLatency / the
                # raised rate of the activation that came last, or the original a deactivation put back
                state = eng.link_faults()
                self._link_fault_state = {}                        # id(link) -> the schedule's place of the latency / loss fault in force (-1: none)
                for f in link_events:
                    if f.on:
                        continue                                   # (every fault has a deactivation: it holds the original)
                    lat, loss, draws = state[g.node_of[id(f.link)]]
                    if f.what == "latency":
                        f.link.latency = f.leaves if lat is None else lat.leaves
                    else:
                        f.link.packet_loss_rate = f.leaves if loss is None else loss.leaves
                    f.link._loss_draws = draws
                    self._link_fault_state[id(f.link)] = (-1 if lat is None else lat.index, -1 if loss is None else loss.index)
        return self._finish(es, wall_s)

    def _run_plain(self, g: LoweredGraph, arrays, end_ns: int, wall0: float, probe_where=None) -> SimulationSummary:
        """n plain Source -> Server -> [Sink] chains (lowering.PlainChains): no per-station Python objects on the way in, Python
        lists instead of numpy scalars on the way out, and the Sink records stay on the device until a Sink's lists are first read
        (LazyRecords keeps the engine until then) -- at 65 536 chains run() used to spend 0.7 s around a 0.45 ms device run."""
        arrays.source_order = g.plain.source_station
        eng = StationEngine(arrays, mode=N.MODE_SINGLE, horizon_ns=end_ns, start_ns=self._start_time.nanoseconds, seed=self._seed,
                            device=self._device, log_capacity=int(self._log_capacity or 0))
        try:
            eng.run_until(end_ns)
            es = eng.summary()
            stats = eng.lp_stats()
        except Exception:
            eng.close()
            raise
        # a few probes: their samples come down now (microseconds each) and nothing pins the engine beyond the Sink records; many
        # (a Probe on every one of 65 536 Servers): they stay on the device until a Data is read, and every unread Data keeps the
        # engine alive through the LazyRecords it holds (a Data read after the Simulation was dropped found a closed engine)
        lazy_probes = bool(probe_where) and len(probe_where) > LAZY_PROBES_MIN
        records = LazyRecords(eng, stats["sink_received"], keep_engine=lazy_probes)
        self._records = records                 # (keeps the device buffers alive as long as the Simulation, or until fetched)
        write_back_plain(g.plain, stats, records, device=self._device)
        if probe_where:
            write_back_plain_probes(self._probes, probe_where, records, lazy=lazy_probes)
        self._events_cancelled = 0
        return self._finish(es, _time.monotonic() - wall0)

    def _log_cap(self, g, horizon_s: float, arrays, is_net: bool) -> int:
        if self._log_capacity:
            return int(self._log_capacity)
        if not is_net:
            return 0                           # the engine derives it from the rates (and the scheduled Requests)
        extra = int(np.diff(arrays.sched_off).max()) if arrays.sched_off is not None and len(arrays.sched_off) > 1 else 0
        return g.log_capacity(horizon_s, extra)

    def _resident_stations(self) -> int:
        """Stations one cooperative launch of the asynchronous network engine holds: one 256-lane workgroup per CU (its
        LDS rings and bags fill the CU)."""
        import torch

        return torch.cuda.get_device_properties(self._device).multi_processor_count * 256

    def _run_time_shared(self, g, arrays, net, end_ns: int, horizon_s: float, wall0: float, cancelled_ns=()) -> SimulationSummary:
        """A network with more stations than one cooperative launch holds: contiguous segments take turns on the device
        under the asynchronous-rounds protocol of the multi-GPU path (happy_simulator_amd/sharded.py) -- the same bits as
        one engine, a few dozen rounds instead of tens of thousands of windows."""
        from .sharded import LocalComm, ShardedNetwork

        world = -(-arrays.n // self._resident_stations())
        with ShardedNetwork.on_gpu(arrays, net, LocalComm(world), horizon_ns=end_ns, start_ns=self._start_time.nanoseconds,
                                   seed=self._seed, device=self._device, log_capacity=self._log_cap(g, horizon_s, arrays, True),
                                   **({"msg_capacity": self._msg_capacity} if self._msg_capacity else {})) as sn:
            es = sn.run_until(end_ns)
            stats, counts, t_ns, created_ns, net_stats = sn.collect(arrays.n, net.n_links)
            if self._probes:
                write_back_probes(g, sn)
        write_back(g, stats, counts, t_ns, created_ns, net_stats, device=self._device)
        write_back_shared_sink_probes(g)
        drained = es.final_time_ns <= end_ns
        self._events_cancelled = sum(1 for t in cancelled_ns if drained or t <= es.final_time_ns)
        return self._finish(es, _time.monotonic() - wall0)

    def _finish(self, es, wall_s: float) -> SimulationSummary:
        """What every engine's run leaves on the Simulation: its summary `es`, the clock and the SimulationSummary."""
        self._engine_summary = es
        self._events_processed = es.events_processed
        self._current_time = Instant(es.final_time_ns)
        self._summary = self._build_summary(wall_s)
        return self._summary

    # core/simulation.py:543-591
    def _build_summary(self, wall_elapsed: float) -> SimulationSummary:
        duration_s = (self._current_time - self._start_time).to_seconds()
        eps = self._events_processed / duration_s if duration_s > 0 else 0.0
        return SimulationSummary(duration_s=duration_s, total_events_processed=self._events_processed,
                                 events_cancelled=self._events_cancelled, events_per_second=eps,
                                 wall_clock_seconds=wall_elapsed,
                                 # (eager like the reference for ordinary sizes; beyond 4 096 entities the loop is deferred until
                                 #  somebody reads the dict -- it would cost more than the device run)
                                 entities=(entity_summaries(self._entities) if len(self._entities) <= 4096 else
                                           LazyEntities(lambda ents=self._entities: entity_summaries(ents))))


def entity_summaries(entities) -> dict[str, EntitySummary]:
    """Simulation._build_entity_summaries (core/simulation.py:560-591): `events_handled` is the first int among the
    attributes count / events_received / stats_processed; QueuedResources report accepted / dropped (peak depth is never
    tracked by the reference, :572)."""
    out: dict[str, EntitySummary] = {}
    for comp in entities:
        if not isinstance(comp, Entity):
            continue
        queue_stats = None
        if isinstance(comp, Server):
            queue_stats = QueueStats(peak_depth=0, total_accepted=comp.stats_accepted, total_dropped=comp.stats_dropped)
        handled = 0
        for attr in ("count", "events_received", "stats_processed"):
            val = getattr(comp, attr, None)
            if isinstance(val, int):
                handled = val
                break
        out[comp.name] = EntitySummary(name=comp.name, entity_type=type(comp).__name__, events_handled=handled,
                                       queue_stats=queue_stats)
    return out
