"""Host-side mirror of the reference's entity constructors for the hot path.

These classes carry PARAMETERS into the engine and RESULTS back out; they contain no event logic (that
lives in csrc/).  Names, argument meaning, defaults and error behaviour follow the reference:

  Source.poisson / Source.constant / Source(name, event_provider, arrival_time_provider)
                                                   happysimulator/load/source.py:93-268
  SimpleEventProvider(target, event_type, stop_after)            load/source.py:31-86
  ExponentialLatency / ConstantLatency             distributions/exponential.py:15-45, constant.py:15-35
  Server(name, concurrency, service_time, queue_policy, queue_capacity, downstream)
                                                   components/server/server.py:43-273
  Sink / Counter                                   components/common.py:18-95
  LatencyTracker                                   instrumentation/collectors.py:18-60
  NetworkLink(name, latency, bandwidth_bps, packet_loss_rate, jitter, egress)
                                                   components/network/link.py:36-234
  RandomRouter(name, targets=[...])                components/random_router.py:9-45
"""
from __future__ import annotations

import random as _random
from dataclasses import dataclass

import numpy as np

from .core.event import Event
from .core.temporal import Duration, Instant


class Entity:
    """Base of every simulation actor (core/entity.py:31-127): a name and topology links."""

    def __init__(self, name: str):
        self.name = name

    def downstream_entities(self) -> list["Entity"]:
        return []

    def has_capacity(self) -> bool:
        return True


# ---- distributions -------------------------------------------------------------------------------
class LatencyDistribution:
    __slots__ = ("_mean_latency",)      # (slotted like the other leaf objects of a chain: lowering 65 536 chains is a walk over
                                        #  ~600 000 Python objects, bound by the cache lines each visit touches)

    def __init__(self, mean_latency):
        if isinstance(mean_latency, Duration):
            self._mean_latency = mean_latency.to_seconds()
        else:
            self._mean_latency = float(mean_latency)

    @property
    def mean(self) -> float:
        return self._mean_latency


class ExponentialLatency(LatencyDistribution):
    """Exponentially distributed latency; on the engine: sample = -hs_log(1-u) / (1/mean)."""
    __slots__ = ("_lambda",)

    def __init__(self, mean_latency):
        super().__init__(mean_latency)
        self._lambda = 1 / self._mean_latency


class ConstantLatency(LatencyDistribution):
    __slots__ = ()

    def get_latency(self, current_time=None) -> Duration:
        return Duration.from_seconds(self._mean_latency)         # distributions/constant.py:33-35


class _CompoundLatency(LatencyDistribution):
    """faults/network_faults.py:27-44: what an active InjectLatency leaves in `link.latency` -- the link's original distribution
    plus a ConstantLatency of the extra.  The engine adds the two terms the same way (csrc/hs_graph.hip, the link handler)."""
    __slots__ = ("_base", "_extra")

    def __init__(self, base: LatencyDistribution, extra: LatencyDistribution):
        super().__init__(base._mean_latency + extra._mean_latency)
        self._base = base
        self._extra = extra

    def get_latency(self, current_time=None) -> Duration:
        return Duration.from_seconds(self._base.get_latency(current_time).to_seconds() + self._extra.get_latency(current_time).to_seconds())


# ---- queue policy --------------------------------------------------------------------------------
class FIFOQueue:
    """components/queue_policy.py:75-114 -- the policy every engine runs (LIFOQueue, AdaptiveLIFO, CoDelQueue: the single-heap loop)."""
    __slots__ = ("_capacity",)

    def __init__(self, capacity: float = float("inf")):
        self._capacity = capacity

    @property
    def capacity(self) -> float:
        return self._capacity


class LIFOQueue:
    """components/queue_policy.py:117-156: push appends and refuses at capacity, pop takes the newest item.  Runs on the single-heap
    loop; `len()` is the depth the last run left."""
    __slots__ = ("_capacity", "_len")

    def __init__(self, capacity: float = float("inf")):
        self._capacity = capacity
        self._len = 0

    @property
    def capacity(self) -> float:
        return self._capacity

    def is_empty(self) -> bool:
        return self._len == 0

    def __len__(self) -> int:
        return self._len


@dataclass(frozen=True)
class AdaptiveLIFOStats:
    enqueued: int = 0
    dequeued_fifo: int = 0
    dequeued_lifo: int = 0
    capacity_rejected: int = 0
    mode_switches: int = 0


class AdaptiveLIFO:
    """components/queue_policies/adaptive_lifo.py: FIFO below `congestion_threshold` items, LIFO from there on; the test is made when
    an item is popped, before it is removed.  Runs on the single-heap loop; the counters are the last run's."""

    def __init__(self, congestion_threshold: int, capacity: int | None = None):
        if congestion_threshold < 1:
            raise ValueError(f"congestion_threshold must be >= 1, got {congestion_threshold}")
        if capacity is not None and capacity < 1:
            raise ValueError(f"capacity must be >= 1 or None, got {capacity}")
        self._congestion_threshold = congestion_threshold
        self._capacity = float("inf") if capacity is None else capacity
        self._len = 0
        self._was_congested = False
        self._enqueued = 0
        self._dequeued_fifo = 0
        self._dequeued_lifo = 0
        self._capacity_rejected = 0
        self._mode_switches = 0

    @property
    def stats(self) -> AdaptiveLIFOStats:
        return AdaptiveLIFOStats(enqueued=self._enqueued, dequeued_fifo=self._dequeued_fifo, dequeued_lifo=self._dequeued_lifo,
                                 capacity_rejected=self._capacity_rejected, mode_switches=self._mode_switches)

    @property
    def congestion_threshold(self) -> int:
        return self._congestion_threshold

    @property
    def capacity(self) -> float:
        return self._capacity

    @property
    def is_congested(self) -> bool:
        return self._len >= self._congestion_threshold

    @property
    def mode(self) -> str:
        return "LIFO" if self.is_congested else "FIFO"

    def is_empty(self) -> bool:
        return self._len == 0

    def __len__(self) -> int:
        return self._len


@dataclass(frozen=True)
class CoDelStats:
    enqueued: int = 0
    dequeued: int = 0
    dropped: int = 0
    capacity_rejected: int = 0
    drop_intervals: int = 0


class CoDelQueue:
    """components/queue_policies/codel.py: a FIFO that, when the sojourn time of the items it pops has stayed above `target_delay` for
    `interval`, drops the items behind the popped one at a rate that grows with the square root of the drop count.  Runs on the
    single-heap loop; the clock is the Simulation's, so `clock_func` / `set_clock` are accepted and ignored."""

    def __init__(self, target_delay: float = 0.005, interval: float = 0.100, capacity: int | None = None, clock_func=None):
        if target_delay <= 0:
            raise ValueError(f"target_delay must be > 0, got {target_delay}")
        if interval <= 0:
            raise ValueError(f"interval must be > 0, got {interval}")
        if capacity is not None and capacity < 1:
            raise ValueError(f"capacity must be >= 1 or None, got {capacity}")
        self._target_delay = target_delay
        self._interval = interval
        self._capacity = float("inf") if capacity is None else capacity
        self._clock_func = clock_func
        self._len = 0
        self._first_above_time: Instant | None = None
        self._drop_next: Instant | None = None
        self._count = 0
        self._dropping = False
        self._last_count = 0
        self._enqueued = 0
        self._dequeued = 0
        self._dropped = 0
        self._capacity_rejected = 0
        self._drop_intervals = 0

    @property
    def stats(self) -> CoDelStats:
        return CoDelStats(enqueued=self._enqueued, dequeued=self._dequeued, dropped=self._dropped,
                          capacity_rejected=self._capacity_rejected, drop_intervals=self._drop_intervals)

    @property
    def target_delay(self) -> float:
        return self._target_delay

    @property
    def interval(self) -> float:
        return self._interval

    @property
    def capacity(self) -> float:
        return self._capacity

    @property
    def dropping(self) -> bool:
        return self._dropping

    def set_clock(self, clock_func) -> None:
        self._clock_func = clock_func

    def is_empty(self) -> bool:
        return self._len == 0

    def __len__(self) -> int:
        return self._len


QUEUE_POLICIES = (LIFOQueue, AdaptiveLIFO, CoDelQueue)          # the policies next to the FIFO that the single-heap loop runs


def _refused_queue_policy(name: str, why: str):
    """A reference policy that no engine runs: the class exists so that Server's refusal can name it and say why."""
    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs
    return type(name, (), {"__init__": __init__, "_refusal": why, "__doc__": f"Not lowered: {why}."})


PriorityQueue = _refused_queue_policy("PriorityQueue", "its order comes from a host callable or the items' own comparison")
DeadlineQueue = _refused_queue_policy("DeadlineQueue", "its deadlines come from a host callable")
FairQueue = _refused_queue_policy("FairQueue", "its flows come from a host callable")
WeightedFairQueue = _refused_queue_policy("WeightedFairQueue", "its flows and weights come from host callables")
REDQueue = _refused_queue_policy("REDQueue", "it draws from the process-wide random generator")


# ---- load ----------------------------------------------------------------------------------------
@dataclass(frozen=True, slots=True)
class ConstantRateProfile:
    rate: float

    def get_rate(self, time: Instant) -> float:
        return self.rate

    @property
    def peak_rate(self) -> float:
        return self.rate


@dataclass(frozen=True)
class LinearRampProfile:
    """Rate ramping linearly from start_rate to end_rate over duration_s, constant afterwards (load/profile.py:52-75)."""

    duration_s: float
    start_rate: float
    end_rate: float

    def get_rate(self, time: Instant) -> float:
        t = time.to_seconds()
        if t <= 0:
            return self.start_rate
        if t >= self.duration_s:
            return self.end_rate
        fraction = t / self.duration_s
        return self.start_rate + fraction * (self.end_rate - self.start_rate)

    @property
    def peak_rate(self) -> float:
        return max(self.start_rate, self.end_rate)


@dataclass(frozen=True)
class SpikeProfile:
    """baseline_rate, then spike_rate during [warmup_s, warmup_s + spike_duration_s), then baseline_rate again
    (load/profile.py:78-113)."""

    baseline_rate: float = 10.0
    spike_rate: float = 150.0
    warmup_s: float = 10.0
    spike_duration_s: float = 15.0

    def get_rate(self, time: Instant) -> float:
        t = time.to_seconds()
        if t < self.warmup_s:
            return self.baseline_rate
        if t < self.warmup_s + self.spike_duration_s:
            return self.spike_rate
        return self.baseline_rate

    @property
    def peak_rate(self) -> float:
        return max(self.baseline_rate, self.spike_rate)


# Results of a run on n plain chains whose objects have not been bound to them yet (lowering.write_back_plain): binding 4 x 65 536
# objects costs more than the run, so it happens when somebody first reads or writes a result attribute of ANY lowered entity
# (or starts another run) -- the same laziness as the Sink records that stay on the device until they are read.
_PENDING: list = []


def _flush_pending() -> None:
    if not _PENDING:
        return
    import gc

    was = gc.isenabled()
    gc.disable()                   # (65 536 new tuples would otherwise trigger full collections over ~600 000 live objects)
    try:
        while _PENDING:
            _PENDING.pop(0)()
    finally:
        if was:
            gc.enable()


_LAZY_LOOKUPS = 32                 # objects bound one by one (an identity search in the run's object lists) before everything is


def _resolve(obj) -> None:
    """A result attribute of `obj` is being touched while a run's results are not bound yet.  Round 5: bind THIS object alone --
    the pending run (lowering.write_back_plain) finds its row by an identity search, ~1 ms at 65 536 chains -- instead of all
    4 x n objects (16-33 ms there: the first counter read after run() cost 70 x the device run); whoever walks many objects gets
    the bulk binding after a few lookups.  Several pending runs, or an object the run does not know: bind everything, in run order."""
    if len(_PENDING) == 1:
        ent = _PENDING[0]
        find = getattr(ent, "find_and_bind", None)
        if find is not None and ent.lookups < _LAZY_LOOKUPS and find(obj):
            ent.lookups += 1
            return
    _flush_pending()


class _Stat:
    """A result counter of an entity: its own value, or -- after a run on n plain chains (lowering.write_back_plain) -- row
    `_bound[1]` of the run's per-LP result arrays `_bound[0]`.  Binding an object is ONE attribute store instead of one per
    counter (196 608 objects at the headline size); assigning a value un-binds the object (the general write-back sets them all)."""

    def __init__(self, key, cast=int, default=0):
        self.key, self.cast, self.default = key, cast, default

    def __set_name__(self, owner, name):
        self.own = "_own" + name

    def __get__(self, obj, owner=None):
        if obj is None:
            return self
        if _PENDING:
            _resolve(obj)
        b = obj._bound
        if b is None:
            return obj.__dict__.get(self.own, self.default)
        key = self.key
        return self.cast(b[0][key][b[1]]) if isinstance(key, str) else key(b[0], b[1])

    def __set__(self, obj, value):
        if _PENDING:
            _flush_pending()
        obj.__dict__[self.own] = value
        if obj._bound is not None:
            obj._bound = None


class SimpleEventProvider:
    # (the attributes the lowering reads live in slots -- inline in the object, no dictionary to chase; everything else, the
    #  _Stat values included, goes to the instance __dict__ as before)
    __slots__ = ("_bound", "_target", "_event_type", "_stop_after", "__dict__")
    _generated = _Stat(lambda st, i: int(st["accepted"][i] + st["dropped"][i]))     # Requests handed out

    def __init__(self, target: Entity, event_type: str = "Request", stop_after: Instant | None = None,
                 context_fn=None):
        if context_fn is not None:
            raise NotImplementedError("context_fn is arbitrary Python and is not lowered to the engine")
        self._bound = None                  # (set first: _Stat's setter reads it; the same keys in the same order keep the instance dicts shared)
        self._target = target
        self._event_type = event_type
        self._stop_after = stop_after
        self._generated = 0


class _ArrivalProvider:
    kind = "constant"
    __slots__ = ("profile",)

    def __init__(self, profile, start_time: Instant = None):
        if not isinstance(profile, (ConstantRateProfile, LinearRampProfile, SpikeProfile)):
            raise NotImplementedError(
                f"profile {type(profile).__name__} is arbitrary Python; the engine lowers ConstantRateProfile, "
                "LinearRampProfile and SpikeProfile (load/profile.py)")
        self.profile = profile


class ConstantArrivalTimeProvider(_ArrivalProvider):
    kind = "constant"
    __slots__ = ()


class PoissonArrivalTimeProvider(_ArrivalProvider):
    kind = "poisson"
    __slots__ = ()


class Source(Entity):
    __slots__ = ("_bound", "_event_provider", "_time_provider")
    _generated_count = _Stat("generated")

    def __init__(self, name: str, event_provider: SimpleEventProvider, arrival_time_provider: _ArrivalProvider):
        super().__init__(name)
        self._bound = None
        self._event_provider = event_provider
        self._time_provider = arrival_time_provider
        self._generated_count = 0

    @classmethod
    def _make(cls, provider_cls, rate, target, event_type, name, stop_after, event_provider):
        if event_provider is None:
            if target is None:
                raise ValueError("Either 'target' or 'event_provider' must be provided")
            event_provider = SimpleEventProvider(target, event_type, cls._resolve_stop_after(stop_after))
        return cls(name=name, event_provider=event_provider,
                   arrival_time_provider=provider_cls(ConstantRateProfile(rate=rate), start_time=Instant.Epoch))

    @classmethod
    def constant(cls, rate: float, target: Entity | None = None, event_type: str = "Request", *,
                 name: str = "Source", stop_after=None, event_provider=None) -> "Source":
        return cls._make(ConstantArrivalTimeProvider, rate, target, event_type, name, stop_after, event_provider)

    @classmethod
    def poisson(cls, rate: float, target: Entity | None = None, event_type: str = "Request", *,
                name: str = "Source", stop_after=None, event_provider=None) -> "Source":
        return cls._make(PoissonArrivalTimeProvider, rate, target, event_type, name, stop_after, event_provider)

    @classmethod
    def with_profile(cls, profile, target: Entity | None = None, event_type: str = "Request", *, poisson: bool = True,
                     name: str = "Source", stop_after=None, event_provider=None) -> "Source":
        """A Source whose arrival rate follows `profile` (load/source.py:271-320)."""
        if event_provider is None:
            if target is None:
                raise ValueError("Either 'target' or 'event_provider' must be provided")
            event_provider = SimpleEventProvider(target, event_type, cls._resolve_stop_after(stop_after))
        provider_cls = PoissonArrivalTimeProvider if poisson else ConstantArrivalTimeProvider
        return cls(name=name, event_provider=event_provider, arrival_time_provider=provider_cls(profile, start_time=Instant.Epoch))

    @staticmethod
    def _resolve_stop_after(stop_after):
        if stop_after is None:
            return None
        if isinstance(stop_after, Instant):
            return stop_after
        return Instant.from_seconds(stop_after)

    @property
    def generated_count(self) -> int:
        return self._generated_count

    @property
    def rate(self) -> float:
        """The profile's rate; for a time-varying profile its peak (what sizes the engine's record logs)."""
        return self._time_provider.profile.peak_rate

    def downstream_entities(self) -> list[Entity]:
        t = getattr(self._event_provider, "_target", None)
        return [t] if isinstance(t, Entity) else []

    def __repr__(self):
        return f"<Source {self.name}>"


# ---- server --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ServerStats:
    requests_completed: int = 0
    requests_rejected: int = 0
    total_service_time: float = 0.0


class _QueueView:
    """What users read off `server.queue`: acceptance / drop counters and depth."""
    _bound = None
    stats_accepted = _Stat("accepted")
    stats_dropped = _Stat("dropped")
    depth = _Stat("queue_depth")

    def __init__(self):
        self._bound = None
        self.stats_accepted = 0
        self.stats_dropped = 0
        self.depth = 0


class Server(Entity):
    __slots__ = ("_bound", "_policy", "_concurrency", "_service_time", "_downstream", "_queue")
    _requests_completed = _Stat("completed")
    _requests_rejected = _Stat("rejected")
    _total_service_time = _Stat("total_service_s", float, 0.0)
    _active = _Stat("active")

    def __init__(self, name: str, concurrency: int = 1, service_time: LatencyDistribution | None = None,
                 queue_policy: "FIFOQueue | LIFOQueue | AdaptiveLIFO | CoDelQueue | None" = None, queue_capacity: int | None = None,
                 downstream: Entity | None = None):
        super().__init__(name)
        if not isinstance(concurrency, int):
            raise NotImplementedError("only FixedConcurrency (an int) is lowered to the engine")
        if concurrency < 1:
            raise ValueError(f"max_concurrent must be >= 1, got {concurrency}")   # server/concurrency.py:87-88
        if queue_policy is None:
            queue_policy = FIFOQueue(capacity=queue_capacity if queue_capacity is not None else float("inf"))
        elif not isinstance(queue_policy, (FIFOQueue,) + QUEUE_POLICIES):     # (with a policy given, queue_capacity is ignored)
            why = getattr(queue_policy, "_refusal", "only FIFOQueue, LIFOQueue, AdaptiveLIFO and CoDelQueue are")
            raise NotImplementedError(f"queue_policy {type(queue_policy).__name__} is not lowered to the engine: {why}")
        self._bound = None
        self._policy = queue_policy
        self._concurrency = concurrency
        self._service_time = service_time or ConstantLatency(0.01)
        self._downstream = downstream
        self._queue = _QueueView()
        self._requests_completed = 0
        self._requests_rejected = 0
        self._total_service_time = 0.0
        self._active = 0

    def downstream_entities(self) -> list[Entity]:
        return [self._downstream] if self._downstream is not None else []

    @property
    def downstream(self):
        return self._downstream

    @downstream.setter
    def downstream(self, target):
        self._downstream = target

    @property
    def concurrency(self) -> int:
        return self._concurrency

    @property
    def service_time(self) -> LatencyDistribution:
        return self._service_time

    @property
    def queue(self) -> _QueueView:
        return self._queue

    @property
    def queue_policy(self):
        return self._policy

    @property
    def depth(self) -> int:
        return self._queue.depth

    @property
    def stats_accepted(self) -> int:
        return self._queue.stats_accepted

    @property
    def stats_dropped(self) -> int:
        return self._queue.stats_dropped

    @property
    def active_requests(self) -> int:
        return self._active

    @property
    def utilization(self) -> float:
        return self._active / self._concurrency if self._concurrency else 0.0

    @property
    def average_service_time(self) -> float:
        return self._total_service_time / self._requests_completed if self._requests_completed else 0.0

    @property
    def stats(self) -> ServerStats:
        return ServerStats(self._requests_completed, self._requests_rejected, self._total_service_time)

    def has_capacity(self, weight: int = 1) -> bool:
        return self._active < self._concurrency


# ---- sinks ---------------------------------------------------------------------------------------
def _percentile_sorted(sorted_values, p: float) -> float:
    """instrumentation/data.py:197-210."""
    n = len(sorted_values)
    if n == 0:
        return 0.0
    if p <= 0:
        return float(sorted_values[0])
    if p >= 1:
        return float(sorted_values[-1])
    pos = p * (n - 1)
    lo = int(pos)
    hi = min(lo + 1, n - 1)
    frac = pos - lo
    return float(sorted_values[lo] * (1.0 - frac) + sorted_values[hi] * frac)


_DEVICE_STATS_MIN = 4096      # Sink.latency_stats(): records from which the device routine is used


class _RecordSink(Entity):
    """Shared result holder: the engine hands back (completion ns, created_at ns) arrays; the Python lists the
    reference exposes are materialised lazily (31 M-element lists are the user's choice, not ours)."""

    _EMPTY = np.zeros(0, np.int64)

    def __init__(self, name: str):
        super().__init__(name)
        self._rec_t = self._EMPTY
        self._rec_cr = self._EMPTY
        self._lazy = None                   # (LazyRecords, station): the run's records are still on the device (lowering.py)
        self._device = 0

    def _set_records(self, t_ns: np.ndarray, created_ns: np.ndarray):
        if _PENDING:
            _flush_pending()
        self._rec_t = t_ns
        self._rec_cr = created_ns
        self._lazy = None

    def _bind_lazy(self, records, station: int, device: int = 0):
        self._lazy = (records, station)
        self._device = device

    def _materialise(self):
        if _PENDING:
            _resolve(self)
        if self._lazy is not None:
            records, i = self._lazy
            self._rec_t, self._rec_cr = records.records(i)
            self._lazy = None

    @property
    def _t_ns(self) -> np.ndarray:
        self._materialise()
        return self._rec_t

    @property
    def _created_ns(self) -> np.ndarray:
        self._materialise()
        return self._rec_cr

    def _n_records(self) -> int:
        if _PENDING:
            _resolve(self)
        return self._lazy[0].count(self._lazy[1]) if self._lazy is not None else int(len(self._rec_t))

    @property
    def completion_ns(self) -> np.ndarray:
        return self._t_ns

    @property
    def latencies_array(self) -> np.ndarray:
        # (event.time - created_at).to_seconds() = float(ns) / 1e9   (components/common.py:39-40)
        return (self._t_ns - self._created_ns).astype(np.float64) / 1_000_000_000


class Sink(_RecordSink):
    def __init__(self, name: str = "Sink"):
        super().__init__(name)

    @property
    def events_received(self) -> int:
        return self._n_records()

    @property
    def completion_times(self) -> list[Instant]:
        return [Instant(int(t)) for t in self._t_ns]

    @property
    def latencies_s(self) -> list[float]:
        return self.latencies_array.tolist()

    def average_latency(self) -> float:
        lat = self.latencies_s
        return sum(lat) / len(lat) if lat else 0.0

    def latency_time_series_seconds(self):
        return [t.to_seconds() for t in self.completion_times], list(self.latencies_s)

    def latency_stats(self) -> dict:
        dev = getattr(self, "_device_latency_stats", None)
        if dev is not None:                      # a load balancer's shared Sink: computed by the engine (hs_lb_latency_stats)
            return dict(dev)
        n = len(self._t_ns)
        if n >= _DEVICE_STATS_MIN:               # a large record set stays numeric: sort + sum + percentiles on the device
            from . import _native as N

            if N.lib().hs_device_count() > 0:
                import ctypes as C

                t = np.ascontiguousarray(self._t_ns, np.int64)
                cr = np.ascontiguousarray(self._created_ns, np.int64)
                out = (C.c_double * 6)()
                rc = N.lib().hs_sink_latency_stats(getattr(self, "_device", 0), n, t.ctypes.data, cr.ctypes.data, out)
                if rc != N.HS_OK:
                    raise N.EngineError(rc, (N.lib().hs_lb_last_error(None) or b"").decode())
                return {"count": int(out[0]), "avg": out[1], "min": out[2], "max": out[3], "p50": out[4], "p99": out[5]}
        lat = self.latencies_s
        if n == 0:
            return {"count": 0, "avg": 0.0, "min": 0.0, "max": 0.0, "p50": 0.0, "p99": 0.0}
        s = sorted(lat)
        return {"count": n, "avg": sum(s) / n, "min": s[0], "max": s[-1],
                "p50": _percentile_sorted(s, 0.50), "p99": _percentile_sorted(s, 0.99)}


class Counter(_RecordSink):
    def __init__(self, name: str = "Counter"):
        super().__init__(name)
        self._event_type = "Request"

    @property
    def total(self) -> int:
        return self._n_records()

    @property
    def by_type(self) -> dict:
        return {self._event_type: self.total} if self.total else {}


class LatencyTracker(_RecordSink):
    def __init__(self, name: str = "LatencyTracker"):
        super().__init__(name)

    @property
    def count(self) -> int:
        return self._n_records()

    def mean_latency(self) -> float:
        lat = self.latencies_array
        return float(sum(lat.tolist()) / len(lat)) if len(lat) else 0.0

    def _pct(self, p):
        return _percentile_sorted(sorted(self.latencies_array.tolist()), p)

    def p50(self) -> float:
        return self._pct(0.50)

    def p99(self) -> float:
        return self._pct(0.99)


# ---- networks of stations ------------------------------------------------------------------------
@dataclass(frozen=True)
class NetworkLinkStats:
    bytes_transmitted: int = 0
    packets_sent: int = 0
    packets_dropped: int = 0


class NetworkLink(Entity):
    """Point-to-point link (components/network/link.py:36-234).  Lowered: a constant base latency > 0 (it is the
    lookahead of the conservative windows) plus optional jitter -- ExponentialLatency (one draw per packet) or ConstantLatency (a
    constant on top, as the reference's datacenter_network preset has it) --, towards a Server.  `packet_loss_rate` is
    lowered with the link's own Philox LOSS stream in place of the process-wide `random.random()` (link.py:131).
    `bandwidth_bps` is accepted: requests of the lowered event providers carry no payload_size, so their transmission
    time is 0 s and `bytes_transmitted` stays 0, as in the reference (link.py:209-234)."""

    def __init__(self, name: str, latency: LatencyDistribution, bandwidth_bps: float | None = None,
                 packet_loss_rate: float = 0.0, jitter: LatencyDistribution | None = None, egress: Entity | None = None):
        super().__init__(name)
        if packet_loss_rate < 0.0 or packet_loss_rate > 1.0:
            raise ValueError(f"packet_loss_rate must be in [0, 1], got {packet_loss_rate}")   # link.py:71-72
        self.latency = latency
        self.bandwidth_bps = bandwidth_bps
        self.packet_loss_rate = packet_loss_rate
        self.jitter = jitter
        self.egress = egress
        self.bytes_transmitted = 0
        self.packets_sent = 0
        self.packets_dropped = 0
        self._entered = 0
        self._loss_draws = 0              # values read from the link's LOSS stream: one per Request that met a rate > 0
        self._reverse_of = None           # the link this one is Network.add_bidirectional_link's reverse copy of

    def downstream_entities(self) -> list[Entity]:
        return [self.egress] if self.egress is not None else []

    @property
    def link_stats(self) -> NetworkLinkStats:
        return NetworkLinkStats(self.bytes_transmitted, self.packets_sent, self.packets_dropped)

    @property
    def current_utilization(self) -> float:
        return 0.0          # bandwidth is infinite on the lowered path (link.py:93-95)


@dataclass(frozen=True)
class LinkStats:
    """components/network/network.py:28-44."""
    source: str = ""
    destination: str = ""
    packets_sent: int = 0
    packets_dropped: int = 0
    bytes_transmitted: int = 0


class Network(Entity):
    """components/network/network.py:82-426 as a REGISTRY: the links by (source name, destination name), where the link faults
    (faults.InjectLatency / InjectPacketLoss) look theirs up.  Traffic goes to the links directly -- `add_link` sets `link.egress` --;
    routing by an Event's source / destination metadata (`handle_event`, `send`) and partitions are not lowered, so the three routing
    counters stay 0.  In `entities=[...]` a Network holds its place in the entity order and receives no Events."""

    def __init__(self, name: str, default_link: "NetworkLink | None" = None):
        super().__init__(name)
        self.default_link = default_link
        self._routes: dict[tuple[str, str], NetworkLink] = {}
        self._known_entities: dict[str, Entity] = {}
        self.events_routed = 0
        self.events_dropped_no_route = 0
        self.events_dropped_partition = 0

    def add_link(self, source: Entity, dest: Entity, link: "NetworkLink") -> None:
        self._known_entities[source.name] = source
        self._known_entities[dest.name] = dest
        link.egress = dest                                           # network.py:141-142
        self._routes[(source.name, dest.name)] = link

    def add_bidirectional_link(self, a: Entity, b: Entity, link: "NetworkLink") -> None:
        """network.py:153-190: the reverse direction is a shallow copy named `<name>_reverse` with its stats zeroed.  The copy shares
        the forward link's jitter object (and, in the recorded runs, its loss stream): it may be looked up and read, but a run that
        sends traffic through it or names it in a fault is refused."""
        import copy

        link.egress = b
        self._routes[(a.name, b.name)] = link
        reverse = copy.copy(link)
        reverse.name = f"{link.name}_reverse"
        reverse.egress = a
        reverse.bytes_transmitted = 0
        reverse.packets_sent = 0
        reverse.packets_dropped = 0
        reverse._entered = 0
        reverse._loss_draws = 0
        reverse._reverse_of = link
        self._routes[(b.name, a.name)] = reverse
        self._known_entities[a.name] = a
        self._known_entities[b.name] = b

    def get_link(self, source_name: str, dest_name: str) -> "NetworkLink | None":
        return self._routes.get((source_name, dest_name), self.default_link)

    def is_partitioned(self, source_name: str, dest_name: str) -> bool:
        return False

    def traffic_matrix(self) -> list[LinkStats]:
        return [LinkStats(source=s, destination=d, packets_sent=link.packets_sent, packets_dropped=link.packets_dropped,
                          bytes_transmitted=link.bytes_transmitted) for (s, d), link in self._routes.items()]

    @staticmethod
    def _refuse(what: str):
        from .lowering import UnsupportedTopology

        raise UnsupportedTopology(f"Network.{what} is not lowered: it acts on traffic routed by Network.handle_event, and the lowered "
                                  "traffic goes to the links directly")

    def partition(self, group_a, group_b, *, asymmetric: bool = False):
        self._refuse("partition")

    def heal_partition(self) -> None:
        self._refuse("heal_partition")

    def send(self, source, destination, event_type, payload=None, daemon=False):
        self._refuse("send")


# ---- network condition presets (components/network/conditions.py:13-258): the same nine links, from one table ----------------
_NETWORK_PRESETS = {
    # name of the function: (default link name, base latency s, bandwidth bit/s, packet loss, jitter kind, jitter mean s)
    "local_network": ("local", 0.0001, 1_000_000_000, 0.0, None, 0.0),
    "datacenter_network": ("datacenter", 0.0005, 10_000_000_000, 0.0, "const", 0.0001),
    "cross_region_network": ("cross_region", 0.050, 1_000_000_000, 0.0001, "exp", 0.005),
    "internet_network": ("internet", 0.100, 100_000_000, 0.001, "exp", 0.020),
    "satellite_network": ("satellite", 0.600, 10_000_000, 0.005, "exp", 0.050),
    "mobile_3g_network": ("mobile_3g", 0.100, 2_000_000, 0.005, "exp", 0.030),
    "mobile_4g_network": ("mobile_4g", 0.050, 20_000_000, 0.001, "exp", 0.015),
}


def _preset_link(key: str, name: str | None = None) -> "NetworkLink":
    dflt, lat, bw, loss, jk, jm = _NETWORK_PRESETS[key]
    jitter = None if jk is None else ConstantLatency(jm) if jk == "const" else ExponentialLatency(jm)
    return NetworkLink(name=dflt if name is None else name, latency=ConstantLatency(lat), bandwidth_bps=bw, packet_loss_rate=loss,
                       jitter=jitter)


def local_network(name: str = "local"): return _preset_link("local_network", name)
def datacenter_network(name: str = "datacenter"): return _preset_link("datacenter_network", name)
def cross_region_network(name: str = "cross_region"): return _preset_link("cross_region_network", name)
def internet_network(name: str = "internet"): return _preset_link("internet_network", name)
def satellite_network(name: str = "satellite"): return _preset_link("satellite_network", name)
def mobile_3g_network(name: str = "mobile_3g"): return _preset_link("mobile_3g_network", name)
def mobile_4g_network(name: str = "mobile_4g"): return _preset_link("mobile_4g_network", name)


def lossy_network(loss_rate: float, name: str = "lossy", base_latency: float = 0.010):
    """conditions.py:148-178: a 100 Mbit/s link that drops `loss_rate` of its packets."""
    if loss_rate < 0.0 or loss_rate > 1.0:
        raise ValueError(f"loss_rate must be in [0, 1], got {loss_rate}")
    return NetworkLink(name=name, latency=ConstantLatency(base_latency), bandwidth_bps=100_000_000, packet_loss_rate=loss_rate, jitter=None)


def slow_network(latency_seconds: float, name: str = "slow", bandwidth_bps: float = 1_000_000):
    """conditions.py:181-204."""
    return NetworkLink(name=name, latency=ConstantLatency(latency_seconds), bandwidth_bps=bandwidth_bps, packet_loss_rate=0.0, jitter=None)


class RandomRouter(Entity):
    """Uniform random fan-out (components/random_router.py:9-45); the engine draws the target from the router's own
    Philox stream: index = int(u * len(targets))."""

    def __init__(self, name: str, *, targets: list[Entity]):
        super().__init__(name)
        self.targets = targets
        self.stats_routed = 0
        self.target_counts: dict[str, int] = {}

    def downstream_entities(self) -> list[Entity]:
        return list(self.targets)


# ---- load balancing ------------------------------------------------------------------------------
class ClientKeyEventProvider:
    """One Request per tick whose metadata carries a random `client_id` for key-based strategies -- the request factory
    of examples/visual/chash_example.py:69-88 (`ClientRequestProvider`: `client_id = rng.randint(0, NUM_CLIENTS - 1)`).
    On the engine the id is `int(u * n_clients)` with u from the source's own Philox KEY stream, and the routing key is
    its decimal string, as `ConsistentHash._default_get_key` would return it (strategies.py:369-375)."""

    def __init__(self, target: Entity, n_clients: int, stop_after: Instant | float | None = None,
                 event_type: str = "Request"):
        if n_clients < 1:
            raise ValueError(f"n_clients must be >= 1, got {n_clients}")
        self._target = target
        self._n_clients = int(n_clients)
        self._event_type = event_type
        self._stop_after = Source._resolve_stop_after(stop_after)
        self._generated = 0


class ConsistentHash:
    """Consistent hashing with virtual nodes (components/load_balancer/strategies.py:336-433): every backend owns
    `virtual_nodes` points md5("<name>:<i>") on a ring; a request goes to the first point whose hash is >= md5(key).
    The ring is built (and searched) inside libhs_hip.so; `ring_backends` / `select_name` expose it for inspection."""

    def __init__(self, virtual_nodes: int = 100, get_key=None):
        if virtual_nodes < 1:
            raise ValueError(f"virtual_nodes must be >= 1, got {virtual_nodes}")        # strategies.py:356-357
        if get_key is not None:
            raise NotImplementedError("a custom get_key is arbitrary Python; the engine hashes metadata['client_id']")
        self._virtual_nodes = int(virtual_nodes)
        self._fallback = RoundRobin()       # what a Request without a key gets (strategies.py:362,420-421): only the single-heap path runs those

    @property
    def virtual_nodes(self) -> int:
        return self._virtual_nodes


class RoundRobin:
    """Cycles through the backends (components/load_balancer/strategies.py:50-73), the LoadBalancer's default strategy: the k-th
    Request the LoadBalancer processes goes to backends[k % len(backends)].  On the engine the Requests of all Sources are ranked
    by arrival on the device (csrc/hs_lb.hip hs_lb_rr_assign); `_index` holds the number of selections after a run."""

    def __init__(self):
        self._index = 0

    def reset(self) -> None:
        self._index = 0


class _Weighted:
    """`_weights` (backend.name -> weight), `set_weight` / `get_weight` of the two weighted strategies (strategies.py:88-109,199-211).
    `LoadBalancer.add_backend(backend, weight=)` calls `set_weight` when it registers the backend (load_balancer.py:203-205) -- so
    `LoadBalancer(backends=[...], strategy=s)` resets the weights `s` held for them to 1, as in the reference: weights are set through
    `add_backend(b, weight=w)` or by `set_weight` AFTER the LoadBalancer exists."""

    def __init__(self):
        self._weights: dict[str, int] = {}
        self._default_weight = 1

    def set_weight(self, backend: Entity, weight: int) -> None:
        if weight < 1:
            raise ValueError(f"weight must be >= 1, got {weight}")                        # strategies.py:103-104,205-206
        self._weights[backend.name] = weight

    def get_weight(self, backend: Entity) -> int:
        return self._weights.get(backend.name, self._default_weight)


class WeightedRoundRobin(_Weighted):
    """Smooth weighted round robin (components/load_balancer/strategies.py:75-134): every current weight grows by its backend's
    weight, the first maximum is taken and loses the total weight W.  The sequence is periodic in W, so the engine selects
    table[k % W] for the k-th Request from one period built in libhs_hip.so (csrc/hs_wrr.hpp; `selection_table`).  After a run
    `_selections` holds the number of selections and `_current_weights` what the reference's dict holds: w_i * t - W * n_i."""

    MAX_TOTAL_WEIGHT = 1 << 24

    def __init__(self):
        super().__init__()
        self._current_weights: dict[str, int] = {}
        self._selections = 0

    @staticmethod
    def selection_table(weights) -> np.ndarray:
        """One period of the selection sequence over backends 0 .. n-1 (hs_lb_wrr_table; host only, no device)."""
        from . import _native as N
        w = np.ascontiguousarray(weights, np.int32)
        if len(w) == 0:
            return np.zeros(0, np.int32)
        if (w < 1).any():
            raise ValueError(f"weight must be >= 1, got {int(w[w < 1][0])}")
        total = int(w.astype(np.int64).sum())
        if total > WeightedRoundRobin.MAX_TOTAL_WEIGHT:
            raise NotImplementedError(f"WeightedRoundRobin: a total weight of {total} needs a selection table beyond 2^24 entries "
                                      "(not lowered)")
        out = np.zeros(total, np.int32)
        got = N.lib().hs_lb_wrr_table(w.ctypes.data, len(w), out.ctypes.data, total)
        if got != total:
            raise N.EngineError(int(got), (N.lib().hs_graph_last_error(None) or b"").decode())
        return out


class IPHash:
    """Hash of the client key (strategies.py:294-333): backends[int(md5(key).hexdigest(), 16) % len(backends)] with key =
    str(metadata["client_id"]); a Request without a key takes the strategy's own RoundRobin (`_fallback`), which only such Requests
    advance.  On the engine a client -> backend table, like ConsistentHash's."""

    def __init__(self, get_key=None):
        if get_key is not None:
            raise NotImplementedError("a custom get_key is arbitrary Python; the engine hashes metadata['client_id']")
        self._fallback = RoundRobin()


class LeastConnections:
    """The backend with the fewest active connections (strategies.py:152-186): min(backends, key=active_requests), the first
    minimum in add_backend order; a Server's `active_requests` is the requests in service, not its queue depth.  The choice feeds
    back from backend state, so only the single-heap loop orders it (csrc/hs_graph.hip: all 64 lanes scan the backends)."""


class WeightedLeastConnections(_Weighted):
    """Least connections with weights (strategies.py:189-237): min(backends, key=active_requests / weight), a true division in
    binary64; the first minimum wins."""


class Random:
    """Random backend selection (strategies.py:137-150: `random.choice(backends)`).  On the engine the choice is
    backends[int(u * len(backends))] with u the Request's draw from its Source's own Philox KEY stream -- the seed-matched form
    of the process-wide `random`, pinned against the reference with that plug (tests/golden/make_golden.py
    `_PerRequestChoice`)."""


class PowerOfTwoChoices:
    """strategies.py:436-475: `random.sample(backends, 2)` on the process-wide generator.  Constructible for API parity; a LoadBalancer
    refuses it by name (no stream of the engine defines that draw)."""


class LeastResponseTime:
    """strategies.py:240-291: `random.choice` among the backends without data, fed by a host-side `record_response_time`.
    Constructible for API parity; a LoadBalancer refuses it by name."""

    def __init__(self, alpha: float = 0.3):
        if not 0 < alpha <= 1:
            raise ValueError(f"alpha must be in (0, 1], got {alpha}")                    # strategies.py:255-256
        self._alpha = alpha


LOWERED_STRATEGIES = (ConsistentHash, RoundRobin, Random, WeightedRoundRobin, IPHash, LeastConnections, WeightedLeastConnections)


@dataclass(frozen=True)
class LoadBalancerStats:
    """components/load_balancer/load_balancer.py:40-58."""

    requests_received: int = 0
    requests_forwarded: int = 0
    requests_failed: int = 0
    no_backend_available: int = 0
    backends_marked_unhealthy: int = 0
    backends_marked_healthy: int = 0


@dataclass
class BackendInfo:
    """load_balancer.py:61-80.  `is_healthy` is what mark_unhealthy / mark_healthy left, before a run on the host and during one
    on the device (a HealthChecker's marks); the consecutive counters are host-side bookkeeping the engine does not keep."""

    backend: Entity
    weight: int = 1
    is_healthy: bool = True
    consecutive_failures: int = 0
    consecutive_successes: int = 0
    total_requests: int = 0
    total_failures: int = 0


class LoadBalancer(Entity):
    """Distributes requests over backends (components/load_balancer/load_balancer.py:83-473).  Lowered: the ConsistentHash,
    RoundRobin (the default), Random, WeightedRoundRobin, IPHash, LeastConnections and WeightedLeastConnections strategies over Server
    backends.  Backends marked unhealthy -- by mark_unhealthy before the run or by a HealthChecker during it -- leave the routing
    pool (`healthy_backends`: registration order, filtered); that is lowered for RoundRobin, WeightedRoundRobin and the two
    LeastConnections strategies, on the single-heap loop."""

    def __init__(self, name: str, backends: list[Entity] | None = None, strategy=None, on_no_backend: str = "reject"):
        super().__init__(name)
        if on_no_backend not in ("reject", "queue"):
            raise ValueError(f"on_no_backend must be 'reject' or 'queue', got {on_no_backend}")   # load_balancer.py:120-121
        if strategy is None:
            strategy = RoundRobin()                                                       # load_balancer.py:112
        if not isinstance(strategy, LOWERED_STRATEGIES):
            why = ""
            if type(strategy).__name__ in ("PowerOfTwoChoices", "LeastResponseTime"):
                # random.sample / random.choice on the process-wide generator (strategies.py:289,470): no engine stream defines them
                why = ": it draws from the process-wide random generator, which no stream of the engine defines"
            raise NotImplementedError(f"strategy {type(strategy).__name__} is not lowered to the engine{why} (ConsistentHash, RoundRobin, "
                                      "Random, WeightedRoundRobin, IPHash, LeastConnections and WeightedLeastConnections are)")
        self._strategy = strategy
        self._on_no_backend = on_no_backend
        self._backends: dict[str, BackendInfo] = {}
        for b in backends or []:
            self.add_backend(b)
        self._requests_received = 0
        self._requests_forwarded = 0
        self._requests_failed = 0
        self._no_backend_available = 0
        self._backends_marked_unhealthy = 0
        self._backends_marked_healthy = 0
        self._in_flight_count = 0

    def mark_unhealthy(self, backend: Entity) -> None:
        """load_balancer.py:244-270: out of the routing pool until marked healthy again (an unknown backend: a no-op)."""
        info = self._backends.get(backend.name)
        if info is not None and info.is_healthy:
            info.is_healthy = False
            info.consecutive_successes = 0
            self._backends_marked_unhealthy += 1

    def mark_healthy(self, backend: Entity) -> None:
        """load_balancer.py:272-297."""
        info = self._backends.get(backend.name)
        if info is not None and not info.is_healthy:
            info.is_healthy = True
            info.consecutive_failures = 0
            self._backends_marked_healthy += 1

    def add_backend(self, backend: Entity, weight: int = 1) -> None:
        if weight < 1:
            raise ValueError(f"weight must be >= 1, got {weight}")                        # load_balancer.py:207-208
        if backend.name in self._backends:
            self._backends[backend.name].weight = weight                                  # (the strategy keeps its weight, :189-196)
            return
        self._backends[backend.name] = BackendInfo(backend=backend, weight=weight)
        if hasattr(self._strategy, "set_weight"):                                         # load_balancer.py:203-205: a backend's FIRST
            self._strategy.set_weight(backend, weight)                                    # registration sets the strategy's weight

    def remove_backend(self, backend: Entity) -> None:
        self._backends.pop(backend.name, None)

    @property
    def strategy(self):
        return self._strategy

    @property
    def all_backends(self) -> list[Entity]:
        return [i.backend for i in self._backends.values()]

    @property
    def healthy_backends(self) -> list[Entity]:
        return [i.backend for i in self._backends.values() if i.is_healthy]

    @property
    def unhealthy_backends(self) -> list[Entity]:
        return [i.backend for i in self._backends.values() if not i.is_healthy]

    @property
    def backend_count(self) -> int:
        return len(self._backends)

    @property
    def healthy_count(self) -> int:
        return len(self.healthy_backends)

    def downstream_entities(self) -> list[Entity]:
        return self.all_backends

    def get_backend_info(self, backend: Entity) -> BackendInfo | None:
        return self._backends.get(backend.name)

    def get_backend_info_by_name(self, name: str) -> BackendInfo | None:
        return self._backends.get(name)

    @property
    def stats(self) -> LoadBalancerStats:
        return LoadBalancerStats(self._requests_received, self._requests_forwarded, self._requests_failed,
                                 self._no_backend_available, self._backends_marked_unhealthy, self._backends_marked_healthy)


@dataclass(frozen=True)
class HealthCheckStats:
    """components/load_balancer/health_check.py:44-53."""

    checks_performed: int = 0
    checks_passed: int = 0
    checks_failed: int = 0
    checks_timed_out: int = 0
    backends_marked_healthy: int = 0
    backends_marked_unhealthy: int = 0


@dataclass
class BackendHealthState:
    """health_check.py:56-64."""

    consecutive_successes: int = 0
    consecutive_failures: int = 0
    last_check_time: Instant | None = None
    last_check_passed: bool | None = None
    is_checking: bool = False


class HealthChecker(Entity):
    """Periodic health checks of a LoadBalancer's backends (components/load_balancer/health_check.py:67-448).  Every `interval`
    seconds a probe -- an ordinary Event aimed at the backend, queued and served like a Request -- goes to every backend that is
    not being checked, with a timeout Event `timeout` seconds later; the probe's completion hook (it fires when the backend's
    enqueue handler returns) is the response.  `unhealthy_threshold` consecutive timeouts mark a backend unhealthy at the
    LoadBalancer, `healthy_threshold` consecutive responses mark it healthy again.  The three handlers run on the device
    (csrc/hs_graph.hip kEvHcCycle / kEvHcResp / kEvHcTimeout); this class carries the parameters in and the statistics and
    per-backend states back out.  `sim.schedule(checker.start())` begins the cycle, as in the reference."""

    def __init__(self, name: str, load_balancer: LoadBalancer, interval: float = 10.0, timeout: float = 5.0, healthy_threshold: int = 2,
                 unhealthy_threshold: int = 3, check_event_type: str = "health_check"):
        super().__init__(name)
        if interval <= 0:                                                                 # health_check.py:109-118
            raise ValueError(f"interval must be > 0, got {interval}")
        if timeout <= 0:
            raise ValueError(f"timeout must be > 0, got {timeout}")
        if timeout >= interval:
            raise ValueError(f"timeout ({timeout}) must be < interval ({interval})")
        if healthy_threshold < 1:
            raise ValueError(f"healthy_threshold must be >= 1, got {healthy_threshold}")
        if unhealthy_threshold < 1:
            raise ValueError(f"unhealthy_threshold must be >= 1, got {unhealthy_threshold}")
        self._load_balancer = load_balancer
        self._interval = interval
        self._timeout = timeout
        self._healthy_threshold = healthy_threshold
        self._unhealthy_threshold = unhealthy_threshold
        self._check_event_type = check_event_type
        self._backend_states: dict[str, BackendHealthState] = {}
        self._pending_checks: dict[str, int] = {}
        self._next_check_id = 0
        self._checks_performed = 0
        self._checks_passed = 0
        self._checks_failed = 0
        self._checks_timed_out = 0
        self._backends_marked_healthy = 0
        self._backends_marked_unhealthy = 0
        self._is_running = False
        self._sim_start: Instant | None = None           # the clock a Simulation hands to its entities: `now` before run() is its start
        self._events = (0, 0, 0)                         # after a run: its cycle / response / timeout Events processed (dropped ones included)

    def downstream_entities(self) -> list[Entity]:
        return [self._load_balancer]

    @property
    def stats(self) -> HealthCheckStats:
        return HealthCheckStats(self._checks_performed, self._checks_passed, self._checks_failed, self._checks_timed_out,
                                self._backends_marked_healthy, self._backends_marked_unhealthy)

    @property
    def load_balancer(self) -> LoadBalancer:
        return self._load_balancer

    @property
    def interval(self) -> float:
        return self._interval

    @property
    def timeout(self) -> float:
        return self._timeout

    @property
    def healthy_threshold(self) -> int:
        return self._healthy_threshold

    @property
    def unhealthy_threshold(self) -> int:
        return self._unhealthy_threshold

    @property
    def is_running(self) -> bool:
        return self._is_running

    def start(self):
        """health_check.py:201-216: the first `_health_check_cycle` Event, for `sim.schedule(...)`; its time is the Simulation's
        start once the checker is one of its entities, Instant.Epoch before."""
        from .core.event import Event

        self._is_running = True
        return Event(time=self._sim_start if self._sim_start is not None else Instant.Epoch, event_type="_health_check_cycle",
                     target=self, context={})

    def stop(self) -> None:
        self._is_running = False

    def get_backend_state(self, backend: Entity) -> BackendHealthState:
        if backend.name not in self._backend_states:
            self._backend_states[backend.name] = BackendHealthState()
        return self._backend_states[backend.name]

    def get_backend_state_by_name(self, name: str) -> BackendHealthState | None:
        return self._backend_states.get(name)


# ---- rate limiting -------------------------------------------------------------------------------
# components/rate_limiter/policy.py and rate_limited_entity.py.  Inside a Simulation the policies run on the device
# (csrc/hs_graph.hip lim_try_acquire / lim_wait_ns); `try_acquire` / `time_until_available` here are the same arithmetic in host
# Python -- binary64, `Instant - Instant` exact, `Instant +- float` truncating float * 1e9 -- so the classes work on their own, and
# the two implementations check each other against the recorded reference (tests/test_rate_limiter_host.py).
class TokenBucketPolicy:
    """Token bucket (policy.py:65-127): `refill_rate` tokens per second up to `capacity`, one token per request."""

    def __init__(self, capacity: float = 10.0, refill_rate: float = 1.0, initial_tokens: float | None = None):
        self._capacity = float(capacity)
        self._refill_rate = float(refill_rate)
        self._tokens = self._capacity if initial_tokens is None else float(initial_tokens)
        self._last_refill_time: Instant | None = None

    capacity = property(lambda self: self._capacity)
    refill_rate = property(lambda self: self._refill_rate)
    tokens = property(lambda self: self._tokens)

    def _refill(self, now: Instant) -> None:
        last = self._last_refill_time
        if last is None:                      # the first call only starts the clock
            self._last_refill_time = now
            return
        elapsed = (now - last).to_seconds()
        if elapsed > 0:
            self._tokens = min(self._capacity, self._tokens + elapsed * self._refill_rate)
            self._last_refill_time = now

    def try_acquire(self, now: Instant) -> bool:
        self._refill(now)
        if self._tokens >= 1.0:
            self._tokens -= 1.0
            return True
        return False

    def time_until_available(self, now: Instant) -> Duration:
        self._refill(now)
        if self._tokens >= 1.0:
            return Duration.ZERO
        wait = Duration.from_seconds((1.0 - self._tokens) / self._refill_rate)
        return Duration(1) if wait == Duration.ZERO else wait       # progress guard (policy.py:124-126)

    def _engine_params(self):
        return N_LIMITER["token"], self._capacity, self._refill_rate, self._tokens, 0

    def _pristine(self) -> bool:
        return self._last_refill_time is None


class LeakyBucketPolicy:
    """Leaky bucket (policy.py:130-170): one request per 1 / leak_rate seconds, no bursts."""

    def __init__(self, leak_rate: float = 1.0):
        self._leak_rate = float(leak_rate)
        self._leak_interval = 1.0 / leak_rate if leak_rate > 0 else float("inf")
        self._last_leak_time: Instant | None = None

    leak_rate = property(lambda self: self._leak_rate)

    def try_acquire(self, now: Instant) -> bool:
        last = self._last_leak_time
        if last is None or (now - last).to_seconds() >= self._leak_interval:
            self._last_leak_time = now
            return True
        return False

    def time_until_available(self, now: Instant) -> Duration:
        last = self._last_leak_time
        if last is None:
            return Duration.ZERO
        remaining = self._leak_interval - (now - last).to_seconds()
        if remaining <= 0:
            return Duration.ZERO
        wait = Duration.from_seconds(remaining)
        return Duration(1) if wait == Duration.ZERO else wait       # policy.py:167-169

    def _engine_params(self):
        return N_LIMITER["leaky"], self._leak_rate, self._leak_interval, 0.0, 0

    def _pristine(self) -> bool:
        return self._last_leak_time is None


class SlidingWindowPolicy:
    """Sliding window log (policy.py:173-222): at most `max_requests` grants inside any window of `window_size_seconds`."""

    def __init__(self, window_size_seconds: float = 1.0, max_requests: int = 10):
        self._window_size = float(window_size_seconds)
        self._max_requests = int(max_requests)
        self._request_log: list[Instant] = []

    window_size_seconds = property(lambda self: self._window_size)
    max_requests = property(lambda self: self._max_requests)

    def _prune(self, now: Instant) -> None:
        cutoff = now - self._window_size
        log = self._request_log
        k = 0
        while k < len(log) and log[k] < cutoff:
            k += 1
        if k:
            del log[:k]

    def try_acquire(self, now: Instant) -> bool:
        self._prune(now)
        if len(self._request_log) < self._max_requests:
            self._request_log.append(now)
            return True
        return False

    def time_until_available(self, now: Instant) -> Duration:
        self._prune(now)
        if len(self._request_log) < self._max_requests:
            return Duration.ZERO
        expires_at = self._request_log[0] + self._window_size      # the oldest grant leaves the window then
        wait = Duration.from_seconds((expires_at - now).to_seconds())
        return Duration(1) if wait == Duration.ZERO else wait       # policy.py:219-221

    def _engine_params(self):
        return N_LIMITER["sliding"], self._window_size, 0.0, 0.0, self._max_requests

    def _pristine(self) -> bool:
        return not self._request_log


class FixedWindowPolicy:
    """Fixed window counter (policy.py:225-289): `requests_per_window` grants per window; windows start at multiples of
    `window_size`, computed as `(now_s // window_size) * window_size` in floats."""

    def __init__(self, requests_per_window: int, window_size: float = 1.0):
        if requests_per_window < 1:
            raise ValueError(f"requests_per_window must be >= 1, got {requests_per_window}")
        if window_size <= 0:
            raise ValueError(f"window_size must be > 0, got {window_size}")
        self._requests_per_window = requests_per_window
        self._window_size = window_size
        self._current_window_start: Instant | None = None
        self._current_window_count: int = 0

    requests_per_window = property(lambda self: self._requests_per_window)
    window_size = property(lambda self: self._window_size)

    def _get_window_start(self, now: Instant) -> Instant:
        return Instant.from_seconds((now.to_seconds() // self._window_size) * self._window_size)

    def _maybe_reset(self, now: Instant) -> None:
        start = self._get_window_start(now)
        if self._current_window_start is None or start > self._current_window_start:
            self._current_window_start = start
            self._current_window_count = 0

    def try_acquire(self, now: Instant) -> bool:
        self._maybe_reset(now)
        if self._current_window_count < self._requests_per_window:
            self._current_window_count += 1
            return True
        return False

    def time_until_available(self, now: Instant) -> Duration:
        self._maybe_reset(now)
        if self._current_window_count < self._requests_per_window:
            return Duration.ZERO
        remaining = ((self._current_window_start + self._window_size) - now).to_seconds()
        if remaining <= 0:
            return Duration.ZERO
        wait = Duration.from_seconds(remaining)
        return Duration(1) if wait == Duration.ZERO else wait       # policy.py:286-288

    def _engine_params(self):
        return N_LIMITER["fixed"], float(self._window_size), 0.0, 0.0, int(self._requests_per_window)

    def _pristine(self) -> bool:
        return self._current_window_start is None and self._current_window_count == 0


N_LIMITER = {"token": 0, "leaky": 1, "sliding": 2, "fixed": 3}      # hs_limiter_policy (include/hs_engine.h)
LIMITER_POLICIES = (TokenBucketPolicy, LeakyBucketPolicy, SlidingWindowPolicy, FixedWindowPolicy)


@dataclass(frozen=True)
class RateLimitedEntityStats:
    received: int = 0
    forwarded: int = 0
    queued: int = 0
    dropped: int = 0


class RateLimitedEntity(Entity):
    """Admission control in front of `downstream` (rate_limited_entity.py:40-193): a Request the policy grants is forwarded at once,
    one it denies waits in a FIFO of `queue_capacity` places that a self-scheduled daemon poll drains at the moment the policy
    reports capacity; only a full queue drops.  Runs on the single-heap loop (csrc/hs_graph.hip kEvLimRequest / kEvLimPoll)."""

    def __init__(self, name: str, downstream: Entity, policy, queue_capacity: int = 1000):
        super().__init__(name)
        self._downstream = downstream
        self._policy = policy
        self._queue = FIFOQueue(capacity=queue_capacity)
        self._queue_depth = 0
        self._poll_scheduled = False
        self._received = self._forwarded = self._queued = self._dropped = 0
        self.received_times: list[Instant] = []
        self.forwarded_times: list[Instant] = []
        self.dropped_times: list[Instant] = []

    def downstream_entities(self) -> list[Entity]:
        return [self._downstream]

    @property
    def downstream(self) -> Entity:
        return self._downstream

    @property
    def policy(self):
        return self._policy

    @property
    def queue_depth(self) -> int:
        return self._queue_depth

    @property
    def stats(self) -> RateLimitedEntityStats:
        return RateLimitedEntityStats(received=self._received, forwarded=self._forwarded, queued=self._queued, dropped=self._dropped)


# ---- resilience ----------------------------------------------------------------------------------
# components/resilience/bulkhead.py and timeout.py: the two client-side guards that are pure event logic.  Their handlers run on the
# device (csrc/hs_graph.hip kEvBhReq .. kEvTwTimeout); these classes carry the parameters in and the reference's state back out.
# Hedge and Fallback (hedge.py, fallback.py) follow below: they send a Request a second time, from a copy of its context the device keeps
# (kEvHgReq .. kEvFbFbResp).  CircuitBreaker (never leaves CLOSED without a host `failure_predicate`) is not mirrored.
@dataclass(frozen=True)
class BulkheadStats:
    """bulkhead.py:35-45."""

    total_requests: int = 0
    accepted_requests: int = 0
    rejected_requests: int = 0
    timed_out_requests: int = 0
    queued_requests: int = 0
    peak_concurrent: int = 0
    peak_queue_depth: int = 0


class Bulkhead(Entity):
    """At most `max_concurrent` Requests in flight at `target` (bulkhead.py:57-409): a Request beyond that waits in a queue of
    `max_wait_queue` places for at most `max_wait_time` seconds (None: for ever), one beyond that is rejected.  A permit returns
    when the completion hook of the forwarded Event fires -- when the target's handler returns, or a NetworkLink's transit ends --
    so a Request dropped at a crashed target keeps its permit for good, as in the reference."""

    MAX_CONCURRENT = 65536                    # include/hs_engine.h HS_BULKHEAD_MAX_CONCURRENT: the ids the in-flight table holds

    def __init__(self, name: str, target: Entity, max_concurrent: int, max_wait_queue: int = 0, max_wait_time: float | None = None):
        super().__init__(name)
        if max_concurrent < 1:                                                            # bulkhead.py:98-103
            raise ValueError(f"max_concurrent must be >= 1, got {max_concurrent}")
        if max_wait_queue < 0:
            raise ValueError(f"max_wait_queue must be >= 0, got {max_wait_queue}")
        if max_wait_time is not None and max_wait_time <= 0:
            raise ValueError(f"max_wait_time must be > 0 or None, got {max_wait_time}")
        self._target = target
        self._max_concurrent = max_concurrent
        self._max_wait_queue = max_wait_queue
        self._max_wait_time = max_wait_time
        self._active_count = 0
        self._wait_queue: list[int] = []          # after a run: the request ids that still wait, head first
        self._next_request_id = 0
        self._in_flight: dict[int, dict] = {}     # after a run: the ids in flight (the reference's values hold Events: not mirrored)
        self._total_requests = 0
        self._accepted_requests = 0
        self._rejected_requests = 0
        self._timed_out_requests = 0
        self._queued_requests = 0
        self._peak_concurrent = 0
        self._peak_queue_depth = 0

    def downstream_entities(self) -> list[Entity]:
        return [self._target]

    @property
    def target(self) -> Entity:
        return self._target

    @property
    def max_concurrent(self) -> int:
        return self._max_concurrent

    @property
    def max_wait_queue(self) -> int:
        return self._max_wait_queue

    @property
    def max_wait_time(self) -> float | None:
        return self._max_wait_time

    @property
    def active_count(self) -> int:
        return self._active_count

    @property
    def queue_depth(self) -> int:
        return len(self._wait_queue)

    @property
    def available_permits(self) -> int:
        return max(0, self._max_concurrent - self._active_count)

    @property
    def stats(self) -> BulkheadStats:
        return BulkheadStats(total_requests=self._total_requests, accepted_requests=self._accepted_requests,
                             rejected_requests=self._rejected_requests, timed_out_requests=self._timed_out_requests,
                             queued_requests=self._queued_requests, peak_concurrent=self._peak_concurrent,
                             peak_queue_depth=self._peak_queue_depth)


@dataclass(frozen=True)
class TimeoutStats:
    """timeout.py:32-38."""

    total_requests: int = 0
    successful_requests: int = 0
    timed_out_requests: int = 0


class TimeoutWrapper(Entity):
    """A deadline of `timeout` seconds on every Request forwarded to `target` (timeout.py:41-295): the response -- the forwarded
    Event's completion hook -- and the timeout Event each resolve the request if it is still in flight, whichever comes second is a
    no-op.  `on_timeout` is a host callable: not lowered."""

    def __init__(self, name: str, target: Entity, timeout: float, on_timeout=None):
        super().__init__(name)
        if timeout <= 0:                                                                  # timeout.py:76-77
            raise ValueError(f"timeout must be > 0, got {timeout}")
        self._target = target
        self._timeout = timeout
        self._on_timeout = on_timeout
        self._in_flight: dict[int, dict] = {}     # after a run: the ids in flight
        self._next_request_id = 0
        self._total_requests = 0
        self._successful_requests = 0
        self._timed_out_requests = 0

    def downstream_entities(self) -> list[Entity]:
        return [self._target]

    @property
    def target(self) -> Entity:
        return self._target

    @property
    def timeout(self) -> float:
        return self._timeout

    @property
    def in_flight_count(self) -> int:
        return len(self._in_flight)

    @property
    def stats(self) -> TimeoutStats:
        return TimeoutStats(total_requests=self._total_requests, successful_requests=self._successful_requests,
                            timed_out_requests=self._timed_out_requests)


@dataclass(frozen=True)
class HedgeStats:
    """hedge.py:31-39."""

    total_requests: int = 0
    primary_wins: int = 0
    hedge_wins: int = 0
    hedges_sent: int = 0
    hedges_cancelled: int = 0


class Hedge(Entity):
    """A duplicate of every Request that has no response `hedge_delay` seconds after it was forwarded to `target`, up to `max_hedges`
    of them, `hedge_delay` apart (hedge.py:42-362).  The duplicates really flow downstream; the first response -- a forwarded
    Event's completion hook -- decides primary_wins / hedge_wins, and a request's entry leaves `_in_flight` once as many responses have
    come as copies were sent by then.  Behind a crashed or paused target no hook fires: the hedges go out and the entry stays."""

    MAX_HEDGES = 65535                        # include/hs_engine.h HS_HEDGE_MAX_HEDGES: what a request's entry counts

    def __init__(self, name: str, target: Entity, hedge_delay: float, max_hedges: int = 1):
        super().__init__(name)
        if hedge_delay <= 0:                                                              # hedge.py:84-87
            raise ValueError(f"hedge_delay must be > 0, got {hedge_delay}")
        if max_hedges < 1:
            raise ValueError(f"max_hedges must be >= 1, got {max_hedges}")
        self._target = target
        self._hedge_delay = hedge_delay
        self._max_hedges = max_hedges
        # after a run: {id: {"start_time", "completed", "hedges_sent", "responses_received"}} (`original_event` is not mirrored)
        self._in_flight: dict[int, dict] = {}
        self._next_request_id = 0
        self._total_requests = 0
        self._primary_wins = 0
        self._hedge_wins = 0
        self._hedges_sent = 0
        self._hedges_cancelled = 0

    def downstream_entities(self) -> list[Entity]:
        return [self._target]

    @property
    def target(self) -> Entity:
        return self._target

    @property
    def hedge_delay(self) -> float:
        return self._hedge_delay

    @property
    def max_hedges(self) -> int:
        return self._max_hedges

    @property
    def in_flight_count(self) -> int:
        return len(self._in_flight)

    @property
    def stats(self) -> HedgeStats:
        return HedgeStats(total_requests=self._total_requests, primary_wins=self._primary_wins, hedge_wins=self._hedge_wins,
                          hedges_sent=self._hedges_sent, hedges_cancelled=self._hedges_cancelled)


@dataclass(frozen=True)
class FallbackStats:
    """fallback.py:31-40."""

    total_requests: int = 0
    primary_successes: int = 0
    primary_failures: int = 0
    fallback_invocations: int = 0
    fallback_successes: int = 0
    fallback_failures: int = 0


class Fallback(Entity):
    """Every Request goes to `primary`; one without a response after `timeout` seconds is sent again to the `fallback` entity
    (fallback.py:43-410), and a primary response that comes later is ignored.  `timeout=None` never invokes the fallback entity.
    `failure_predicate` and a callable `fallback` are host callables: not lowered.  `fallback_failures` stays 0, as in the reference."""

    def __init__(self, name: str, primary: Entity, fallback, failure_predicate=None, timeout: float | None = None):
        super().__init__(name)
        if timeout is not None and timeout <= 0:                                          # fallback.py:83-84
            raise ValueError(f"timeout must be > 0 or None, got {timeout}")
        self._primary = primary
        self._fallback = fallback
        self._failure_predicate = failure_predicate
        self._timeout = timeout
        self._in_flight: dict[int, dict] = {}     # after a run: {id: {"start_time", "state"}} (`original_event` is not mirrored)
        self._next_request_id = 0
        self._total_requests = 0
        self._primary_successes = 0
        self._primary_failures = 0
        self._fallback_invocations = 0
        self._fallback_successes = 0
        self._fallback_failures = 0

    def downstream_entities(self) -> list[Entity]:
        return [self._primary] + ([self._fallback] if isinstance(self._fallback, Entity) else [])

    @property
    def primary(self) -> Entity:
        return self._primary

    @property
    def fallback(self):
        return self._fallback

    @property
    def timeout(self) -> float | None:
        return self._timeout

    @property
    def stats(self) -> FallbackStats:
        return FallbackStats(total_requests=self._total_requests, primary_successes=self._primary_successes,
                             primary_failures=self._primary_failures, fallback_invocations=self._fallback_invocations,
                             fallback_successes=self._fallback_successes, fallback_failures=self._fallback_failures)


# ---- client --------------------------------------------------------------------------------------
# components/client/retry.py and client.py: the caller that answers a timeout by sending again.  The policies are host Python like the
# limiter policies (they work on their own); the Client's three handlers run on the device (csrc/hs_graph.hip kEvClReq .. kEvClTimeout)
# from a table of delays the host evaluates.  PooledClient / ConnectionPool are not mirrored.
class NoRetry:
    """retry.py:62-90: never retry."""

    def should_retry(self, attempt: int, error: Exception | None = None) -> bool:
        return False

    def get_delay(self, attempt: int) -> float:
        return 0.0


class FixedRetry:
    """retry.py:93-160: the same delay before every retry, `max_attempts` attempts in all."""

    def __init__(self, max_attempts: int, delay: float):
        if max_attempts < 1:
            raise ValueError(f"max_attempts must be >= 1, got {max_attempts}")
        if delay < 0:
            raise ValueError(f"delay must be >= 0, got {delay}")
        self._max_attempts = max_attempts
        self._delay = delay

    @property
    def max_attempts(self) -> int:
        return self._max_attempts

    @property
    def delay(self) -> float:
        return self._delay

    def should_retry(self, attempt: int, error: Exception | None = None) -> bool:
        return attempt < self._max_attempts

    def get_delay(self, attempt: int) -> float:
        return self._delay


class ExponentialBackoff:
    """retry.py:163-289: min(initial_delay * multiplier ** max(0, attempt - 2), max_delay), plus random.uniform(0, jitter) when
    jitter > 0 (the process-wide generator: such a policy works on the host, a Client that holds one is not lowered)."""

    def __init__(self, max_attempts: int, initial_delay: float, max_delay: float, multiplier: float = 2.0, jitter: float = 0.0):
        if max_attempts < 1:
            raise ValueError(f"max_attempts must be >= 1, got {max_attempts}")
        if initial_delay <= 0:
            raise ValueError(f"initial_delay must be > 0, got {initial_delay}")
        if max_delay < initial_delay:
            raise ValueError(f"max_delay ({max_delay}) must be >= initial_delay ({initial_delay})")
        if multiplier < 1:
            raise ValueError(f"multiplier must be >= 1, got {multiplier}")
        if jitter < 0:
            raise ValueError(f"jitter must be >= 0, got {jitter}")
        self._max_attempts = max_attempts
        self._initial_delay = initial_delay
        self._max_delay = max_delay
        self._multiplier = multiplier
        self._jitter = jitter

    @property
    def max_attempts(self) -> int:
        return self._max_attempts

    @property
    def initial_delay(self) -> float:
        return self._initial_delay

    @property
    def max_delay(self) -> float:
        return self._max_delay

    @property
    def multiplier(self) -> float:
        return self._multiplier

    @property
    def jitter(self) -> float:
        return self._jitter

    def should_retry(self, attempt: int, error: Exception | None = None) -> bool:
        return attempt < self._max_attempts

    def get_delay(self, attempt: int) -> float:
        exponent = max(0, attempt - 2)
        delay = self._initial_delay * (self._multiplier**exponent)
        delay = min(delay, self._max_delay)
        if self._jitter > 0:
            delay += _random.uniform(0, self._jitter)
        return delay


class DecorrelatedJitter:
    """retry.py:292-395: random.uniform(base_delay, min(max_delay, previous * 3)) from the process-wide generator -- host only, a Client
    that holds one is not lowered."""

    def __init__(self, max_attempts: int, base_delay: float, max_delay: float):
        if max_attempts < 1:
            raise ValueError(f"max_attempts must be >= 1, got {max_attempts}")
        if base_delay <= 0:
            raise ValueError(f"base_delay must be > 0, got {base_delay}")
        if max_delay < base_delay:
            raise ValueError(f"max_delay ({max_delay}) must be >= base_delay ({base_delay})")
        self._max_attempts = max_attempts
        self._base_delay = base_delay
        self._max_delay = max_delay
        self._previous_delay = base_delay

    @property
    def max_attempts(self) -> int:
        return self._max_attempts

    @property
    def base_delay(self) -> float:
        return self._base_delay

    @property
    def max_delay(self) -> float:
        return self._max_delay

    def should_retry(self, attempt: int, error: Exception | None = None) -> bool:
        return attempt < self._max_attempts

    def get_delay(self, attempt: int) -> float:
        upper = min(self._max_delay, self._previous_delay * 3)
        delay = _random.uniform(self._base_delay, upper)
        self._previous_delay = delay
        return delay

    def reset(self) -> None:
        self._previous_delay = self._base_delay


@dataclass(frozen=True)
class ClientStats:
    """client.py:34-42."""

    requests_sent: int = 0
    responses_received: int = 0
    timeouts: int = 0
    retries: int = 0
    failures: int = 0


class Client(Entity):
    """Sends every Event it receives on to `target` as a NEW Event with a completion hook, waits `timeout` seconds (None: for ever)
    for the hook's response and answers a timeout as `retry_policy` says (client.py:45-470).  Attempts are keyed
    (request_id, attempt); a Request that did not come from `send_request` has no request_id, so all of them share the keys
    (None, attempt), as in the reference.  `on_success` / `on_failure` are host callables: not lowered."""

    MAX_ATTEMPTS = 65536                      # include/hs_engine.h HS_CLIENT_MAX_ATTEMPTS
    MAX_REQUEST_ID = 1 << 30                  # a request_id the engine carries is a positive int below this

    def __init__(self, name: str, target: Entity, timeout: float | None = None, retry_policy=None, on_success=None, on_failure=None):
        super().__init__(name)
        if timeout is not None and timeout < 0:                                           # client.py:89-90
            raise ValueError(f"timeout must be >= 0, got {timeout}")
        self._target = target
        self._timeout = timeout
        self._retry_policy = retry_policy or NoRetry()
        self._on_success = on_success
        self._on_failure = on_failure
        self._in_flight: dict[tuple, dict] = {}    # after a run: the (request_id or None, attempt) keys in flight
        self._next_request_id = 0
        self._requests_sent = 0
        self._responses_received = 0
        self._timeouts = 0
        self._retries = 0
        self._failures = 0
        self._response_times: list[float] = []
        self._sim = None                           # the Simulation that lists it: its clock (core/simulation.py:118-135)

    def downstream_entities(self) -> list[Entity]:
        return [self._target]

    @property
    def target(self) -> Entity:
        return self._target

    @property
    def timeout(self) -> float | None:
        return self._timeout

    @property
    def retry_policy(self):
        return self._retry_policy

    @property
    def in_flight_count(self) -> int:
        return len(self._in_flight)

    @property
    def average_response_time(self) -> float:
        if not self._response_times:
            return 0.0
        return sum(self._response_times) / len(self._response_times)

    @property
    def stats(self) -> ClientStats:
        return ClientStats(requests_sent=self._requests_sent, responses_received=self._responses_received, timeouts=self._timeouts,
                           retries=self._retries, failures=self._failures)

    def send_request(self, payload=None, event_type: str = "request", on_success=None, on_failure=None) -> Event:
        """client.py:163-204: the next request id and an Event aimed at this Client, ready for `Simulation.schedule()` once the caller
        has set its time.  Its time is the clock's `now`: Instant.Epoch outside a Simulation, the Simulation's start time before
        run(), its current time afterwards."""
        self._next_request_id += 1
        now = self._sim._current_time if self._sim is not None else Instant.Epoch
        return Event(time=now, event_type=event_type, target=self,
                     context={"metadata": {"request_id": self._next_request_id, "payload": payload, "attempt": 1, "client_name": self.name},
                              "_on_success": on_success or self._on_success, "_on_failure": on_failure or self._on_failure})

    def get_response_time_percentile(self, percentile: float) -> float:
        """client.py:445-470."""
        if not self._response_times:
            return 0.0
        sorted_times = sorted(self._response_times)
        n = len(sorted_times)
        if percentile <= 0:
            return sorted_times[0]
        if percentile >= 1:
            return sorted_times[-1]
        pos = percentile * (n - 1)
        lo = int(pos)
        hi = min(lo + 1, n - 1)
        frac = pos - lo
        return sorted_times[lo] * (1.0 - frac) + sorted_times[hi] * frac


# ---- stations that hold Requests back --------------------------------------------------------------
# components/industrial/batch_processor.py, conveyor.py, gate_controller.py: the three entities that turn one Event into none now and
# many later.  Their handlers run on the device (csrc/hs_graph.hip kEvBpItem .. kEvGtClose); the delays go there as whole nanoseconds.
# Not mirrored from that package: ShiftedServer, RenegingQueuedResource, BalkingQueue, InspectionStation, BreakdownScheduler (the last
# three draw from the process-wide `random`), SplitMerge (SimFuture), ConditionalRouter (callables).
@dataclass(frozen=True)
class BatchProcessorStats:
    """batch_processor.py:25-31."""

    batches_processed: int = 0
    items_processed: int = 0
    timeouts: int = 0


class BatchProcessor(Entity):
    """Buffers items until `batch_size` of them wait or `timeout_s` has passed since the first one arrived, takes `process_time`
    seconds for the batch and forwards every item to `downstream` (batch_processor.py:34-157).  `timeout_s = 0` never schedules a
    timeout; several batches may be in process at once."""

    MAX_BATCH_SIZE = 1 << 20                  # include/hs_engine.h HS_FLOW_MAX_ITEMS

    def __init__(self, name: str, downstream: Entity, batch_size: int = 10, process_time: float = 1.0, timeout_s: float = 0.0):
        if batch_size <= 0:                                                               # batch_processor.py:59-62
            raise ValueError(f"batch_size must be > 0, got {batch_size}")
        if process_time < 0:
            raise ValueError(f"process_time must be >= 0, got {process_time}")
        super().__init__(name)
        self.downstream = downstream
        self.batch_size = batch_size
        self.process_time = process_time
        self.timeout_s = timeout_s
        self._buffer_depth = 0                # after a run: len(_buffer)
        self._batches_processed = 0
        self._items_processed = 0
        self._timeouts = 0

    def downstream_entities(self) -> list[Entity]:
        return [self.downstream]

    @property
    def batches_processed(self) -> int:
        return self._batches_processed

    @property
    def items_processed(self) -> int:
        return self._items_processed

    @property
    def timeouts(self) -> int:
        return self._timeouts

    @property
    def buffer_depth(self) -> int:
        return self._buffer_depth

    @property
    def stats(self) -> BatchProcessorStats:
        return BatchProcessorStats(batches_processed=self._batches_processed, items_processed=self._items_processed, timeouts=self._timeouts)


@dataclass(frozen=True)
class ConveyorStats:
    """conveyor.py:23-29."""

    items_transported: int = 0
    items_in_transit: int = 0
    items_rejected: int = 0


class ConveyorBelt(Entity):
    """Holds every item for `transit_time` seconds, then forwards it to `downstream`; with `capacity` > 0 an item that finds that many
    in transit is rejected (conveyor.py:32-113)."""

    def __init__(self, name: str, downstream: Entity, transit_time: float, capacity: int = 0):
        if transit_time < 0:                                                              # conveyor.py:53-54
            raise ValueError(f"transit_time must be >= 0, got {transit_time}")
        super().__init__(name)
        self.downstream = downstream
        self.transit_time = transit_time
        self._capacity = capacity             # <= 0: unlimited
        self._items_in_transit = 0
        self._items_transported = 0
        self._items_rejected = 0

    def downstream_entities(self) -> list[Entity]:
        return [self.downstream]

    @property
    def items_in_transit(self) -> int:
        return self._items_in_transit

    @property
    def items_transported(self) -> int:
        return self._items_transported

    @property
    def items_rejected(self) -> int:
        return self._items_rejected

    @property
    def stats(self) -> ConveyorStats:
        return ConveyorStats(items_transported=self._items_transported, items_in_transit=self._items_in_transit,
                             items_rejected=self._items_rejected)

    def has_capacity(self) -> bool:
        return self._capacity <= 0 or self._items_in_transit < self._capacity


@dataclass(frozen=True)
class GateStats:
    """gate_controller.py:23-31."""

    passed_through: int = 0
    queued_while_closed: int = 0
    rejected: int = 0
    open_cycles: int = 0
    is_open: bool = True


class GateController(Entity):
    """Passes items on to `downstream` while open; while closed it queues them, or rejects them once `queue_capacity` (> 0) of them
    wait, and forwards the whole queue when it opens (gate_controller.py:34-186).  `schedule` = [(open_at_s, close_at_s), ...]:
    `start_events()` returns the daemon Events for `Simulation.schedule()`.  `open()` / `close()` before `run()` act on the state the
    run starts from."""

    MAX_QUEUE_CAPACITY = 1 << 20              # include/hs_engine.h HS_FLOW_MAX_ITEMS (a bounded queue; 0 is unbounded)

    def __init__(self, name: str, downstream: Entity, schedule: list | None = None, initially_open: bool = True, queue_capacity: int = 0):
        super().__init__(name)
        self.downstream = downstream
        self.schedule = schedule or []
        self._is_open = initially_open
        self._queue_capacity = queue_capacity
        self._queue_depth = 0                 # after a run: len(_queue)
        self._passed_through = 0
        self._queued_while_closed = 0
        self._rejected = 0
        self._open_cycles = 0

    def downstream_entities(self) -> list[Entity]:
        return [self.downstream]

    @property
    def is_open(self) -> bool:
        return self._is_open

    @property
    def queue_depth(self) -> int:
        return self._queue_depth

    @property
    def stats(self) -> GateStats:
        return GateStats(passed_through=self._passed_through, queued_while_closed=self._queued_while_closed, rejected=self._rejected,
                         open_cycles=self._open_cycles, is_open=self._is_open)

    def start_events(self) -> list[Event]:
        """gate_controller.py:89-111: one daemon `_GateOpen` and one daemon `_GateClose` Event per interval, in list order."""
        events: list[Event] = []
        for open_at, close_at in self.schedule:
            events.append(Event(time=Instant.from_seconds(open_at), event_type="_GateOpen", target=self, daemon=True))
            events.append(Event(time=Instant.from_seconds(close_at), event_type="_GateClose", target=self, daemon=True))
        return events

    def open(self) -> list[Event]:
        """gate_controller.py:154-179 on the host: before a run the queue is empty, so nothing is forwarded."""
        if not self._is_open:
            if self._queue_depth:
                raise NotImplementedError("GateController.open() after a run that left items queued: their Events live on the device")
            self._is_open = True
            self._open_cycles += 1
        return []

    def close(self) -> list[Event]:
        """gate_controller.py:181-186."""
        self._is_open = False
        return []


# ---- pools and stock -----------------------------------------------------------------------------
# components/industrial/pooled_cycle.py, inventory.py: a pool of units with a fixed cycle and a waiting line, and an (s, Q) stock
# counter with lead-time replenishment.  Both are deterministic; their handlers run on the device (csrc/hs_graph.hip kEvPcItem ..
# kEvIbReplenish, the last four of the 64 kinds the loop's kind word holds).  Not mirrored from that package: PerishableInventory (its
# spoilage sweep is a daemon chain over a list of batches), PreemptibleResource (callbacks and SimFuture grants), AppointmentScheduler
# (it draws no-shows from the process-wide `random`, and would need a 65th kind).
@dataclass(frozen=True)
class PooledCycleStats:
    """pooled_cycle.py:24-34."""

    pool_size: int = 0
    available: int = 0
    active: int = 0
    queued: int = 0
    completed: int = 0
    rejected: int = 0
    utilization: float = 0.0


class PooledCycleResource(Entity):
    """`pool_size` identical units; a Request that finds one free holds it for `cycle_time` seconds and then goes on to `downstream`
    (None: it ends there), one that finds none waits in a line -- unbounded with `queue_capacity = 0`, otherwise a Request that finds
    the line full is rejected (pooled_cycle.py:37-179).  A unit that comes free sends the head of the line to the pool again as a new
    Event of the same nanosecond: an arrival of that nanosecond that sorts ahead of it takes the unit, and the waiting Request queues
    again at the back."""

    MAX_POOL_SIZE = 1 << 20                   # include/hs_engine.h HS_POOL_MAX_UNITS (pool_size, and a bounded queue_capacity)

    def __init__(self, name: str, pool_size: int, cycle_time: float, downstream: Entity | None = None, queue_capacity: int = 0):
        if pool_size <= 0:                                                                # pooled_cycle.py:61-64
            raise ValueError(f"pool_size must be > 0, got {pool_size}")
        if cycle_time < 0:
            raise ValueError(f"cycle_time must be >= 0, got {cycle_time}")
        super().__init__(name)
        self.pool_size = pool_size
        self.cycle_time = cycle_time
        self.downstream = downstream
        self._queue_capacity = queue_capacity
        self._available = pool_size
        self._active = 0
        self._queue: list = []                # after a run: one placeholder per waiting Request (the Requests live on the device)
        self._completed = 0
        self._rejected = 0

    def downstream_entities(self) -> list[Entity]:
        return [self.downstream] if self.downstream is not None else []

    @property
    def available(self) -> int:
        return self._available

    @property
    def active(self) -> int:
        return self._active

    @property
    def queued(self) -> int:
        return len(self._queue)

    @property
    def completed(self) -> int:
        return self._completed

    @property
    def rejected(self) -> int:
        return self._rejected

    @property
    def utilization(self) -> float:
        return 0.0 if self.pool_size == 0 else self._active / self.pool_size

    @property
    def stats(self) -> PooledCycleStats:
        return PooledCycleStats(pool_size=self.pool_size, available=self._available, active=self._active, queued=len(self._queue),
                                completed=self._completed, rejected=self._rejected, utilization=self.utilization)


@dataclass(frozen=True)
class InventoryStats:
    """inventory.py:21-37."""

    current_stock: int = 0
    stockouts: int = 0
    reorders: int = 0
    items_consumed: int = 0
    items_replenished: int = 0

    @property
    def fill_rate(self) -> float:
        """The share of the demand that was met from stock (1.0 without any demand)."""
        total = self.items_consumed + self.stockouts
        return 1.0 if total == 0 else self.items_consumed / total


class InventoryBuffer(Entity):
    """A stock counter under an (s, Q) policy: every Request consumes one item and goes on to `downstream`; a Request that finds the
    stock empty counts as a stock-out and goes to `stockout_target`.  Once the stock is at or below `reorder_point` and no order is
    pending, `order_quantity` items are ordered and arrive `lead_time` seconds later (inventory.py:40-194).  `supplier` is kept and
    listed among `downstream_entities()`; nothing is ever sent to it, as in the reference.  Stock and counters are 64-bit."""

    MAX_STOCK = 1 << 62                       # include/hs_engine.h HS_INVENTORY_MAX (initial_stock, reorder_point, order_quantity)
    MAX_LEVEL = (1 << 63) - (1 << 48)         # HS_INVENTORY_MAX_LEVEL: reorder_point + order_quantity, the level the stock can reach

    def __init__(self, name: str, initial_stock: int = 100, reorder_point: int = 20, order_quantity: int = 50, lead_time: float = 5.0,
                 supplier: Entity | None = None, downstream: Entity | None = None, stockout_target: Entity | None = None):
        if initial_stock < 0:                                                             # inventory.py:73-78
            raise ValueError(f"initial_stock must be >= 0, got {initial_stock}")
        if reorder_point < 0:
            raise ValueError(f"reorder_point must be >= 0, got {reorder_point}")
        if order_quantity <= 0:
            raise ValueError(f"order_quantity must be > 0, got {order_quantity}")
        super().__init__(name)
        self._stock = initial_stock
        self.reorder_point = reorder_point
        self.order_quantity = order_quantity
        self.lead_time = lead_time
        self.supplier = supplier
        self.downstream = downstream
        self.stockout_target = stockout_target
        self._stockouts = 0
        self._reorders = 0
        self._items_consumed = 0
        self._items_replenished = 0
        self._order_pending = False

    def downstream_entities(self) -> list[Entity]:
        return [x for x in (self.downstream, self.supplier, self.stockout_target) if x is not None]

    @property
    def stock(self) -> int:
        return self._stock

    @property
    def stats(self) -> InventoryStats:
        return InventoryStats(current_stock=self._stock, stockouts=self._stockouts, reorders=self._reorders,
                              items_consumed=self._items_consumed, items_replenished=self._items_replenished)


# ---- auto scaling --------------------------------------------------------------------------------
# components/deployment/auto_scaler.py.  Inside a Simulation the policies are evaluated on the device (csrc/hs_graph.hip kEvAsEval);
# `evaluate` here is the reference's expression over host objects, for a policy used on its own.
class TargetUtilization:
    """auto_scaler.py:58-98: scale to keep the backends' average utilization near `target`."""

    def __init__(self, target: float = 0.7):
        if not 0 < target <= 1.0:
            raise ValueError(f"target must be in (0, 1], got {target}")
        self._target = target

    @property
    def target(self) -> float:
        return self._target

    def evaluate(self, backends: list, current_count: int, min_instances: int, max_instances: int) -> int:
        if not backends:
            return min_instances
        utilizations = [b.utilization for b in backends if hasattr(b, "utilization")]
        if not utilizations:
            return current_count
        avg_util = sum(utilizations) / len(utilizations)
        if self._target > 0:
            desired = int(current_count * avg_util / self._target + 0.5)
        else:
            desired = current_count
        return max(min_instances, min(max_instances, desired))


class StepScaling:
    """auto_scaler.py:101-139: (utilization threshold, adjustment) steps, evaluated from the highest threshold down."""

    def __init__(self, steps: list):
        self._steps = sorted(steps, key=lambda s: s[0], reverse=True)

    def evaluate(self, backends: list, current_count: int, min_instances: int, max_instances: int) -> int:
        if not backends:
            return current_count
        utilizations = [b.utilization for b in backends if hasattr(b, "utilization")]
        if not utilizations:
            return current_count
        avg_util = sum(utilizations) / len(utilizations)
        for threshold, adjustment in self._steps:
            if avg_util >= threshold:
                desired = current_count + adjustment
                return max(min_instances, min(max_instances, desired))
        return current_count


class QueueDepthScaling:
    """auto_scaler.py:142-168: one instance more or fewer by the backends' total queue depth."""

    def __init__(self, scale_out_threshold: int = 100, scale_in_threshold: int = 10):
        self._scale_out_threshold = scale_out_threshold
        self._scale_in_threshold = scale_in_threshold

    def evaluate(self, backends: list, current_count: int, min_instances: int, max_instances: int) -> int:
        total_depth = 0
        for b in backends:
            if hasattr(b, "depth"):
                total_depth += b.depth
        if total_depth >= self._scale_out_threshold:
            desired = current_count + 1
        elif total_depth <= self._scale_in_threshold and current_count > min_instances:
            desired = current_count - 1
        else:
            desired = current_count
        return max(min_instances, min(max_instances, desired))


SCALING_POLICIES = (TargetUtilization, StepScaling, QueueDepthScaling)


@dataclass
class ScalingEvent:
    """auto_scaler.py:171-179."""

    time: Instant
    action: str
    from_count: int
    to_count: int
    reason: str


@dataclass(frozen=True)
class AutoScalerStats:
    """auto_scaler.py:182-191."""

    evaluations: int = 0
    scale_out_count: int = 0
    scale_in_count: int = 0
    instances_added: int = 0
    instances_removed: int = 0
    cooldown_blocks: int = 0


class AutoScaler(Entity):
    """Periodic controller that adds backends to a LoadBalancer and removes them again (components/deployment/auto_scaler.py:194-455).
    Every `evaluation_interval` seconds the policy reads the backends' utilization or queue depth; a scale-out calls `server_factory`
    for instances `{name}_server_{k}`, a scale-in removes the newest managed ones, and a cooldown follows either.  The handler runs on
    the device (csrc/hs_graph.hip kEvAsEval).  The device cannot call the factory, so the Simulation calls it up front, when it
    lowers the graph, for a pool of P instances -- a bound on what the run can create -- and lowers them as dormant
    Servers; this class carries the parameters in and the statistics, history and membership back out."""

    MAX_POOL = 4096                  # include/hs_engine.h HS_AUTOSCALER_MAX_POOL
    MAX_STEPS = 16                   # HS_AUTOSCALER_MAX_STEPS

    def __init__(self, name: str, load_balancer: LoadBalancer, server_factory, policy=None, min_instances: int = 1, max_instances: int = 10,
                 evaluation_interval: float = 10.0, scale_out_cooldown: float = 30.0, scale_in_cooldown: float = 60.0):
        super().__init__(name)
        self._load_balancer = load_balancer
        self._server_factory = server_factory
        self._policy = policy or TargetUtilization()
        self._min_instances = min_instances
        self._max_instances = max_instances
        self._evaluation_interval = evaluation_interval
        self._scale_out_cooldown = scale_out_cooldown
        self._scale_in_cooldown = scale_in_cooldown
        self._is_running = False
        self._last_scale_time: Instant | None = None
        self._last_scale_action: str | None = None
        self._next_instance_id = 0
        self._managed_servers: list[Entity] = []
        self._evaluations = 0
        self._scale_out_count = 0
        self._scale_in_count = 0
        self._instances_added = 0
        self._instances_removed = 0
        self._cooldown_blocks = 0
        self.scaling_history: list[ScalingEvent] = []
        self._sim_start: Instant | None = None           # the clock a Simulation hands to its entities: `now` before run() is its start
        self._pool: list[Entity] = []                    # the factory's results for instances 1 .. len(_pool), made when a graph is lowered

    def downstream_entities(self) -> list[Entity]:
        return [self._load_balancer] + list(self._managed_servers)

    @property
    def stats(self) -> AutoScalerStats:
        return AutoScalerStats(self._evaluations, self._scale_out_count, self._scale_in_count, self._instances_added,
                               self._instances_removed, self._cooldown_blocks)

    @property
    def load_balancer(self) -> LoadBalancer:
        return self._load_balancer

    @property
    def policy(self):
        return self._policy

    @property
    def min_instances(self) -> int:
        return self._min_instances

    @property
    def max_instances(self) -> int:
        return self._max_instances

    @property
    def current_count(self) -> int:
        return len(self._load_balancer.all_backends)

    @property
    def is_running(self) -> bool:
        return self._is_running

    def start(self):
        """auto_scaler.py:302-315: the first `_autoscaler_evaluate` Event, a daemon, for `sim.schedule(...)`; its time is the
        Simulation's start once the scaler is one of its entities, Instant.Epoch before."""
        from .core.event import Event

        self._is_running = True
        return Event(time=self._sim_start if self._sim_start is not None else Instant.Epoch, event_type="_autoscaler_evaluate",
                     target=self, daemon=True, context={})

    def stop(self) -> None:
        self._is_running = False

    def _instance(self, k: int) -> Entity:
        """Instance k of the pool (1-based), from the factory the first time it is asked for."""
        while len(self._pool) < k:
            self._pool.append(self._server_factory(f"{self.name}_server_{len(self._pool) + 1}"))
        return self._pool[k - 1]


# ---- rolling deployment --------------------------------------------------------------------------
# components/deployment/rolling_deployer.py.  Inside a Simulation the handlers run on the device (csrc/hs_graph.hip kEvRdStart ..).
@dataclass
class DeploymentState:
    """rolling_deployer.py:30-38."""

    status: str = "idle"  # idle, in_progress, completed, rolled_back
    total_instances: int = 0
    replaced: int = 0
    failed: int = 0
    current_batch: int = 0


@dataclass(frozen=True)
class RollingDeployerStats:
    """rolling_deployer.py:41-51."""

    deployments_started: int = 0
    deployments_completed: int = 0
    deployments_rolled_back: int = 0
    instances_replaced: int = 0
    health_checks_performed: int = 0
    health_checks_passed: int = 0
    health_checks_failed: int = 0


class RollingDeployer(Entity):
    """Replaces the backends of a LoadBalancer batch by batch with instances `{name}_v2_{k}` from `server_factory`, health-checking
    every new instance before the old ones of its batch leave, and rolls back after more than `max_failures` failed checks
    (components/deployment/rolling_deployer.py:54-424).  The handlers run on the device (csrc/hs_graph.hip kEvRdStart ..).  The
    device cannot call the factory, so the Simulation calls it up front, when it lowers the graph, for a pool of P instances -- a bound
    on what the scheduled deploy() Events can create -- and lowers them as dormant Servers; this class carries the
    parameters in and the statistics, state and lists back out."""

    MAX_POOL = 4096                  # include/hs_engine.h HS_DEPLOYER_MAX_POOL

    def __init__(self, name: str, load_balancer: LoadBalancer, server_factory, batch_size: int = 1, health_check_interval: float = 2.0,
                 healthy_threshold: int = 2, max_failures: int = 1):
        super().__init__(name)
        self._load_balancer = load_balancer
        self._server_factory = server_factory
        self._batch_size = batch_size
        self._health_check_interval = health_check_interval
        self._healthy_threshold = healthy_threshold
        self._max_failures = max_failures
        self._old_backends: list[Entity] = []
        self._new_backends: list[Entity] = []
        self._current_batch_old: list[Entity] = []
        self._current_batch_new: list[Entity] = []
        self._health_pass_count: dict[str, int] = {}
        self._health_fail_count = 0
        self._next_instance_id = 0
        self._deployments_started = 0
        self._deployments_completed = 0
        self._deployments_rolled_back = 0
        self._instances_replaced = 0
        self._health_checks_performed = 0
        self._health_checks_passed = 0
        self._health_checks_failed = 0
        self.state = DeploymentState()
        self._sim_start: Instant | None = None           # the clock a Simulation hands to its entities: `now` before run() is its start
        self._pool: list[Entity] = []                    # the factory's results for instances 1 .. len(_pool), made when a graph is lowered

    def downstream_entities(self) -> list[Entity]:
        return [self._load_balancer] + list(self._old_backends) + list(self._new_backends)

    @property
    def stats(self) -> RollingDeployerStats:
        return RollingDeployerStats(self._deployments_started, self._deployments_completed, self._deployments_rolled_back,
                                    self._instances_replaced, self._health_checks_performed, self._health_checks_passed,
                                    self._health_checks_failed)

    @property
    def load_balancer(self) -> LoadBalancer:
        return self._load_balancer

    def deploy(self):
        """rolling_deployer.py:145-156: the `_rolling_deploy_start` Event for `sim.schedule(...)`, no daemon; its time is the
        Simulation's start once the deployer is one of its entities, Instant.Epoch before.  The caller may set another time."""
        from .core.event import Event

        return Event(time=self._sim_start if self._sim_start is not None else Instant.Epoch, event_type="_rolling_deploy_start",
                     target=self, context={})

    def _instance(self, k: int) -> Entity:
        """Instance k of the pool (1-based), from the factory the first time it is asked for."""
        while len(self._pool) < k:
            self._pool.append(self._server_factory(f"{self.name}_v2_{len(self._pool) + 1}"))
        return self._pool[k - 1]


# ---- canary deployment ---------------------------------------------------------------------------
# components/deployment/canary_deployer.py.  Inside a Simulation the handlers and the evaluators run on the device (csrc/hs_graph.hip
# kEvCnStart ..); `is_healthy` here is the reference's expression over host objects, for an evaluator used on its own.
@dataclass
class CanaryStage:
    """canary_deployer.py:36-46."""

    traffic_percentage: float
    evaluation_period: float = 30.0


@dataclass
class CanaryState:
    """canary_deployer.py:49-56."""

    status: str = "idle"  # idle, in_progress, promoting, rolled_back, completed
    current_stage: int = 0
    total_stages: int = 0
    canary_traffic_pct: float = 0.0


def _against_baseline(value: float, baseline: list, limit: float, multiplier: float) -> bool:
    """The comparison both evaluators make (canary_deployer.py:87-100, 123-138): the canary's figure against its own limit, then
    against the baseline's plain average times the multiplier where that average is positive."""
    if value > limit:
        return False
    if not baseline:
        return value <= limit
    average = sum(baseline) / len(baseline)
    if average > 0:
        return value <= average * multiplier
    return value <= limit


class ErrorRateEvaluator:
    """canary_deployer.py:76-109: the canary's share of rejected Requests against the baseline's average share."""

    def __init__(self, max_error_rate: float = 0.05, threshold_multiplier: float = 2.0):
        self._max_error_rate = max_error_rate
        self._threshold_multiplier = threshold_multiplier

    def is_healthy(self, canary, baseline_backends: list) -> bool:
        return _against_baseline(self._get_error_rate(canary), [self._get_error_rate(b) for b in baseline_backends],
                                 self._max_error_rate, self._threshold_multiplier)

    def _get_error_rate(self, backend) -> float:
        if hasattr(backend, "stats"):
            stats = backend.stats
            rejected = getattr(stats, "requests_rejected", 0)
            total = getattr(stats, "requests_completed", 0) + rejected
            if total > 0:
                return (rejected + getattr(stats, "total_failures", 0)) / total
        return 0.0


class LatencyEvaluator:
    """canary_deployer.py:112-143: the canary's average service time against the baseline's average."""

    def __init__(self, max_latency: float = 1.0, threshold_multiplier: float = 1.5):
        self._max_latency = max_latency
        self._threshold_multiplier = threshold_multiplier

    def is_healthy(self, canary, baseline_backends: list) -> bool:
        return _against_baseline(self._get_avg_latency(canary), [self._get_avg_latency(b) for b in baseline_backends],
                                 self._max_latency, self._threshold_multiplier)

    def _get_avg_latency(self, backend) -> float:
        return backend.average_service_time if hasattr(backend, "average_service_time") else 0.0


METRIC_EVALUATORS = (ErrorRateEvaluator, LatencyEvaluator)


@dataclass(frozen=True)
class CanaryDeployerStats:
    """canary_deployer.py:146-156."""

    deployments_started: int = 0
    deployments_completed: int = 0
    deployments_rolled_back: int = 0
    stages_completed: int = 0
    evaluations_performed: int = 0
    evaluations_passed: int = 0
    evaluations_failed: int = 0


class CanaryDeployer(Entity):
    """One new instance `{name}_canary` joins a LoadBalancer and takes a growing share of its traffic stage by stage -- the strategy's
    weights are rewritten at every stage --, watched by a metric evaluator every `evaluation_interval` seconds; the last stage ends in
    a promotion (the baseline leaves), a failed evaluation in a rollback (components/deployment/canary_deployer.py:159-494).  The
    handlers run on the device (csrc/hs_graph.hip kEvCnStart ..); the factory is called once, when the graph is lowered, and the canary
    stands as a dormant Server behind all of the Simulation's own nodes until the deployment starts."""

    DEFAULT_STAGES = [CanaryStage(0.01, 30.0), CanaryStage(0.05, 30.0), CanaryStage(0.25, 30.0), CanaryStage(1.0, 30.0)]
    MAX_STAGES = 16                  # include/hs_engine.h HS_CANARY_MAX_STAGES

    def __init__(self, name: str, load_balancer: LoadBalancer, server_factory, stages=None, metric_evaluator=None,
                 evaluation_interval: float = 5.0):
        super().__init__(name)
        self._load_balancer = load_balancer
        self._server_factory = server_factory
        self._stages = stages or list(self.DEFAULT_STAGES)
        self._metric_evaluator = metric_evaluator or ErrorRateEvaluator()
        self._evaluation_interval = evaluation_interval
        self._canary: Entity | None = None
        self._baseline_backends: list[Entity] = []
        self._stage_start_time: Instant | None = None
        self._original_strategy = None
        self._deployments_started = 0
        self._deployments_completed = 0
        self._deployments_rolled_back = 0
        self._stages_completed = 0
        self._evaluations_performed = 0
        self._evaluations_passed = 0
        self._evaluations_failed = 0
        self.state = CanaryState()
        self._sim_start: Instant | None = None           # the clock a Simulation hands to its entities: `now` before run() is its start
        self._pool: list[Entity] = []                    # the factory's one result, made when a graph is lowered

    def downstream_entities(self) -> list[Entity]:
        return [self._load_balancer] + ([self._canary] if self._canary is not None else []) + list(self._baseline_backends)

    @property
    def stats(self) -> CanaryDeployerStats:
        return CanaryDeployerStats(self._deployments_started, self._deployments_completed, self._deployments_rolled_back,
                                   self._stages_completed, self._evaluations_performed, self._evaluations_passed,
                                   self._evaluations_failed)

    @property
    def canary(self):
        return self._canary

    @property
    def load_balancer(self) -> LoadBalancer:
        return self._load_balancer

    def deploy(self):
        """canary_deployer.py:252-263: the `_canary_deploy_start` Event for `sim.schedule(...)`, no daemon; its time is the Simulation's
        start once the deployer is one of its entities, Instant.Epoch before.  The caller may set another time.  One per deployer."""
        from .core.event import Event

        return Event(time=self._sim_start if self._sim_start is not None else Instant.Epoch, event_type="_canary_deploy_start",
                     target=self, context={})

    def _instance(self, k: int = 1) -> Entity:
        """The canary instance, from the factory the first time it is asked for."""
        if not self._pool:
            self._pool.append(self._server_factory(f"{self.name}_canary"))
        return self._pool[0]


# ---- probes --------------------------------------------------------------------------------------
class Data:
    """Time-series container of a Probe (instrumentation/data.py:20-110): `values` = [(time_s, value), ...]."""

    def __init__(self) -> None:
        self._tt = np.zeros(0, np.int64)
        self._vv = np.zeros(0, np.int64)
        self._scale = None           # utilisation: value / concurrency
        self._lazy = None            # () -> (t_ns, v): the samples are still on the device (lowering.write_back_plain_probes)

    def _set(self, t_ns: np.ndarray, v: np.ndarray, scale=None) -> None:
        self._tt, self._vv, self._scale, self._lazy = t_ns, v, scale, None

    def _set_lazy(self, fetch, scale=None) -> None:
        self._lazy, self._scale = fetch, scale

    def _load(self) -> None:
        if self._lazy is not None:
            fetch, self._lazy = self._lazy, None
            self._tt, self._vv = fetch()

    @property
    def _t_ns(self) -> np.ndarray:
        self._load()
        return self._tt

    @property
    def _v(self) -> np.ndarray:
        self._load()
        return self._vv

    def _val(self, v):
        if self._scale is None:
            return int(v)
        return self._scale(int(v)) if callable(self._scale) else int(v) / self._scale

    @property
    def values(self) -> list:
        return [(float(t) / 1_000_000_000, self._val(v)) for t, v in zip(self._t_ns.tolist(), self._v.tolist())]

    def times(self) -> list:
        return [float(t) / 1_000_000_000 for t in self._t_ns.tolist()]

    def raw_values(self) -> list:
        return [self._val(v) for v in self._v.tolist()]

    def count(self) -> int:
        return int(len(self._v))

    def mean(self) -> float:
        vals = self.raw_values()
        return sum(vals) / len(vals) if vals else 0.0

    def min(self) -> float:
        vals = self.raw_values()
        return min(vals) if vals else 0.0

    def max(self) -> float:
        vals = self.raw_values()
        return max(vals) if vals else 0.0

    def __len__(self) -> int:
        return self.count()


class Probe(Entity):
    """Periodic metric sampler (instrumentation/probe.py:81-164): a daemon Source that reads `getattr(target, metric)`
    every `interval` seconds into a Data container.  Lowered metrics: Server.depth / active_requests / utilization / available_capacity / has_capacity /
    stats_accepted / stats_dropped / requests completed, Sink.events_received, Source.generated_count, RateLimitedEntity.queue_depth,
    Bulkhead.active_count / queue_depth / available_permits, TimeoutWrapper.in_flight_count, Client.in_flight_count,
    BatchProcessor.buffer_depth, ConveyorBelt.items_in_transit, GateController.queue_depth, PooledCycleResource.available / active /
    queued, InventoryBuffer.stock."""

    _LOWERED = {"depth", "active_requests", "utilization", "available_capacity", "has_capacity", "stats_accepted", "stats_dropped",
                "requests_completed", "_requests_completed", "events_received", "generated_count", "_generated_count", "queue_depth",
                "active_count", "available_permits", "in_flight_count", "buffer_depth", "items_in_transit", "current_count",
                "available", "active", "queued", "stock"}
    _ON_WRAPPER = {"active_count": Bulkhead, "available_permits": Bulkhead, "in_flight_count": (TimeoutWrapper, Client, Hedge),
                   "buffer_depth": BatchProcessor, "items_in_transit": ConveyorBelt, "current_count": AutoScaler,
                   "available": PooledCycleResource, "active": PooledCycleResource, "queued": PooledCycleResource, "stock": InventoryBuffer}
    # Server attributes that are functions of `active_requests` and the (fixed) concurrency: the engine samples the integer,
    # the Data container applies the reference's expression (components/server/server.py:153-173,191-200, concurrency.py:117-131)
    _ON_ACTIVE = ("utilization", "available_capacity", "has_capacity")

    @classmethod
    def engine_metric(cls, metric: str) -> str:
        """The counter the engine samples for `metric`."""
        return "active_requests" if metric in cls._ON_ACTIVE else "generated_count" if metric == "_generated_count" else metric

    @classmethod
    def value_map(cls, metric: str, server):
        """What `Data` does with a sampled integer: None = keep, a number = divide by it, a callable = apply it."""
        if metric not in cls._ON_ACTIVE:
            return None
        c = int(server.concurrency)
        if metric == "utilization":
            return c                                        # active / limit
        if metric == "available_capacity":
            return lambda active: c - active                # FixedConcurrency.available
        return lambda active: active < c                    # has_capacity(): a callable attribute, the probe calls it (probe.py:52-55)

    def __init__(self, target: Entity, metric: str, data: Data, interval: float = 1.0, start_time: Instant | None = None):
        if interval <= 0:
            raise ValueError("Probe interval must be positive.")                  # probe.py:29-30
        if (metric not in self._LOWERED or (metric == "queue_depth" and not isinstance(target, (RateLimitedEntity, Bulkhead, GateController)))
                or (metric in self._ON_WRAPPER and not isinstance(target, self._ON_WRAPPER[metric]))):
            raise NotImplementedError(f"probe metric '{metric}' is an arbitrary attribute; lowered: {sorted(self._LOWERED)}")
        super().__init__(f"Probe_{target.name}_{metric}")
        self.target = target
        self.metric = metric
        self.data_sink = data
        self.interval = float(interval)
        # `start_time` only seeds the arrival-time provider, and Source.start() overwrites that with the Simulation's start time
        # before the first tick is drawn (load/source.py:120-127): the reference samples at start + k * interval whatever it is
        # (tests/test_oracle_live_reference.py::test_live_reference_ignores_a_probe_start_time)
        self.start_time = start_time if start_time is not None else Instant.Epoch

    @classmethod
    def on(cls, target: Entity, metric: str, interval: float = 1.0):
        data = Data()
        return cls(target=target, metric=metric, data=data, interval=interval), data

    @classmethod
    def on_many(cls, target: Entity, metrics: list, interval: float = 1.0):
        probes, data = [], {}
        for m in metrics:
            p, d = cls.on(target, m, interval=interval)
            probes.append(p)
            data[m] = d
        return probes, data
