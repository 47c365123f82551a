"""Fault injection: mirrors of happysimulator/faults/ (`FaultSchedule`, `FaultHandle`, `FaultStats`, `CrashNode`, `PauseNode`,
`InjectLatency`, `InjectPacketLoss`).

A node fault is two daemon Events constructed inside `Simulation.__init__` (faults/schedule.py:68-100, core/simulation.py:162-169)
that set and clear `entity._crashed`; `Event.invoke` (core/event.py:261) drops every Event aimed at an entity whose flag is set.
On the engine both are heap entries of the single-heap loop (csrc/hs_graph.hip kEvFaultOn / kEvFaultOff) and the flag is a byte of
the node's row; this module only carries what the caller wrote down: names, times, and which handles were cancelled when.

A link fault (faults/network_faults.py:27-198) is two daemon Events as well, aimed at a callback entity of their own: at `start` the
link's latency becomes `_CompoundLatency(original, ConstantLatency(extra_ms / 1000))` (its packet_loss_rate `min(1.0, original +
loss_rate)`), at `end` the original comes back -- the original the fault read when Simulation.__init__ constructed it.  The link is
found through a `Network` of the Simulation (entities.Network: a registry).  On the engine the two are the same heap-entry kinds with
the fault's index riding along; which fault is active on a link is a word of the link's state (csrc/hs_graph.hip).
"""
from __future__ import annotations

from dataclasses import dataclass

from .core.event import Event
from .core.temporal import Instant
from .entities import ConstantLatency, Entity, Network, NetworkLink, _CompoundLatency

# what the reference's other faults act on has no mirror here (faults/network_faults.py:201-385: traffic routed by Network.handle_event;
# faults/resource_faults.py: Resource).  A class of another library that merely bears the name of a lowered link fault is refused too.
_ROUTED = "it acts only on traffic routed by Network.handle_event, which is not lowered"
_FOREIGN = "only this package's own class finds its link through a mirrored Network"
NOT_LOWERED = {"InjectLatency": _FOREIGN, "InjectPacketLoss": _FOREIGN, "NetworkPartition": _ROUTED, "RandomPartition": _ROUTED,
               "ReduceCapacity": "there is no Resource"}
LOWERED = "CrashNode, PauseNode, InjectLatency, InjectPacketLoss"


@dataclass(frozen=True)
class CrashNode:
    """faults/node_faults.py:23-78: `entity._crashed = True` at `at`, False again at `restart_at` (None: for good)."""

    entity_name: str
    at: float
    restart_at: float | None = None

    def _fault_events(self) -> list[tuple[str, float, bool]]:
        out = [("crash", self.at, True)]
        if self.restart_at is not None:
            out.append(("restart", self.restart_at, False))
        return out


@dataclass(frozen=True)
class PauseNode:
    """faults/node_faults.py:81-128: CrashNode under the names start / end."""

    entity_name: str
    start: float
    end: float

    def _fault_events(self) -> list[tuple[str, float, bool]]:
        return [("pause", self.start, True), ("resume", self.end, False)]


def _resolve_network(fault, networks: dict):
    """network_faults.py:117-122 / :193-198."""
    if fault.network_name is not None:
        return networks[fault.network_name]
    if not networks:
        raise ValueError("No networks registered in simulation")
    return next(iter(networks.values()))


@dataclass(frozen=True)
class InjectLatency:
    """faults/network_faults.py:47-122: `extra_ms` milliseconds on top of the link `source_name -> dest_name` from `start` to `end`."""

    source_name: str
    dest_name: str
    extra_ms: float
    start: float
    end: float
    network_name: str | None = None

    _what = "latency"


@dataclass(frozen=True)
class InjectPacketLoss:
    """faults/network_faults.py:125-198: `loss_rate` on top of the link's packet_loss_rate (at most 1.0) from `start` to `end`."""

    source_name: str
    dest_name: str
    loss_rate: float
    start: float
    end: float
    network_name: str | None = None

    _what = "loss"


class LinkFaultEvent:
    """One of the two Events of a link fault as Simulation.__init__ constructed it: the link, whether it activates, the value it sets
    (activate: the extra latency in seconds as the Duration the reference adds -- or the loss rate; deactivate: the original the fault
    read), the object it leaves on the link (`_CompoundLatency` / the float) and its fault's place among the schedule's faults."""

    __slots__ = ("link", "what", "on", "value", "leaves", "event", "index")

    def __init__(self, link, what, on, value, leaves, event, index):
        self.link, self.what, self.on, self.value, self.leaves, self.event, self.index = link, what, on, value, leaves, event, index


class FaultHandle:
    """faults/fault.py:60-87.  cancel() cancels the Events that EXIST: they come into being in Simulation.__init__, so a handle
    cancelled before that cancels nothing (and still reports `cancelled`)."""

    def __init__(self, fault) -> None:
        self.fault = fault
        self._events: list[Event] = []
        self._cancelled = False

    @property
    def cancelled(self) -> bool:
        return self._cancelled

    def cancel(self) -> None:
        if self._cancelled:
            return
        self._cancelled = True
        for event in self._events:
            event.cancel()


@dataclass(frozen=True)
class FaultStats:
    """faults/fault.py:90-104.  The reference never increments faults_activated / faults_deactivated."""

    faults_scheduled: int
    faults_activated: int
    faults_deactivated: int
    faults_cancelled: int


class FaultSchedule(Entity):
    """faults/schedule.py:31-135."""

    def __init__(self, name: str = "FaultSchedule") -> None:
        super().__init__(name)
        self._faults: list = []
        self._handles: list[FaultHandle] = []

    def add(self, fault) -> FaultHandle:
        handle = FaultHandle(fault)
        self._faults.append(fault)
        self._handles.append(handle)
        return handle

    @property
    def stats(self) -> FaultStats:
        return FaultStats(faults_scheduled=len(self._faults), faults_activated=0, faults_deactivated=0,
                          faults_cancelled=sum(1 for h in self._handles if h.cancelled))

    def handle_event(self, event) -> None:
        """FaultSchedule does not process events itself."""

    def _start(self, sim) -> list:
        """FaultSchedule.start: (entity, its Event, on) of the node faults and a LinkFaultEvent per Event of the link faults, in
        add() order, activation before deactivation.  Names resolve in dicts over entities + sources + probes (:112-135: the last
        object of a name wins); an unknown name is the dict's KeyError."""
        from .lowering import UnsupportedTopology

        components = list(sim._entities) + list(sim._sources) + list(sim._probes)
        entities = {c.name: c for c in components if isinstance(c, Entity)}
        networks = {c.name: c for c in components if isinstance(c, Network)}
        out = []
        for index, (fault, handle) in enumerate(zip(self._faults, self._handles)):
            if isinstance(fault, (InjectLatency, InjectPacketLoss)):
                handle._events = self._link_fault(fault, networks, out, index)
                continue
            if not isinstance(fault, (CrashNode, PauseNode)):
                kind = type(fault).__name__
                if kind in NOT_LOWERED:
                    raise UnsupportedTopology(f"fault {kind} is not lowered: {NOT_LOWERED[kind]} (lowered: {LOWERED})")
                raise UnsupportedTopology(f"fault {kind} is not lowered: its generate_events is host Python (lowered: {LOWERED})")
            if fault.entity_name not in entities:
                # an instance a deployer's or scaler's factory makes is no entity of the Simulation: say so (any other unknown name
                # is the dict's KeyError, as in the reference)
                for c in components:
                    pools = {"RollingDeployer": f"{c.name}_v2_", "CanaryDeployer": f"{c.name}_canary", "AutoScaler": f"{c.name}_server_"}
                    prefix = pools.get(type(c).__name__)
                    if prefix and fault.entity_name.startswith(prefix):
                        raise UnsupportedTopology(f"fault {type(fault).__name__} names '{fault.entity_name}', an instance of the pool of "
                                                  f"{type(c).__name__} '{c.name}': a pool instance is no entity of the Simulation and cannot "
                                                  "be named by a FaultSchedule (the reference cannot either; the fault may name "
                                                  f"'{c.name}' itself)")
            entity = entities[fault.entity_name]
            events = []
            for what, t_s, on in fault._fault_events():
                ev = Event(time=Instant.from_seconds(t_s), event_type=f"fault.{what}:{fault.entity_name}", target=entity, daemon=True)
                events.append(ev)
                out.append((entity, ev, on))
            handle._events = events
        return out

    @staticmethod
    def _link_fault(fault, networks: dict, out: list, index: int) -> list[Event]:
        """generate_events of a link fault (network_faults.py:70-115 / :148-191): the link and its original value are read now."""
        from .lowering import UnsupportedTopology

        kind = type(fault).__name__
        network = _resolve_network(fault, networks)
        link = network.get_link(fault.source_name, fault.dest_name)
        if link is None:
            raise ValueError(f"No link found: {fault.source_name} -> {fault.dest_name}")
        if not isinstance(link, NetworkLink):
            raise UnsupportedTopology(f"fault {kind}: '{getattr(link, 'name', link)}' is not a lowered NetworkLink")
        if link._reverse_of is not None:
            raise UnsupportedTopology(f"fault {kind}: link '{link.name}' is the reverse copy add_bidirectional_link made of "
                                      f"'{link._reverse_of.name}' -- it shares its jitter object and its loss stream with the forward link "
                                      "(not lowered)")
        if fault._what == "latency":
            if not (fault.extra_ms >= 0):
                raise UnsupportedTopology(f"fault {kind}: extra_ms = {fault.extra_ms!r} is negative or not a number (not lowered)")
            original = link.latency
            if not isinstance(original, ConstantLatency):
                raise UnsupportedTopology(f"link '{link.name}': the base latency must be a ConstantLatency >= 0")
            extra = ConstantLatency(fault.extra_ms / 1000.0)
            if not extra.mean < 4.0e9:
                raise UnsupportedTopology(f"fault {kind}: extra_ms = {fault.extra_ms!r} is beyond 4e9 s (not lowered)")
            on_value, on_leaves = extra.get_latency(None).to_seconds(), _CompoundLatency(original, extra)
        else:
            if not (0.0 <= fault.loss_rate <= 1.0):
                raise UnsupportedTopology(f"fault {kind}: loss_rate = {fault.loss_rate!r} is outside [0, 1] (not lowered)")
            original = link.packet_loss_rate
            on_value = on_leaves = min(1.0, original + fault.loss_rate)
        events = []
        off_value = original if fault._what == "loss" else 0.0
        for on, t_s, value, leaves in ((True, fault.start, on_value, on_leaves), (False, fault.end, off_value, original)):
            et = f"fault.{fault._what}.{'activate' if on else 'deactivate'}:{fault.source_name}->{fault.dest_name}"
            ev = Event(time=Instant.from_seconds(t_s), event_type=et, target=Entity(f"once:{et}"), daemon=True)   # (Event.once: a callback entity)
            events.append(ev)
            out.append(LinkFaultEvent(link, fault._what, on, value, leaves, ev, index))
        return events
