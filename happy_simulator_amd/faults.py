"""Fault injection: mirrors of happysimulator/faults/ (`FaultSchedule`, `FaultHandle`, `FaultStats`, `CrashNode`, `PauseNode`).

A node fault is two daemon Events constructed inside `Simulation.__init__` (faults/schedule.py:68-100, core/simulation.py:162-169)
that set and clear `entity._crashed`; `Event.invoke` (core/event.py:261) drops every Event aimed at an entity whose flag is set.
On the engine both are heap entries of the single-heap loop (csrc/hs_graph.hip kEvFaultOn / kEvFaultOff) and the flag is a byte of
the node's row; this module only carries what the caller wrote down: names, times, and which handles were cancelled when.
"""
from __future__ import annotations

from dataclasses import dataclass

from .core.event import Event
from .core.temporal import Instant
from .entities import Entity

# what the reference's other faults act on has no mirror here (faults/network_faults.py: the Network entity;
# faults/resource_faults.py: Resource)
NOT_LOWERED = {"InjectLatency": "the Network entity is not mirrored", "InjectPacketLoss": "the Network entity is not mirrored",
               "NetworkPartition": "the Network entity is not mirrored", "RandomPartition": "the Network entity is not mirrored",
               "ReduceCapacity": "there is no Resource"}


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

    def _start(self, sim) -> list[tuple[Entity, Event, bool]]:
        """FaultSchedule.start for the node faults: (entity, its Event, on) in add() order, crash before restart.  Names resolve in
        a dict over entities + sources + probes (:112-135: the last object of a name wins); an unknown name is the dict's KeyError."""
        from .lowering import UnsupportedTopology

        entities = {c.name: c for c in list(sim._entities) + list(sim._sources) + list(sim._probes) if isinstance(c, Entity)}
        out = []
        for fault, handle in zip(self._faults, self._handles):
            if not isinstance(fault, (CrashNode, PauseNode)):
                kind = type(fault).__name__
                if kind in NOT_LOWERED:
                    raise UnsupportedTopology(f"fault {kind} is not lowered: {NOT_LOWERED[kind]} (lowered: CrashNode, PauseNode)")
                raise UnsupportedTopology(f"fault {kind} is not lowered: its generate_events is host Python (lowered: CrashNode, PauseNode)")
            entity = entities[fault.entity_name]
            events = []
            for what, t_s, on in fault._fault_events():
                ev = Event(time=Instant.from_seconds(t_s), event_type=f"fault.{what}:{fault.entity_name}", target=entity, daemon=True)
                events.append(ev)
                out.append((entity, ev, on))
            handle._events = events
        return out
