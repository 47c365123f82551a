"""Host side of fault injection (no GPU): the mirrors of FaultSchedule / FaultHandle / FaultStats / CrashNode / PauseNode against the
recorded live reference (tests/golden/live_faults/), name resolution at construction, the named refusals, and what the lowering
hands to the single-heap loop."""
import dataclasses
import os
import re

import numpy as np
import pytest

import fault_specs as FS
import graph_family as GF
import happy_simulator_amd as hs
import rate_limiter_specs as RS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph
from recorded import FAULTS as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(fs=None, **kw):
    sink, hidden = hs.Sink("sink"), hs.Sink("hidden")
    srv = hs.Server("srv", service_time=hs.ExponentialLatency(0.05), downstream=sink)
    src = hs.Source.constant(rate=1, target=srv, name="src")
    return hs.Simulation(end_time=hs.Instant.from_seconds(1), sources=[src], entities=[srv, sink], fault_schedule=fs, **kw), (src, srv, sink, hidden)


def test_mirrors_equal_the_recorded_defaults():
    ref = FR.get("defaults")
    c, p = hs.CrashNode("a", at=1.0), hs.PauseNode("b", start=1.0, end=2.0)
    assert [c.entity_name, c.at, c.restart_at] == ref["crash"]["fields"] and repr(c) == ref["crash"]["repr"]
    assert (c == hs.CrashNode("a", 1.0, None)) == ref["crash"]["eq"]
    assert [p.entity_name, p.start, p.end] == ref["pause"]["fields"] and repr(p) == ref["pause"]["repr"]
    for key, obj, attr in (("crash", c, "at"), ("pause", p, "start")):
        with pytest.raises(dataclasses.FrozenInstanceError) as e:
            setattr(obj, attr, 5.0)
        assert type(e.value).__name__ == ref[key]["frozen"]
    fs = hs.FaultSchedule()
    h = fs.add(c)
    fs.add(p)
    st = fs.stats
    want = ref["schedule"]
    assert isinstance(fs, hs.Entity) and fs.name == want["name"] == "FaultSchedule" and hs.FaultSchedule("chaos").name == want["named"]
    assert type(st).__name__ == want["stats_type"] == "FaultStats"
    assert [st.faults_scheduled, st.faults_activated, st.faults_deactivated, st.faults_cancelled] == want["stats"]
    assert (h.fault is c) == want["handle_fault_is"] and h.cancelled == want["handle_cancelled"] and len(h._events) == want["handle_events"]
    h.cancel()
    h.cancel()
    st = fs.stats
    assert [st.faults_scheduled, st.faults_activated, st.faults_deactivated, st.faults_cancelled] == want["stats_after_cancel"]
    assert h.cancelled == want["handle_cancelled_after"]
    with pytest.raises(dataclasses.FrozenInstanceError) as e:
        st.faults_scheduled = 3
    assert type(e.value).__name__ == want["stats_frozen"]


def test_names_resolve_at_construction_like_the_reference():
    ref = FR.get("defaults")["key_errors"]
    for label, name in (("unknown", "nobody"), ("unlisted", "hidden")):
        fs = hs.FaultSchedule()
        fs.add(hs.CrashNode(name, at=1.0))
        with pytest.raises(KeyError) as e:
            _chain(fs)
        assert [type(e.value).__name__, str(e.value)] == ref[label]


def test_fault_events_come_into_being_with_the_simulation():
    ref = FR.get("defaults")["events"]
    fs = hs.FaultSchedule()
    h3 = fs.add(hs.CrashNode("srv", at=1.0, restart_at=2.0))
    h4 = fs.add(hs.CrashNode("sink", at=1.5))
    assert h3._events == [] and h4._events == []
    sim, (src, srv, sink, _hidden) = _chain(fs)
    evs = h3._events + h4._events
    assert [e.event_type for e in evs] == ref["types"] and [e.daemon for e in evs] == ref["daemon"]
    assert [e.time.nanoseconds for e in evs] == ref["times_ns"]
    # behind the Source's first tick, in add() order, crash before restart: the next values of the process-wide counter
    assert ref["sort_index"] == [1, 2, 3]
    g = sim.lowered()
    assert isinstance(g, GeneralGraph) and "fault" in sim._station_refusal
    assert sim._general_faults(g) == [(g.node_of[id(srv)], 10 ** 9, True, False), (g.node_of[id(srv)], 2 * 10 ** 9, False, False),
                                      (g.node_of[id(sink)], 1_500_000_000, True, False)]
    h3.cancel()                                            # between construction and run(): the Events exist and are cancelled
    assert [c for _n, _t, _on, c in sim._general_faults(g)] == [True, True, False]


def test_a_handle_cancelled_before_construction_cancels_nothing():
    fs = hs.FaultSchedule()
    h = fs.add(hs.PauseNode("srv", 0.2, 0.4))
    h.cancel()
    sim, _ = _chain(fs)
    assert fs.stats.faults_cancelled == 1 and h.cancelled
    assert [c for _n, _t, _on, c in sim._general_faults(sim.lowered())] == [False, False]


def test_an_empty_schedule_behaves_as_none():
    sim, _ = _chain(hs.FaultSchedule())
    g = sim.lowered()
    assert not isinstance(g, GeneralGraph) and not hasattr(sim, "_station_refusal")
    none_sim, _ = _chain(None)
    assert type(none_sim.lowered()) is type(g)


def test_a_duplicate_name_resolves_to_the_last_object():
    spec = FS.FIXTURES["duplicate_name"]
    sim, pools = GF.build(spec)
    g = sim.lowered()
    assert pools["server"][0].name == pools["server"][1].name == "srv0"
    assert {n for n, _t, _on, _c in sim._general_faults(g)} == {g.node_of[id(pools["server"][1])]}


class _Named:
    def __init__(self, *a, **k):
        pass

    def generate_events(self, ctx):
        return []


@pytest.mark.parametrize("kind,why", [("InjectLatency", "Network"), ("InjectPacketLoss", "Network"), ("NetworkPartition", "Network"),
                                      ("RandomPartition", "Network"), ("ReduceCapacity", "Resource"), ("MyOwnFault", "host Python")])
def test_other_faults_are_refused_by_name(kind, why):
    fs = hs.FaultSchedule()
    fs.add(type(kind, (_Named,), {})())
    with pytest.raises(hs.UnsupportedTopology, match=rf"fault {kind} is not lowered.*{why}"):
        _chain(fs)


def test_refusals_around_the_schedule():
    with pytest.raises(hs.UnsupportedTopology, match="not a lowered FaultSchedule"):
        _chain(object())
    fs = hs.FaultSchedule()
    fs.add(hs.CrashNode("srv", at=0.5))
    sink = hs.Sink("sink")
    srv = hs.Server("srv", service_time=hs.ExponentialLatency(0.05), downstream=sink)
    part = hs.SimulationPartition(name="p0", entities=[srv, sink], sources=[hs.Source.poisson(rate=8, target=srv, name="src")], fault_schedule=fs)
    with pytest.raises(hs.UnsupportedTopology, match="fault schedule on a ParallelSimulation partition"):
        hs.ParallelSimulation([part], end_time=hs.Instant.from_seconds(1))
    assert hs.SimulationPartition(name="p1").fault_schedule is None


def test_every_spec_lowers_to_the_single_heap_loop():
    """What the recorder asserted when it ran: the product takes every fixture and every random graph; the fault Events name nodes of
    every entity kind."""
    kinds = set()
    for spec in FS.all_specs():
        sim, _pools = GF.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph), spec["name"]
        faults = sim._general_faults(g)
        assert len(faults) >= len(spec["faults"]) >= 1
        kinds.update(int(g.arrays.kind[n]) for n, _t, _on, _c in faults)
    assert kinds == {N.NODE_SOURCE, N.NODE_SERVER, N.NODE_SINK, N.NODE_LINK, N.NODE_ROUTER, N.NODE_PROBE, N.NODE_LB, N.NODE_RATE_LIMITER}


def test_new_header_symbols_are_exported():
    N.build()
    lib = N.lib()
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    for sym in ("hs_graph_add_fault", "hs_graph_get_faults"):
        assert sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"^int {sym}\(", hdr, re.M), sym
    assert N.ABI_VERSION == 16 and re.search(r"#define HS_ABI_VERSION 16\b", hdr) and N.EV_KINDS == 15
    assert lib.hs_graph_add_fault(None, 0, 0, 1, 0) == N.HS_E_INVALID and lib.hs_graph_get_faults(None, None, None, None) == N.HS_E_INVALID


def test_the_recordings_hold_what_the_issue_observed():
    get = lambda name: FR.get("case", FS.FIXTURES[name])  # noqa: E731
    r = get("cancelled_before_construction")
    assert r["fault_stats"].tolist() == [1, 0, 0, 1] and r["fault_events"] == 2 and r["events_cancelled"] == 0
    r = get("cancelled_after_construction")
    assert r["fault_stats"].tolist() == [2, 0, 0, 1] and r["events_cancelled"] == 2
    assert get("fault_before_start")["time_travel"] == 1
    r = get("fault_is_the_event_beyond_the_end")
    assert r["final_ns"] == 3_000_010_000 and r["crashed"].tolist() == [0, 1, 0]
    assert get("fault_later_than_the_event_beyond_the_end")["fault_events"] == 0
    r = get("auto_terminate_pending_restart")
    assert r["pending_events"] == 1 and r["crashed"].tolist() == [1, 0]
    r = get("source_crash_restart")                       # restarted at 4 s, and never generates again
    assert r["crashed"].sum() == 0 and r["sink_t_ns"].max() < 4 * 10 ** 9
    assert r["generated"].tolist() == [15] and r["by_kind"][0] == 16       # the one pending tick was popped, counted and dropped
    assert get("overlapping_crash_and_pause")["crashed"].sum() == 0
    for k in RS.POLICIES:
        r = get(f"limiter_{k}_crash")
        assert r["lim_stats"][0, 5] == 1 and r["lim_stats"][0, 4] > 0
    # every fault_stats row: activated / deactivated are never incremented
    assert all(FR.get("case", s)["fault_stats"][1:3].tolist() == [0, 0] for s in FS.all_specs())
    assert sorted(os.path.getsize(os.path.join(FR.rec_dir, f)) for f in os.listdir(FR.rec_dir))[-1] <= FR.max_part_bytes
    assert np.all([len(FR.get("case", FS.FIXTURES[n])["trace"]) > 100 for n in FS.TRACED])
