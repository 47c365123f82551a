"""Host side of the mixed-family graphs (no GPU): every spec of tests/mixed_specs.py has a recording (tests/golden/live_mixed/) and
lowers on the host, and the recordings cover what the family is there for.  The coverage conditions are computed from the
recordings alone: they are conditions on what the live reference did, not on the engine."""
import itertools

import numpy as np
import pytest

import family_checks as FC
import happy_simulator_amd as hs
import mixed_specs as MX
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, split_parts

MR = MX.MIXED


@pytest.fixture(scope="module")
def recordings():
    return [(spec, MR.get("case", spec)) for spec in MX.all_specs()]


def test_every_spec_has_a_recording_and_lowers_on_the_host():
    names = [s["name"] for s in MX.recorded_specs()]
    assert len(names) == len(set(names)) and len(MX.FIXTURES) >= 24 and MX.N_RANDOM >= 150 and len(MX.TRACED) >= 8
    kinds = {"batch": N.NODE_BATCH_PROCESSOR, "conveyor": N.NODE_CONVEYOR, "gate": N.NODE_GATE}
    for spec in MX.recorded_specs():
        ref = MR.get("case", spec)
        assert ref["total_events"] <= 40_000 and len(ref["by_kind"]) == 39, spec["name"]
        assert spec.get("auto") or spec["end_s"] <= 20.0
        sim, pools = MX.build(spec)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph) and bool(g.arrays.has_flows) == bool(spec["flows"]), spec["name"]
        assert bool(g.arrays.has_clients) == bool(spec["clients"]) and bool(g.arrays.has_wrappers) == bool(spec["wrappers"])
        assert bool(g.arrays.has_health) == bool(spec.get("checkers"))
        for fl, ent in zip(spec["flows"], pools["flow"]):
            assert g.arrays.kind[g.node_of[id(ent)]] == kinds[fl["kind"]]
        sim._general_prepare(g, bool(spec.get("auto")))
    for name in MX.TRACED:
        assert len(MR.get("case", MX.FIXTURES[name])["trace"]) > 0


def test_every_case_but_the_groups_is_one_connected_graph():
    for spec in MX.all_specs() + [make() for make in MX.GROWTH]:
        sim, _pools = MX.build(spec)
        assert split_parts(sim.lowered().arrays) is None, spec["name"]        # (None: one component)
    for spec, n in [(MX.groups_spec(32), 32)] + [(s, 2) for s in MX.wide_groups_specs()]:
        sim, _pools = MX.build(spec)
        assert len(split_parts(sim.lowered().arrays)) == n


def test_what_the_issue_says_holds_in_the_recordings():
    get = lambda name: MR.get("case", MX.FIXTURES[name])  # noqa: E731
    r = get("gate_flush_into_a_client_fixed_retry")
    assert r["total_events"] == 304 and r["by_kind"][28:31].tolist() == [25, 25, 25] and r["by_kind"][36:].tolist() == [30, 2, 2]
    assert r["flow_stats"].tolist() == [[25, 20, 0, 2, 0, 5]] and r["events_cancelled"] == 0
    r = get("gate_flush_into_a_small_bulkhead")
    assert r["total_events"] == 161 and r["by_kind"][22:25].tolist() == [15, 10, 3] and r["by_kind"][36:].tolist() == [30, 1, 1]
    assert r["flow_stats"].tolist() == [[15, 25, 0, 1, 0, 15]] and r["events_cancelled"] == 0
    r = get("client_server_batch_processor")
    assert r["total_events"] == 501 and r["by_kind"][28:31].tolist() == [41, 41, 39] and r["by_kind"][31:34].tolist() == [38, 4, 11]
    assert r["flow_stats"][0, :4].tolist() == [11, 38, 4, 0] and r["events_cancelled"] == 7
    r = get("batch_into_a_timeout_wrapper_link_server")
    assert r["total_events"] == 613 and r["by_kind"][25:28].tolist() == [43, 78, 39] and r["by_kind"][31:34].tolist() == [44, 3, 10]
    assert r["flow_stats"][0, :4].tolist() == [10, 43, 3, 1] and r["events_cancelled"] == 7
    # the flush of ten lands on the Client on ONE nanosecond, and every Request of it shares the keys (None, attempt)
    r = get("gate_flush_into_a_client_fixed_retry")
    open_t = r["trace"][r["trace"][:, 1] == 37][0, 0]
    assert int(((r["trace"][:, 1] == 28) & (r["trace"][:, 0] == open_t)).sum()) == 10 and r["cl_stats"][0, 6] == 0
    # the Bulkhead's 2 permits and 3 queue places are smaller than the flush of 10
    r = get("gate_flush_into_a_small_bulkhead")
    assert r["wrap_stats"][0, 2] >= 5 and r["wrap_stats"][0, 4] >= 3
    # probes of a checker were dropped by the bounded queue that the Client's Requests fill
    r = get("client_target_is_a_checked_bounded_backend")
    assert r["dropped"][0] > 0 and r["by_kind"][19:22].all() and r["by_kind"][28:31].all() and r["probe_drops"] > 0
    # the second Client reads the first one's attempt off the forwarded context: it counts retries though none of its 31 timeouts may be
    # retried more than once, fails at the first timeout of an attempt >= 2 and is left with a key of attempt 2 that it never sent twice
    r = get("retries_of_one_client_reach_a_second_with_fewer_attempts")
    assert r["cl_stats"][1].tolist() == [35, 1, 31, 20, 18, 1, 0] and r["cl_keys"].tolist() == [[0, 2]] and r["cl_stats"][0, 3] == 13
    # events_cancelled from more than one origin
    r = get("cancelled_events_of_three_origins")
    assert r["events_cancelled"] > r["flow_stats"][0, 0] - r["flow_stats"][0, 2]
    r = get("auto_terminating_run_with_three_daemon_families")
    assert r["pending_events"] > 0 and r["by_kind"][16] > 0 and r["by_kind"][37] > 0 and r["checker_stats"][0, 6] == 0
    for make in MX.GROWTH:
        assert MR.get("case", make())["total_events"] > 2000
    assert MR.get("case", MX.big_flush_spec())["wrap_stats"][0, :3].tolist() == [1100, 40, 1056]          # 4 permits, 40 queue places
    r = MR.get("case", MX.retry_storm_spec())
    assert r["cl_stats"][0, 2] >= 1000 and r["cl_stats"][0, 3] >= 800 and r["cl_stats"][0, 4] >= 150      # timeouts, retries, failures


# ---- coverage, from the recordings alone ------------------------------------------------------------------------------------------------
def test_every_kind_of_the_five_families_and_the_faults_is_processed_often(recordings):
    used = np.zeros(39, np.int64)
    for _spec, ref in recordings:
        used += ref["by_kind"]
    assert (used[15:] >= 50).all(), used[15:].tolist()


def test_every_pair_of_families_meets_in_eight_cases(recordings):
    pairs = {p: 0 for p in itertools.combinations(MX.FAMILIES, 2)}
    three = 0
    for _spec, ref in recordings:
        fams = MX.families_of(ref)
        for p in pairs:
            pairs[p] += set(p) <= fams
        three += len(fams) >= 3
    assert len(pairs) == 10 and all(n >= 8 for n in pairs.values()), pairs
    assert three >= 30, three


def test_faults_and_cancelled_events_meet_the_mix(recordings):
    faulted = sum(1 for _s, ref in recordings if ref["fault_events"] > 0 and len(MX.families_of(ref)) >= 2)
    cancelled = sum(1 for _s, ref in recordings if ref["events_cancelled"] > 0)
    assert faulted >= 15 and cancelled >= 10, (faulted, cancelled)


def test_events_before_the_start_are_skipped_in_ten_cases(recordings):
    """The reference pops and skips an Event that lies before the Simulation's start (it counts in no kind): gate Events and fault
    Events with absolute times and an early `checker.start()` under a later start_time."""
    travelled = [spec["name"] for spec, ref in recordings if ref["time_travel"] > 0]
    assert len(travelled) >= 10, travelled
    assert all(spec.get("start_ns") for spec, ref in recordings if ref["time_travel"] > 0)
    r = MR.get("case", MX.FIXTURES["gate_events_and_an_early_checker_before_a_later_start_time"])
    assert r["time_travel"] == 2 and not r["by_kind"][19:22].any() and r["by_kind"][37:].tolist() == [1, 2]


def _families_on_one_nanosecond(spec, ref):
    """Two Events of different families on one nanosecond of the case's trace."""
    trace = ref.get("trace")
    if trace is None:
        return False
    fam = np.full(39, -1)
    for i, f in enumerate(MX.FAMILIES):
        lo, hi = MX.FAMILY_KINDS[f]
        fam[lo:hi] = i
    rows = trace[fam[trace[:, 1]] >= 0]
    seen = {}
    for t, k in zip(rows[:, 0].tolist(), fam[rows[:, 1]].tolist()):
        seen.setdefault(t, set()).add(k)
    return any(len(v) >= 2 for v in seen.values())


def test_two_families_meet_on_one_nanosecond_in_twelve_traces(recordings):
    hits = [spec["name"] for spec, ref in recordings if _families_on_one_nanosecond(spec, ref)]
    assert len(hits) >= 12, hits


def test_the_groups_cross_the_node_window():
    """kLdsNodesBatch = 48 node rows of a side-by-side run stay in LDS: 49-node parts are beyond it, 48-node parts fill it."""
    src = open(N.__file__.replace("_native.py", "csrc/hs_graph.hip")).read()
    assert "kLdsNodesBatch = 48" in src
    for spec, want in zip(MX.wide_groups_specs(), (49, 48)):
        sim, _pools = MX.build(spec)
        parts = split_parts(sim.lowered().arrays)
        assert [len(ids) for ids, _pos, _b in parts] == [want, want]
    assert MX.FAMILIES == ("limiter", "health", "wrapper", "client", "flow")
    assert len(MX.families_of(MR.get("case", MX.groups_spec(32)))) == 4


def test_refused_shapes_are_refused_by_name():
    for name, (spec, text) in MX.REFUSED.items():
        sim, _pools = MX.build(spec)
        with pytest.raises(hs.UnsupportedTopology, match=text):
            sim.lowered()


def test_compare_sees_a_difference_in_a_mixed_case():
    """family_checks.compare on one mixed recording (tests/test_family_checks_host.py holds the full set of alterations)."""
    spec = MX.FIXTURES["probes_on_every_family"]
    ref = MR.get("case", spec)
    got = dict(ref, by_kind=ref["by_kind"][:15].copy())
    first = 15
    for key, end in MX.BY_KIND_SLICES[1:]:
        got[key] = ref["by_kind"][first:end].copy()
        first = end
    MX.compare(spec["name"], got, ref)
    with pytest.raises(AssertionError, match="flow_stats"):
        MX.compare(spec["name"], dict(got, flow_stats=got["flow_stats"] + 1), ref)
    assert FC.compare is not None and len(MX.families_of(ref)) == 4
