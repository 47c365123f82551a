"""Host side of the queue policies (no GPU): the three classes against the reference's recorded defaults, the lowering of every spec
of tests/queue_specs.py, the refusals by name, and what the recordings (tests/golden/live_queues/) cover.  The coverage conditions
are computed from the recordings alone: they are conditions on what the live reference did, not on the engine."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import happy_simulator_amd as hs
import queue_specs as QS
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, split_parts
from happy_simulator_amd.lowering import UnsupportedTopology as UT

QR = QS.QUEUES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(policy, n=1, **server_kw):
    sink = hs.Sink("sink")
    servers = [hs.Server(f"srv{i}", service_time=hs.ExponentialLatency(0.05), queue_policy=policy if i == 0 else None, downstream=sink, **server_kw)
               for i in range(n)]
    sources = [hs.Source.poisson(rate=20.0, target=sv, name=f"src{i}") for i, sv in enumerate(servers)]
    return hs.Simulation(sources=sources, entities=servers + [sink], end_time=hs.Instant.from_seconds(1.0)), servers


def test_mirrors_equal_the_recorded_defaults_and_errors():
    ref = QR.get("defaults")
    got = QS.policy_defaults(hs)
    assert set(got) == set(ref)
    for key in ref:
        assert got[key] == ref[key], (key, got[key], ref[key])
    inf = float("inf")
    assert ref["lifo"] == [inf, 3, 0, 0, True] and ref["alifo"][:9] == [4, inf, 5, 1, False, "FIFO", 0, True, False]
    assert ref["codel"][:7] == [0.005, 0.1, inf, 0.01, 0.2, 7, False] and ref["codel"][14] == 2
    assert ref["errors"] == ["congestion_threshold must be >= 1, got 0", "congestion_threshold must be >= 1, got -2", "capacity must be >= 1 or None, got 0",
                             "capacity must be >= 1 or None, got -1", "target_delay must be > 0, got 0", "target_delay must be > 0, got -0.5",
                             "interval must be > 0, got 0", "interval must be > 0, got -1.0", "capacity must be >= 1 or None, got 0",
                             "target_delay must be > 0, got 0", "congestion_threshold must be >= 1, got 0", None, None]
    assert ref["stats_types"] == ["AdaptiveLIFOStats", "CoDelStats"] and ref["stats_frozen"] == ["FrozenInstanceError"] * 2
    assert ref["stats_fields"] == [["enqueued", "dequeued_fifo", "dequeued_lifo", "capacity_rejected", "mode_switches"],
                                   ["enqueued", "dequeued", "dropped", "capacity_rejected", "drop_intervals"]]
    assert hs.AdaptiveLIFOStats() == hs.AdaptiveLIFOStats(0, 0, 0, 0, 0) and hs.CoDelStats(1, 2, 3).dropped == 3


def test_a_server_takes_the_three_policies_and_ignores_queue_capacity_next_to_one():
    for pol in (hs.LIFOQueue(), hs.AdaptiveLIFO(3, 9), hs.CoDelQueue(capacity=4)):
        sv = hs.Server("s", queue_policy=pol, queue_capacity=2)
        assert sv.queue_policy is pol and sv.depth == 0 == len(pol)
    assert hs.Server("s", queue_policy=hs.LIFOQueue(), queue_capacity=2).queue_policy.capacity == float("inf")
    assert hs.Server("s", queue_capacity=2).queue_policy.capacity == 2 and type(hs.Server("s").queue_policy) is hs.FIFOQueue


def test_every_spec_has_a_recording_and_lowers_with_has_queue_policies():
    names = [s["name"] for s in QS.recorded_specs()]
    assert len(names) == len(set(names)) and len(QS.FIXTURES) >= 36 and QS.N_RANDOM >= 120 and len(QS.TRACED) >= 6
    codes = {"lifo": N.QUEUE_LIFO, "alifo": N.QUEUE_ADAPTIVE_LIFO, "codel": N.QUEUE_CODEL}
    seen = set()
    for spec in QS.recorded_specs():
        ref = QR.get("case", spec)
        assert ref["total_events"] <= 40_000 and len(ref["by_kind"]) == 39, spec["name"]       # (no new Event kinds)
        assert spec.get("auto") or spec["end_s"] <= 20.0
        sim, pools = QS.build(spec)
        g = sim.lowered()
        policied = [(i, sv["qp"]) for i, sv in enumerate(spec["servers"]) if sv.get("qp")]
        assert isinstance(g, GeneralGraph) and bool(g.arrays.has_queue_policies) == bool(policied), spec["name"]
        assert ref["q_state"][:, 0].tolist() == [i for i, _ in policied]
        for i, qp in policied:
            row = g.arrays.qp_params[g.node_of[id(pools["server"][i])]]
            assert row[0] == codes[qp[0]] and row[1] == (-1 if qp[1] is None else qp[1]), (spec["name"], i, row)
            assert (row[2] == qp[2] if qp[0] == "alifo" else row[2] == 0) and (row[3:].tolist() == [float(qp[2]), float(qp[3])] if qp[0] == "codel" else True)
            seen.add(qp[0])
        sim._general_prepare(g, bool(spec.get("auto")))
    assert seen == set(codes)
    for name in QS.TRACED:
        assert len(QR.get("case", QS.FIXTURES[name])["trace"]) > 0


def test_the_recordings_take_every_distinguishing_branch():
    get = lambda name: QR.get("case", QS.FIXTURES[name])  # noqa: E731
    r = get("alifo_threshold_3_switches_modes")["q_state"][0]
    assert r[8] >= 3 and r[5] > 0 and r[6] > 0
    r = get("alifo_threshold_1_is_always_congested")["q_state"][0]
    assert r[5] == 0 and r[6] > 20 and r[8] == 1 and QS.FIXTURES["alifo_threshold_1_is_always_congested"]["servers"][0]["qp"][2] == 1
    qp = QS.FIXTURES["alifo_threshold_above_its_capacity_is_a_fifo"]["servers"][0]["qp"]
    r = get("alifo_threshold_above_its_capacity_is_a_fifo")
    assert qp[2] > qp[1] and r["q_state"][0, 6] == 0 and r["dropped"][0] == r["q_state"][0, 7] > 0
    assert QS.BRANCHES == ("enter_delta_below_1", "enter_count_is_delta_above_1", "enter_delta_reset_to_1", "leave", "two_or_more_drops_in_one_pop")
    assert (get("codel_c2_enters_leaves_and_re_enters")["codel_branches"][:4] > 0).all()
    b = get("codel_c2_short_interval")["codel_branches"]
    assert b[0] > 0 and b[1] > 0 and b[3] > 0
    r = get("codel_one_nanosecond_interval_drains_the_queue")
    assert r["codel_branches"][4] > 0 and r["q_state"][0, 6] > r["q_state"][0, 8]
    # a LIFO's Sink sees other latencies than arrival order gives: some Request overtakes an older one
    r = get("lifo_unbounded_overloaded")
    created = r["sink_t_ns"] - np.round(r["sink_latency_s"] * 1e9).astype(np.int64)
    assert (np.diff(created) < 0).any()
    r = get("codel_checked_backend")
    assert r["by_kind"][19] > 0 and r["q_state"][:, 6].sum() > 0
    for nm in ("lifo", "alifo", "codel"):
        assert get(f"{nm}_behind_a_client_with_fixed_retry")["cl_stats"][0, 3] > 0 and get(f"{nm}_behind_a_gate_flush")["flow_stats"][0, 3] == 2
        assert get(f"{nm}_under_a_probe_on_depth")["probe_v"].max() >= 3 and get(f"{nm}_crashed_and_restarted")["fault_events"] == 4
    total = sum(QR.get("case", s)["codel_branches"] for s in QS.recorded_specs())
    assert (total > 0).all()


def test_the_refusals_by_name():
    for cls, why in ((hs.PriorityQueue, "host callable"), (hs.DeadlineQueue, "host callable"), (hs.FairQueue, "host callable"),
                     (hs.WeightedFairQueue, "host callables"), (hs.REDQueue, "process-wide random generator")):
        with pytest.raises(NotImplementedError, match=rf"queue_policy {cls.__name__} is not lowered to the engine.*{why}"):
            hs.Server("s", queue_policy=cls())
        with pytest.raises(NotImplementedError, match=cls.__name__):
            hs.Server("s", queue_policy=cls(3, key=len))
    with pytest.raises(NotImplementedError, match="queue_policy dict is not lowered to the engine: only FIFOQueue, LIFOQueue, AdaptiveLIFO and CoDelQueue"):
        hs.Server("s", queue_policy={})
    # a policy object that still holds items of an earlier run
    sim, servers = _chain(hs.LIFOQueue())
    servers[0].queue_policy._len = 2
    with pytest.raises(UT, match="server 'srv0': 2 items are still queued in its LIFOQueue"):
        sim.lowered()
    # a ParallelSimulation partition
    for pol in (hs.LIFOQueue(), hs.AdaptiveLIFO(2), hs.CoDelQueue()):
        sv = hs.Server("srv", queue_policy=pol)
        part = hs.SimulationPartition("p0", entities=[sv], sources=[hs.Source.poisson(rate=5, target=sv, name="src")])
        with pytest.raises(UT, match=rf"partition 'p0': the queue policy {type(pol).__name__} of Server 'srv' on a ParallelSimulation partition is not lowered"):
            hs.ParallelSimulation([part], end_time=hs.Instant.from_seconds(1))


def test_the_station_engines_name_the_policy_and_the_simulation_falls_to_the_single_heap():
    from happy_simulator_amd.lowering import LoweredGraph, lower, lower_lb

    for pol in (hs.LIFOQueue(), hs.AdaptiveLIFO(2), hs.CoDelQueue()):
        text = rf"server 'srv0': queue policy {type(pol).__name__} is not lowered on the station, network and pipeline engines"
        sim, servers = _chain(pol)
        with pytest.raises(UT, match=text):
            lower(sim._sources, sim._entities)
        g = sim.lowered()
        assert isinstance(g, GeneralGraph) and g.arrays.has_queue_policies and re.match(text, sim._station_refusal)
        # 64 plain chains take the fast path of the station engine; one policy among them and they do not
        sim, _servers = _chain(pol, n=64)
        assert isinstance(sim.lowered(), GeneralGraph) and re.match(text, sim._station_refusal)
    sim, _servers = _chain(None, n=64)
    assert isinstance(sim.lowered(), LoweredGraph)
    # the pipeline engine (a LoadBalancer over Servers)
    sink = hs.Sink("sink")
    backends = [hs.Server("b0", downstream=sink), hs.Server("b1", queue_policy=hs.CoDelQueue(), downstream=sink)]
    lb = hs.LoadBalancer("lb", backends=backends, strategy=hs.RoundRobin())
    sources = [hs.Source.poisson(rate=20.0, target=lb, name="src")]
    with pytest.raises(UT, match="backend 'b1': queue policy CoDelQueue is not lowered on the station, network and pipeline engines"):
        lower_lb(sources, backends + [lb, sink], lb)
    sim = hs.Simulation(sources=sources, entities=backends + [lb, sink], end_time=hs.Instant.from_seconds(1.0))
    assert isinstance(sim.lowered(), GeneralGraph) and "backend 'b1': queue policy CoDelQueue" in sim._station_refusal


def test_parts_carry_the_policy_rows_with_their_server():
    spec = QS.groups_spec(4)
    spec["servers"].append(QS.srv(0.05, None, out=None))
    spec["sources"].append(QS.src(["server", 8], 9.0))                      # a fifth component without a policy
    sim, pools = QS.build(spec)
    a = sim.lowered().arrays
    parts = split_parts(a)
    assert len(parts) == 5
    with_policy = [(ids, b) for ids, _pos, b in parts if b.qp_params is not None]
    assert len(with_policy) == 4
    for ids, b in with_policy:
        assert np.array_equal(b.qp_params, a.qp_params[ids]) and (b.qp_params[:, 0] != 0).sum() == 1
        assert (b.qp_params[b.kind != N.NODE_SERVER] == 0).all()


def test_compare_sees_a_difference_in_every_column_of_the_policy_state():
    spec = QS.FIXTURES["codel_c2_enters_leaves_and_re_enters"]
    ref = QR.get("case", spec)
    got = copy.deepcopy(ref)
    got["by_kind"] = ref["by_kind"][:N.EV_KINDS].copy()
    for key, (lo, hi) in {"internal_by_kind": (15, 19), "health_by_kind": (19, 22), "resilience_by_kind": (22, 28), "client_by_kind": (28, 31),
                          "flow_by_kind": (31, 39)}.items():
        got[key] = ref["by_kind"][lo:hi].copy()
    assert QS.NOT_COMPARED == {"trace", "by_kind", "pending_events", "time_travel", "probe_drops", "codel_branches"}
    QS.compare(spec["name"], got, ref)
    assert ref["q_state"].shape == (1, 16) and ref["q_state"][0, 13] > 0 and ref["q_state"][0, 15] > 0    # both Instants are set
    for col in range(16):
        altered = dict(got, q_state=got["q_state"].copy())
        altered["q_state"][0, col] += 1
        with pytest.raises(AssertionError, match="q_state"):
            QS.compare(spec["name"], altered, ref)
    with pytest.raises(AssertionError, match="q_state"):
        QS.compare(spec["name"], {k: v for k, v in got.items() if k != "q_state"}, ref)


def test_the_new_symbols_are_in_the_header_and_the_library_and_no_struct_changed():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    syms = ("hs_graph_set_queue_policy", "hs_graph_get_queue_policy", "hs_debug_codel_next")
    for sym in syms:
        assert re.search(rf"\bint {sym}\(", hdr) and sym in N.EXPORTED_SYMBOLS
    assert re.search(r"HS_QUEUE_FIFO = 0, HS_QUEUE_LIFO = 1, HS_QUEUE_ADAPTIVE_LIFO = 2, HS_QUEUE_CODEL = 3", hdr)
    assert (N.QUEUE_FIFO, N.QUEUE_LIFO, N.QUEUE_ADAPTIVE_LIFO, N.QUEUE_CODEL) == (0, 1, 2, 3)
    assert re.search(rf"#define HS_QUEUE_FIELDS {N.QUEUE_FIELDS}\b", hdr)
    assert re.search(r"#define HS_ABI_VERSION 16\b", hdr) and N.ABI_VERSION == 16 and N.EV_KINDS == 15
    assert C.sizeof(N.GraphConfig) == 64 and C.sizeof(N.GraphNodes) == 208 and C.sizeof(N.GraphStats) == 128
    if os.path.exists(N.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
        for sym in syms:
            assert re.search(rf" T {sym}$", out, re.M), sym
        lib = N.lib()
        assert lib.hs_abi_version() == 16
        for sym in syms:
            getattr(lib, sym)
