"""CPU: the WeightedRoundRobin / IPHash / LeastConnections / WeightedLeastConnections strategies on the host side -- the classes'
constructors, weights and errors, the selection table of csrc/hs_wrr.hpp and the IPHash table against what the LIVE reference
computed (tests/golden/live_strategies/, recorded by tests/golden/make_golden_strategies.py), the arrays both lowerings build, the
refusals, and the new C-ABI symbols.  No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import happy_simulator_amd as hs
import strategy_specs as SS
from happy_simulator_amd import _native as N
from happy_simulator_amd import lowering as L
from happy_simulator_amd.graph_engine import GeneralGraph, lower_general, split_parts
from recorded import STRATEGIES as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    N.build()
    return N.lib()


def _backends(n, sink=None, **kw):
    return [hs.Server(f"srv{j}", service_time=hs.ExponentialLatency(0.05), downstream=sink, **kw) for j in range(n)]


def test_constructors_weights_and_errors_equal_the_reference():
    ref = SR.get("defaults")
    for kind, cls in (("wrr", hs.WeightedRoundRobin), ("wlc", hs.WeightedLeastConnections)):
        st, a, b = cls(), hs.Server("a"), hs.Server("b")
        st.set_weight(a, 4)
        errors = []
        for w in (0, -3):
            with pytest.raises(ValueError) as e:
                st.set_weight(b, w)
            errors.append(str(e.value))
        got = dict(default_weight=st.get_weight(b), set_weight=st.get_weight(a), weights=dict(st._weights), errors=errors)
        assert got == {k: ref[kind][k] for k in got}
        assert set(ref[kind]["attrs"]) <= set(vars(st))             # `_weights`, `_default_weight` (and `_current_weights`)
    ip = hs.IPHash()
    assert type(ip._fallback).__name__ == ref["ip_hash"]["fallback"] and ip._fallback._index == ref["ip_hash"]["fallback_index"]
    assert vars(hs.LeastConnections()) == {} and ref["least_conn"]["attrs"] == []
    # how weights reach a strategy (load_balancer.py:104-106,189-205): a backend's first add_backend sets it, a repeated one only
    # BackendInfo.weight; the constructor registers its backends with weight 1, over whatever the strategy held
    st = hs.WeightedRoundRobin()
    a, b = hs.Server("a"), hs.Server("b")
    st.set_weight(a, 7)
    lb = hs.LoadBalancer("lb", backends=[a], strategy=st)
    lb.add_backend(b, weight=9)
    lb.add_backend(b, weight=3)
    assert dict(constructor=st.get_weight(a), first=st.get_weight(b), info=lb.get_backend_info(b).weight) == ref["weights_through_add_backend"]
    assert ref["weights_through_add_backend"] == dict(constructor=1, first=9, info=3)
    with pytest.raises(ValueError) as e:
        lb.add_backend(hs.Server("x"), weight=0)
    assert str(e.value) == ref["add_backend_error"]


@pytest.mark.parametrize("name", sorted(SS.WEIGHT_VECTORS))
def test_the_class_model_table_is_the_live_selection_sequence(lib, name):
    """hs_lb_wrr_table (csrc/hs_wrr.hpp, O(W x weight classes)) against 2 W + 3 selections of the live smooth weighted round robin:
    equal on every selection, periodic in W, and `_current_weights` follows from the per-backend counts."""
    w = SS.WEIGHT_VECTORS[name]
    ref = SR.get("wrr_sequence", w)
    table = hs.WeightedRoundRobin.selection_table(w)
    W = sum(w)
    assert len(table) == W and len(ref["sequence"]) == 2 * W + 3
    np.testing.assert_array_equal(table[np.arange(2 * W + 3) % W], ref["sequence"])
    np.testing.assert_array_equal(np.bincount(table, minlength=len(w)), w)           # backend i is taken w_i times per period
    t = 2 * W + 3
    counts = np.bincount(ref["sequence"], minlength=len(w))
    np.testing.assert_array_equal(np.asarray(w, np.int64) * t - W * counts, ref["current_weights"])
    if len(set(w)) == 1:
        np.testing.assert_array_equal(table, np.arange(W) % len(w))                   # all weights equal: RoundRobin's sequence


@pytest.mark.parametrize("n_clients,n_backends", SS.IP_HASH_TABLES)
def test_the_ip_hash_table_is_the_live_select(lib, n_clients, n_backends):
    ref = SR.get("ip_hash_table", n_clients, n_backends)
    got = [lib.hs_lb_ip_hash_select(str(c).encode(), n_backends) for c in range(n_clients)]
    np.testing.assert_array_equal(got, ref["table"])
    np.testing.assert_array_equal(np.arange(2 * n_backends + 1) % n_backends, ref["keyless"])      # the fallback RoundRobin
    assert ref["fallback_index"] == 2 * n_backends + 1


def test_new_symbols_are_declared_exported_and_check_their_arguments(lib):
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    for sym in ("hs_lb_set_weights", "hs_graph_set_lb_weights", "hs_graph_coop_selects", "hs_debug_graph_flags", "hs_lb_wrr_table",
                "hs_lb_ip_hash_select"):
        assert sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"\b{sym}\s*\(", hdr), sym
    enum = dict(re.findall(r"(HS_LB_[A-Z_]+) = (\d+)", hdr))
    assert {k: int(v) for k, v in enum.items() if "RUN" not in k} == dict(
        HS_LB_CONSISTENT_HASH=0, HS_LB_ROUND_ROBIN=1, HS_LB_RANDOM=2, HS_LB_WEIGHTED_ROUND_ROBIN=3, HS_LB_IP_HASH=4,
        HS_LB_LEAST_CONNECTIONS=5, HS_LB_WEIGHTED_LEAST_CONNECTIONS=6)
    src = open(os.path.join(ROOT, "happy_simulator_amd", "csrc", "hs_graph.hip")).read()
    assert int(re.search(r"constexpr int kCoopMinBackends = (\d+);", src).group(1)) == N.GRAPH_COOP_MIN_BACKENDS
    assert (N.LB_WEIGHTED_ROUND_ROBIN, N.LB_IP_HASH, N.LB_LEAST_CONNECTIONS, N.LB_WEIGHTED_LEAST_CONNECTIONS) == (3, 4, 5, 6)
    # out-of-range weights without a device
    out = np.zeros(8, np.int32)
    for bad in ([1, 0, 2], [-1], [3, 1, -7]):
        w = np.array(bad, np.int32)
        assert lib.hs_lb_wrr_table(w.ctypes.data, len(w), out.ctypes.data, len(out)) == N.HS_E_INVALID
        assert b"weight must be >= 1" in lib.hs_graph_last_error(None)
    big = np.array([1 << 23, 1 << 23, 1], np.int32)                                  # W = 2^24 + 1: beyond the table bound
    assert lib.hs_lb_wrr_table(big.ctypes.data, 3, None, 0) == N.HS_E_UNSUPPORTED
    assert b"2^24" in lib.hs_graph_last_error(None)
    one = np.ones(3, np.int32)
    assert lib.hs_lb_set_weights(None, one.ctypes.data) == N.HS_E_INVALID
    assert lib.hs_graph_set_lb_weights(None, 0, one.ctypes.data, 3) == N.HS_E_INVALID
    assert lib.hs_graph_coop_selects(None) == N.HS_E_INVALID and lib.hs_debug_graph_flags(None, 1) == N.HS_E_INVALID
    with pytest.raises(ValueError, match="weight must be >= 1, got 0"):
        hs.WeightedRoundRobin.selection_table([2, 0])
    with pytest.raises(NotImplementedError, match="2\\^24"):
        hs.WeightedRoundRobin.selection_table([1 << 24, 1])


def test_refusals_read_as_specified():
    for cls in (hs.PowerOfTwoChoices, hs.LeastResponseTime):
        with pytest.raises(NotImplementedError, match=f"strategy {cls.__name__} is not lowered.*process-wide random generator"):
            hs.LoadBalancer("lb", strategy=cls())
    with pytest.raises(NotImplementedError, match="strategy object is not lowered"):
        hs.LoadBalancer("lb", strategy=object())
    with pytest.raises(ValueError, match="alpha must be in"):
        hs.LeastResponseTime(alpha=0.0)
    with pytest.raises(NotImplementedError, match="custom get_key is arbitrary Python"):
        hs.IPHash(get_key=lambda ev: "k")
    sink = hs.Sink("k")
    for cls in (hs.LeastConnections, hs.WeightedLeastConnections):
        srv = _backends(3, sink)
        lb = hs.LoadBalancer("lb", backends=srv, strategy=cls())
        src = hs.Source.poisson(rate=5, target=lb, name="s")
        with pytest.raises(hs.UnsupportedTopology, match=f"{cls.__name__} selects by the backends' live active_requests.*feedback"):
            L.lower_lb([src], [lb, *srv, sink], lb)
        sim = hs.Simulation(duration=1, sources=[src], entities=[lb, *srv, sink])
        assert isinstance(sim.lowered(), GeneralGraph) and "feedback" in sim._station_refusal
    # IPHash on the pipeline needs keyed Sources, like ConsistentHash; with a plain Source the single-heap loop runs its fallback
    srv = _backends(3, sink)
    lb = hs.LoadBalancer("lb", backends=srv, strategy=hs.IPHash())
    plain = hs.Source.poisson(rate=5, target=lb, name="s")
    with pytest.raises(hs.UnsupportedTopology, match="ClientKeyEventProvider"):
        L.lower_lb([plain], [lb, *srv, sink], lb)
    assert isinstance(hs.Simulation(duration=1, sources=[plain], entities=[lb, *srv, sink]).lowered(), GeneralGraph)


def test_the_pipeline_lowering_takes_weighted_round_robin_and_ip_hash():
    sink = hs.Sink("k")
    srv = _backends(4, sink)
    st = hs.WeightedRoundRobin()
    lb = hs.LoadBalancer("lb", backends=srv, strategy=st)
    st.set_weight(srv[1], 3)
    st.set_weight(srv[3], 2)
    srcs = [hs.Source.poisson(rate=5, target=lb, name=f"s{i}") for i in range(2)]
    g = hs.Simulation(duration=1, sources=srcs, entities=[lb, *srv, sink]).lowered()
    assert isinstance(g, L.LbGraph) and g.backends == srv and [st.get_weight(b) for b in g.backends] == [1, 3, 1, 2]
    srv = _backends(4, sink)
    lb = hs.LoadBalancer("lb", backends=srv, strategy=hs.IPHash())
    keyed = [hs.Source.poisson(rate=5, event_provider=hs.ClientKeyEventProvider(lb, n_clients=40), name=f"c{i}") for i in range(2)]
    g = hs.Simulation(duration=1, sources=keyed, entities=[lb, *srv, sink]).lowered()
    assert isinstance(g, L.LbGraph)
    src, _be = g.engine_arrays()
    np.testing.assert_array_equal(src.n_clients, [40, 40])


def test_the_graph_lowering_carries_strategies_and_weights():
    spec = SS.FIXTURES["lb_behind_server_and_router"]
    sim, ents = SS.build(spec)
    g = sim.lowered()
    assert isinstance(g, GeneralGraph)
    a = g.arrays
    lb_nodes = [g.node_of[id(lb)] for lb in ents["lbs"]]
    np.testing.assert_array_equal(a.lb_strategy[lb_nodes], [N.LB_LEAST_CONNECTIONS, N.LB_WEIGHTED_ROUND_ROBIN])
    off, cnt = int(a.rt_off[lb_nodes[1]]), int(a.rt_cnt[lb_nodes[1]])
    np.testing.assert_array_equal(a.lb_weights[off:off + cnt], [1, 3, 2])
    np.testing.assert_array_equal(a.rt_targets[off:off + cnt], [g.node_of[id(ents["servers"][b])] for b in (4, 5, 3)])
    off0, cnt0 = int(a.rt_off[lb_nodes[0]]), int(a.rt_cnt[lb_nodes[0]])
    np.testing.assert_array_equal(a.lb_weights[off0:off0 + cnt0], [1, 1, 1])
    # a graph without a weighted strategy carries no weights at all
    assert SS.build(SS.FIXTURES["lc_poisson"])[0].lowered().arrays.lb_weights is None
    # parts keep each LoadBalancer's weights next to its backends
    from random_specs import union_spec
    union = union_spec([dict(SS.FIXTURES["wlc_poisson"]), dict(SS.FIXTURES["two_lbs_shared_backends"])], name="u")
    ua = SS.build(union)[0].lowered().arrays
    parts = split_parts(ua)
    assert parts is not None and len(parts) == 2
    for ids, pos, b in parts:
        np.testing.assert_array_equal(b.lb_weights, ua.lb_weights[pos])
    np.testing.assert_array_equal(np.sort(np.concatenate([b.lb_weights for _i, _p, b in parts])), np.sort(ua.lb_weights))
    # too large a total weight is refused by name
    sink = hs.Sink("k")
    srv = _backends(2, sink)
    st = hs.WeightedRoundRobin()
    lb = hs.LoadBalancer("lb", backends=srv, strategy=st)
    st.set_weight(srv[0], 1 << 24)
    inner = hs.Server("front", service_time=hs.ExponentialLatency(0.01), downstream=lb)
    with pytest.raises(hs.UnsupportedTopology, match="total weight of 16777217"):
        lower_general([hs.Source.poisson(rate=5, target=inner, name="s")], [inner, lb, *srv, sink])


def test_every_spec_has_a_recording():
    """A spec without a recorded reference result fails here by name (never a skip)."""
    for spec in SS.all_specs():
        rec = SR.get("case", spec)
        assert rec["total_events"] == int(rec["by_kind"].sum()) > 0, spec["name"]
        assert ("trace" in rec) == (spec["name"] in SS.FIXTURES and len(spec["servers"]) <= 64), spec["name"]
    assert len(SS.FIXTURES) >= 8 and SS.N_RANDOM >= 150
    with pytest.raises(KeyError, match="no recorded reference result for case"):
        SR.get("case", dict(SS.FIXTURES["lc_poisson"], seed=-1))
    for path in os.listdir(SR.rec_dir):
        assert os.path.getsize(os.path.join(SR.rec_dir, path)) <= SR.part_bytes, path


def test_recorded_least_connections_follow_min_active_on_the_trace():
    """The recordings are what the issue says the reference does: in `lc_lockstep_constant` four lock-step Sources meet three idle
    backends, so the same-nanosecond selections see equal `active` (nothing has started service yet) and all take backend 0."""
    rec = SR.get("case", SS.FIXTURES["lc_lockstep_constant"])
    tr = rec["trace"]
    first = tr[tr[:, 0] == tr[tr[:, 1] == 11][0, 0]]                      # the first nanosecond with a LoadBalancer event
    enq = first[first[:, 1] == 1]
    assert len(enq) == 4 and len(set(enq[:, 2].tolist())) == 1            # four enqueues, one backend
