"""CPU: the oracle against the upstream reference on randomly drawn configurations -- beyond the 55 committed fixtures, which were
produced by exactly the same code path (tests/golden/make_golden.py: the reference's own event loop, queue protocol, Server generator
and sort-index ledger with per-entity Philox streams plugged in through its extension points).  Every count, statistic, Sink record
and, for the small cases, the full processed-event trace incl. `_sort_index`.  The reference's results are the ones recorded from the
live reference under tests/golden/live_reference/ (tests/reference_runs.py: `REF.run_case(spec)` returns what
`make_golden.run_case(spec)` returned; HS_RECORD_REFERENCE=1 re-records them where the reference is installed)."""
import numpy as np
import pytest

import helpers as H
from reference_runs import REF
from test_oracle_golden import (check_oracle_against_graph_golden, check_oracle_against_lb_golden, check_oracle_against_ring_golden,
                                check_oracle_against_station_golden, check_oracle_against_tandem_golden)

from random_specs import (graph_spec, jitter_ring_spec, lb_graph_spec, lb_probe_spec, lb_profile_spec, lb_spec as _lb_spec, lb_strategy_spec, lb_workers_spec, multi_source_ring_spec, multi_source_spec, ring_spec as _ring_spec, station_spec as _station_spec,
                          tie_spec)

pytestmark = pytest.mark.live_reference


@pytest.mark.parametrize("k", range(40))
def test_oracle_equals_live_reference_on_random_station_specs(k):
    spec = _station_spec(k)
    if spec["mode"] == "replicas":
        spec["trace"] = False                      # traces are recorded for one Simulation
    out, meta = REF.run_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert sum(gold.meta["total_events"]) > 0
    check_oracle_against_station_golden(gold)


@pytest.mark.parametrize("k", range(30))
def test_oracle_equals_live_reference_on_random_ring_specs(k):
    spec = _ring_spec(k)
    out, meta = REF.run_ring_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 100
    check_oracle_against_ring_golden(gold)


@pytest.mark.parametrize("k", range(20))
def test_oracle_equals_live_reference_on_random_load_balancer_specs(k):
    spec = _lb_spec(k)
    out, meta = REF.run_lb_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 50
    check_oracle_against_lb_golden(gold)


@pytest.mark.parametrize("k", range(40))
def test_oracle_equals_live_reference_on_tie_storms(k):
    """Same-nanosecond orders (lock-step constant sources, Requests injected at the start instant, c up to 16): the oracle's
    sort-index ledger against the reference's, full traces."""
    out, meta = REF.run_case(tie_spec(k))
    check_oracle_against_station_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", list(range(60)) + [1374])          # (1374 ...: the cases tools/gpu_random_sweep.py found, tests/test_gpu_random.py)
def test_oracle_equals_live_reference_with_several_sources_per_server(k):
    """Up to four Sources feeding one Server, in two `sources=[...]` orders, on tie storms and random configurations."""
    spec = multi_source_spec(k)
    if spec["mode"] == "replicas":
        spec["trace"] = False
    out, meta = REF.run_case(spec)
    check_oracle_against_station_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", list(range(30)) + [1068, 1084, 1282])
def test_oracle_equals_live_reference_with_several_sources_per_server_on_rings(k):
    out, meta = REF.run_ring_case(multi_source_ring_spec(k))
    check_oracle_against_ring_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", range(20))
def test_oracle_equals_live_reference_with_probes_on_load_balancer_graphs(k):
    out, meta = REF.run_lb_case(lb_probe_spec(k))
    check_oracle_against_lb_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", list(range(12)) + [1351])
def test_oracle_equals_live_reference_with_profiles_on_load_balancer_sources(k):
    out, meta = REF.run_lb_case(lb_profile_spec(k))
    check_oracle_against_lb_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", range(60))
def test_oracle_equals_live_reference_on_random_tandem_queues(k):
    """Server(downstream=<Server>), up to four in a row (tests/tandem_specs.py; every fourth case a lock-step tie storm): the
    cases tests/test_gpu_tandem.py runs engine == oracle on MI355X."""
    import tandem_specs as TS

    out, meta = REF.run_tandem_case(TS.tandem_spec(k))
    check_oracle_against_tandem_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", list(range(40)) + [7932, 8264])
def test_oracle_equals_live_reference_on_tandem_queues_with_probes_and_injected_requests(k):
    """tests/tandem_specs.py tandem_probe_case: Probes on Servers of the chains and Simulation.schedule() Requests next to tandem
    queues -- statistics, Sink records, every Probe sample and the full trace with sort indices.  7932 / 8264: two Requests reach
    an idle one-worker Server in one nanosecond and the reference rejects the second at the worker (server.py:223-234)."""
    import tandem_specs as TS

    out, meta = REF.run_tandem_case(TS.tandem_probe_case(k))
    check_oracle_against_tandem_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", list(range(0, 60)) + [1788, 4095, 4329, 4857, 6237])
def test_oracle_equals_live_reference_on_forests_of_servers(k):
    """tests/tandem_specs.py fan_in_case: several Servers forwarding to one, Sources of their own on downstream Servers; every third
    case lock-step constants.  The five extra cases are the ones the GPU sweep differed on while fan-in was being built (the worker's
    rejection of a second same-nanosecond Request; the Sources' first ticks and the restarted sort counter)."""
    import tandem_specs as TS
    from test_oracle_golden import check_oracle_against_fan_in_reference

    case = TS.fan_in_case(k)
    check_oracle_against_fan_in_reference(case, REF.run_fan_in_case(case))


# ---- the reference's own ParallelSimulation ---------------------------------------------------------------
def test_live_parallel_simulation_fixtures_are_current():
    """The committed parallel_* fixtures are what the live `ParallelSimulation(...).run()` computes now (threads and all)."""
    for spec in REF.attr("PARALLEL_CASES"):
        fn = REF.run_parallel_linked_case if spec["kind"] == "linked" else REF.run_parallel_independent_case
        out, meta = fn(dict(spec))
        gold = H.Golden(spec["name"])
        fresh = H.Golden.from_results(out, meta)
        drop = lambda m: {k: v for k, v in m.items() if k != "spec"}                                    # noqa: E731
        assert drop(fresh.meta) == drop(gold.meta), spec["name"]
        for k, v in gold.arrays.items():
            np.testing.assert_array_equal(fresh.arrays[k], v, err_msg=f"{spec['name']}: {k}")


def _two_partition_chain(hop):
    """Source -> Server_a -> <hop> -> Server_b -> Sink with library components; `hop(srv_b)` builds the hop."""
    from happysimulator import ConstantLatency, Server, Sink, Source

    sink = Sink("sink_b")
    srv_b = Server("srv_b", service_time=ConstantLatency(0.02), downstream=sink)
    h = hop(srv_b)
    srv_a = Server("srv_a", service_time=ConstantLatency(0.03), downstream=h if h is not None else srv_b)
    return Source.constant(rate=7, target=srv_a, event_type="Request"), srv_a, h, srv_b, sink


def _linked_refusals():
    """What the live reference raises in the three linked setups of the test below: [(exception type, message)] in order."""
    import warnings

    import make_golden as MG
    from happysimulator import ConstantLatency
    from happysimulator.components.network.link import NetworkLink
    from happysimulator.parallel import ParallelSimulation, PartitionLink, SimulationPartition

    def outcome(ps):
        try:
            ps.run()
        except Exception as e:                  # noqa: BLE001  (the refusal is the result)
            return (type(e).__name__, str(e))
        return ("", "")

    warnings.simplefilter("ignore")
    link = lambda srv_b: NetworkLink("hop", latency=ConstantLatency(0.05), egress=srv_b)           # noqa: E731
    src, a, hop, b, sink = _two_partition_chain(link)
    got = [outcome(ParallelSimulation([SimulationPartition(name="A", entities=[a, hop], sources=[src]),
                                       SimulationPartition(name="B", entities=[b, sink])], duration=2.0,
                                      links=[PartitionLink("A", "B", min_latency=0.05)]))]
    for owner in ("A", "B"):
        src, a, hop, b, sink = _two_partition_chain(link)
        pa = SimulationPartition(name="A", entities=MG._server_parts(a) + ([hop] if owner == "A" else []), sources=[src])
        pb = SimulationPartition(name="B", entities=([hop] if owner == "B" else []) + MG._server_parts(b) + [sink])
        got.append(outcome(ParallelSimulation([pa, pb], duration=2.0, links=[PartitionLink("A", "B", min_latency=0.05)])))
    src, a, hop, b, sink = _two_partition_chain(lambda srv_b: None)
    got.append(outcome(ParallelSimulation([SimulationPartition(name="A", entities=MG._server_parts(a), sources=[src]),
                                           SimulationPartition(name="B", entities=MG._server_parts(b) + [sink])], duration=2.0,
                                          links=[PartitionLink("A", "B", min_latency=0.05, latency=ConstantLatency(0.05))])))
    return got


def test_what_the_live_linked_parallel_simulation_refuses():
    """Failing by design -- three facts about the reference's LINKED mode that shape what `hs.ParallelSimulation(links=...)` mirrors
    (DESIGN section 7): (1) a library Server inside a linked partition needs its private queue / driver / worker listed as entities
    (parallel/routing.py:52-60); (2) a library NetworkLink cannot cross partitions, whichever side owns it: it forwards at its own
    `now`, the coordinator demands `delay >= min_latency` (parallel/coordinator.py:213-219); (3) `PartitionLink(latency=<library
    distribution>)` is unusable: the coordinator calls `.sample()` (`coordinator.py:209`), which no LatencyDistribution has.  What
    does cross is an entity that returns `Event(time=self.now + delay)` -- the pattern of the reference's own tests, which the
    parallel_linked_* fixtures use."""
    import re

    got = REF.value("linked_parallel_refusals", _linked_refusals)
    expect = [("RuntimeError", "srv_a.driver.*not in this partition"), ("RuntimeError", "violates min_latency: delay=0.000000s"),
              ("RuntimeError", "violates min_latency: delay=0.000000s"), ("AttributeError", "no attribute 'sample'")]
    assert len(got) == len(expect)
    for (kind, msg), (want_kind, pattern) in zip(got, expect):
        assert kind == want_kind and re.search(pattern, msg), (kind, msg)


@pytest.mark.parametrize("k", range(24))
def test_oracle_equals_live_reference_on_random_round_robin_and_random_load_balancers(k):
    """The LoadBalancer's default RoundRobin strategy and Random (its `random.choice` plugged per Request) on random topologies: the
    live reference against the oracle -- totals, per-backend statistics, every Sink record, probes, the full trace."""
    out, meta = REF.run_lb_case(lb_strategy_spec(k))
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 50
    check_oracle_against_lb_golden(gold)


@pytest.mark.parametrize("k", range(6))
def test_live_reference_ignores_a_probe_start_time(k):
    """`Probe(start_time=...)` seeds the probe's ConstantArrivalTimeProvider, but `Source.start()` overwrites the provider's
    clock with the Simulation's start time before it draws the first tick (load/source.py:120-127): the live reference samples
    at start + k * interval whatever `start_time` says.  The mirror accepts the argument and does the same."""
    spec = next(s for s in (_station_spec(j) for j in range(7 * k, 400)) if s.get("probes") and s["mode"] != "replicas")
    spec["trace"] = False
    plain, meta = REF.run_case(dict(spec))
    shifted, meta2 = REF.run_case(dict(spec, probe_start_s=0.37 * spec["end_s"]))
    assert len(plain["probe_t_ns"]) > 0
    for key in plain:
        if key != "meta":                         # (the spec itself, with the extra field)
            assert np.array_equal(plain[key], shifted[key]), key
    check_oracle_against_station_golden(H.Golden.from_results(shifted, meta2))


@pytest.mark.parametrize("k", range(6))
def test_live_reference_capacity_probes_are_functions_of_active_requests(k):
    """`Server.available_capacity` (= limit - active, concurrency.py:129-131) and the callable `Server.has_capacity` (the probe
    calls it: probe.py:52-55; active < limit, concurrency.py:117-127) sampled by the live reference == the mirror's value maps
    applied to the live `active_requests` samples of the same run (probes draw no random numbers: same trajectory)."""
    import happy_simulator_amd as hs

    spec = next(s for s in (_station_spec(j) for j in range(5 * k, 400)) if s["mode"] != "replicas" and s["downstream"])
    spec["trace"] = False
    n = spec["n_chains"]
    conc = spec["concurrency"] if isinstance(spec["concurrency"], (list, tuple)) else [spec["concurrency"]] * n
    spec["probes"] = [["active_requests", 0.05 * spec["end_s"]]] * n
    base, _ = REF.run_case(dict(spec))
    for metric in ("available_capacity", "has_capacity"):
        out, _ = REF.run_case(dict(spec, probes=[[metric, 0.05 * spec["end_s"]]] * n))
        assert np.array_equal(out["probe_t_ns"], base["probe_t_ns"]) and np.array_equal(out["probe_off"], base["probe_off"])
        for c in range(n):
            lo, hi = int(base["probe_off"][c]), int(base["probe_off"][c + 1])
            srv = hs.Server(f"s{c}", concurrency=int(conc[c]))
            f = hs.Probe.value_map(metric, srv)
            assert [int(f(int(a))) for a in base["probe_v"][lo:hi]] == [int(v) for v in out["probe_v"][lo:hi]], (metric, c)
            assert hi > lo


@pytest.mark.parametrize("k", range(8))
def test_oracle_equals_live_reference_on_load_balancers_with_up_to_32_workers_per_backend(k):
    out, meta = REF.run_lb_case(lb_workers_spec(k))
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 500
    check_oracle_against_lb_golden(gold)


@pytest.mark.parametrize("k", range(24))
def test_oracle_equals_live_reference_on_rings_with_constant_exponential_and_no_jitter(k):
    """NetworkLink(jitter=ConstantLatency(x)) -- the reference's datacenter_network preset (components/network/conditions.py:60-63) --
    next to exponential jitter and none, per link: a constant on top of the base latency, no random number (link.py:195-200)."""
    out, meta = REF.run_ring_case(jitter_ring_spec(k))
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 100
    check_oracle_against_ring_golden(gold)


_PRESETS = ("local_network", "datacenter_network", "cross_region_network", "internet_network", "satellite_network", "mobile_3g_network",
            "mobile_4g_network")


def _preset_params(link):
    jit = link.jitter
    jm = None if jit is None else getattr(jit, "mean", None)
    if jm is None and jit is not None:
        jm = jit._mean_latency
    lat = getattr(link.latency, "mean", None)
    if lat is None:
        lat = link.latency._mean_latency
    return (link.name, float(lat), link.bandwidth_bps, link.packet_loss_rate, None if jit is None else type(jit).__name__, None if jm is None else float(jm))


def _presets(C):
    """Every preset's parameters from the module `C` (the reference's conditions module or the mirror) and whether
    lossy_network(1.5) raises ValueError."""
    out = {}
    for fn in _PRESETS:
        out[fn] = (_preset_params(getattr(C, fn)()), _preset_params(getattr(C, fn)("x")))
    out["lossy"] = (_preset_params(C.lossy_network(0.07)), _preset_params(C.lossy_network(0.5, "l2", 0.2)))
    out["slow"] = (_preset_params(C.slow_network(0.3)), _preset_params(C.slow_network(0.3, "s2", 5e5)))
    try:
        C.lossy_network(1.5)
        out["lossy_1.5"] = ""
    except ValueError:
        out["lossy_1.5"] = "ValueError"
    return out


def test_network_condition_presets_equal_the_live_references():
    """components/network/conditions.py:13-258 -- nine NetworkLink presets -- against the mirror's table: every parameter."""
    import happy_simulator_amd as hs

    def reference():
        from happysimulator.components.network import conditions as RC

        return _presets(RC)

    ref = REF.value("network_condition_presets", reference)
    mine = _presets(hs)
    assert list(ref) == list(mine)
    for fn in ref:
        assert mine[fn] == ref[fn], fn
    assert mine["lossy_1.5"] == "ValueError"


@pytest.mark.parametrize("k", range(40))
def test_oracle_equals_live_reference_on_random_graphs_beyond_the_engines(k):
    """random_specs.graph_spec: routers with up to 8 targets incl. Servers and several upstreams, links with several senders, Servers
    behind Servers inside link networks, more than four Sources per Server -- live reference == oracle."""
    out, meta = REF.run_graph_case(graph_spec(k))
    check_oracle_against_graph_golden(H.Golden.from_results(out, meta))


@pytest.mark.parametrize("k", range(60))
def test_oracle_equals_live_reference_on_graphs_with_several_load_balancers(k):
    """random_specs.lb_graph_spec: one to three LoadBalancers (ConsistentHash / RoundRobin / Random) behind Sources, Servers and
    routers of a general graph, `schedule()`d Requests on the key-less ones -- LoadBalancer.stats, BackendInfo.total_requests,
    RoundRobin._index and everything test_..._on_random_graphs_beyond_the_engines compares: live reference == oracle."""
    out, meta = REF.run_graph_case(lb_graph_spec(k))
    check_oracle_against_graph_golden(H.Golden.from_results(out, meta))


def _same_results(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "meta":
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("kind,k", [("station", 3), ("station", 11), ("tie", 5), ("ring", 2), ("ring", 9), ("lb", 1), ("lb", 7),
                                    ("multi_ring", 4)])
def test_the_reference_in_windows_equals_the_reference_in_one_run(kind, k):
    """VERDICT r4 missing 4: what `hs_engine_run_until` / `hs_lb_run` rely on when they serve a later window end by repeating the
    run (include/hs_engine.h).  The LIVE reference driven window by window (core/simulation.py:527-541 `_run_window`: growing ends,
    an end inside the gap before the event beyond the previous end, a repeated and an EARLIER end) leaves exactly what ONE run to
    the last end leaves: every count, statistic, Sink record, the total and the final time."""
    spec, run = {"station": (_station_spec(k), REF.run_case), "tie": (tie_spec(k), REF.run_case), "ring": (_ring_spec(k), REF.run_ring_case),
                 "lb": (_lb_spec(k), REF.run_lb_case), "multi_ring": (multi_source_ring_spec(k), REF.run_ring_case)}[kind]
    spec = dict(spec, trace=False)
    if spec.get("mode") == "replicas":
        spec["mode"] = "single"
    one, meta1 = run(dict(spec))
    e = spec["end_s"]
    win, meta2 = run(dict(spec, windows=[e / 7, e / 7 + 1e-9, e / 3, e / 3, e / 5, 2 * e / 3]))
    assert meta1["total_events"] == meta2["total_events"] and meta1["final_ns"] == meta2["final_ns"]
    assert sum(meta1["total_events"]) > 20
    _same_results(one, win, f"{kind} {k}")


# ---- the same configurations far from the epoch: Simulation(start_time=Instant(ns)) with an integer start ------------------------
# The engines choose their exact arithmetic by absolute time (tests/test_gpu_time_range.py runs them against the oracle at these
# offsets); here the oracle is held to the reference at the same offsets: 2^39 (the wavefront kernel's bound), 2^51 (binary64 whole
# ns) and 2^53 + 1 (float(ns) rounds).  Every absolute time of a spec -- the end, stop_after, window ends, scheduled Requests -- moves
# with the start; profiles keep their absolute definition, as in the reference.  A negative start: the reference accepts it, the
# oracle and the engines refuse it by name (test_a_negative_start_is_refused_by_the_oracle).
START_OFFSETS = pytest.mark.parametrize("start_ns", [1 << 39, 1 << 51, (1 << 53) + 1], ids=["2^39", "2^51", "2^53+1"])


def test_a_negative_start_is_refused_by_the_oracle():
    from oracle import hs_oracle as O

    out, meta = REF.run_case(dict(_station_spec(0), start_ns=-(1 << 31) - 7))     # the reference runs it ...
    assert sum(meta["total_events"]) > 0
    with pytest.raises(ValueError, match="start_time"):                          # ... the oracle does not guess
        H.run_oracle_for_spec(dict(_station_spec(0), start_ns=-(1 << 31) - 7))


@START_OFFSETS
@pytest.mark.parametrize("k", [0, 3])
def test_oracle_equals_live_reference_on_station_specs_at_an_offset(k, start_ns):
    spec = dict(_station_spec(k), start_ns=start_ns)
    spec["trace"] = spec["mode"] != "replicas" and spec.get("trace", False)
    out, meta = REF.run_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert sum(gold.meta["total_events"]) > 0
    assert min(gold.meta["final_ns"]) > start_ns
    check_oracle_against_station_golden(gold)


@START_OFFSETS
@pytest.mark.parametrize("k", [1])
def test_oracle_equals_live_reference_on_ring_specs_at_an_offset(k, start_ns):
    spec = dict(_ring_spec(k), start_ns=start_ns)
    out, meta = REF.run_ring_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 100 and gold.meta["final_ns"][0] > start_ns
    check_oracle_against_ring_golden(gold)


@START_OFFSETS
@pytest.mark.parametrize("make,k", [(_lb_spec, 2), (lb_profile_spec, 1), (lb_probe_spec, 0), (lb_strategy_spec, 1)],
                         ids=["lb", "profile", "probes", "strategy"])
def test_oracle_equals_live_reference_on_load_balancers_at_an_offset(make, k, start_ns):
    spec = dict(make(k), start_ns=start_ns)
    out, meta = REF.run_lb_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 50 and gold.meta["final_ns"][0] > start_ns
    check_oracle_against_lb_golden(gold)


@START_OFFSETS
@pytest.mark.parametrize("make,k", [(graph_spec, 0), (lb_graph_spec, 0)], ids=["graph", "lb_graph"])
def test_oracle_equals_live_reference_on_graphs_at_an_offset(make, k, start_ns):
    spec = dict(make(k), start_ns=start_ns)
    out, meta = REF.run_graph_case(spec)
    gold = H.Golden.from_results(out, meta)
    assert gold.meta["total_events"][0] > 50 and gold.meta["final_ns"][0] > start_ns
    check_oracle_against_graph_golden(gold)
