"""GPU: Client with timeouts and retry policies on the single-heap loop (csrc/hs_graph.hip kEvClReq .. kEvClTimeout and the completion
hook at every place a handler returns) against the recorded live reference (tests/golden/live_client/, written by
tests/golden/make_golden_client.py).  Every comparison is exact equality: Sink records, per-entity statistics, the Clients' counters,
keys in flight and response times bit for bit, event totals including the new kinds, the final `_crashed` flags.  No case is skipped
or excluded (test_every_recorded_case_is_compared)."""
import numpy as np
import pytest

import client_specs as CS
import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine
from recorded import CLIENT as CR

pytestmark = pytest.mark.gpu

# what the engine has no counterpart for (the reference heap's length, the recorder's time-travel count) or what is compared in a form
# of its own (by_kind: the engine reports the public fifteen kinds, the internal ones per graph; trace: test_record_order_follows_the_trace)
_NOT_COMPARED = {"trace", "by_kind", "pending_events", "time_travel"}
_FIRST_HC, _FIRST_WRAPPER, _FIRST_CLIENT = N.EV_KINDS + 4, N.EV_KINDS + 7, N.EV_KINDS + 13
_BY_KIND_SLICES = [("by_kind", N.EV_KINDS), ("internal_by_kind", _FIRST_HC), ("health_by_kind", _FIRST_WRAPPER), ("resilience_by_kind", _FIRST_CLIENT),
                   ("client_by_kind", _FIRST_CLIENT + 3)]


def _equals_the_recording(spec, sim, pools, ref):
    got = GF.results(spec, sim, pools, "client")
    FC.compare(spec["name"], got, ref, _NOT_COMPARED, _BY_KIND_SLICES)
    assert len(ref["by_kind"]) == 31
    for c in pools["client"]:
        # average_response_time: the reference's expression over the list, evaluated here (sum() differs between Python versions)
        times = c._response_times
        assert c.average_response_time == (sum(times) / len(times) if times else 0.0)
        assert c.in_flight_count == len(c._in_flight) and len(times) == c.stats.responses_received
        if times:
            assert c.get_response_time_percentile(0) == min(times) and c.get_response_time_percentile(1) == max(times)
            assert min(times) <= c.get_response_time_percentile(0.5) <= max(times)
    return got


def _run(spec, **kw):
    sim, pools = GF.build(spec, **kw)
    sim.run()
    assert isinstance(sim._graph, GeneralGraph) and "Client" in sim._station_refusal
    return sim, pools


def test_every_recorded_case_is_compared():
    """The parametrised tests below run every fixture and every random graph of client_specs, and every one has a recording."""
    names = [s["name"] for s in CS.all_specs()]
    assert len(names) == len(set(names)) == len(CS.FIXTURES) + CS.N_RANDOM and CS.N_RANDOM >= 120 and len(CS.FIXTURES) >= 40
    for spec in CS.all_specs():
        assert CR.get("case", spec)["total_events"] <= 40_000
    assert len(CS.TRACED) == 6
    for name in CS.TRACED:
        assert len(CR.get("case", CS.FIXTURES[name])["trace"]) > 0


@pytest.mark.parametrize("name", sorted(CS.FIXTURES))
def test_named_fixture_equals_the_reference(name):
    spec = CS.FIXTURES[name]
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, CR.get("case", spec))


@pytest.mark.parametrize("k", range(CS.N_RANDOM))
def test_random_graph_equals_the_reference(k):
    spec = CS.random_spec(k)
    sim, pools = _run(spec)
    _equals_the_recording(spec, sim, pools, CR.get("case", spec))


def test_what_the_issue_says_about_the_reference():
    sim, pools = _run(CS.FIXTURES["link_double_response_twenty_requests"])   # Client(0.02, FixedRetry(2, 0.05)) -> NetworkLink(0.03) -> Server
    c = pools["client"][0]
    assert c.stats == hs.ClientStats(requests_sent=40, responses_received=0, timeouts=40, retries=20, failures=20)
    assert sim._client_by_kind.tolist() == [40, 80, 40] and pools["sink"][0].events_received == 40
    assert pools["sink"][0].latencies_s == [0.04] * 40                       # created_at is the send time of the attempt
    sim, pools = _run(CS.FIXTURES["timeout_zero_sink"])                      # the timeout pops in front of the response
    c = pools["client"][0]
    assert c.stats == hs.ClientStats(15, 0, 15, 10, 5) and pools["sink"][0].events_received == 15 and c._next_request_id == 5
    sim, pools = _run(CS.FIXTURES["keyless_ten_plain_events"])               # ten plain Events share the keys (None, attempt)
    c = pools["client"][0]
    assert c.stats == hs.ClientStats(10, 3, 5, 0, 5) and c.in_flight_count == 0 and c._next_request_id == 0
    sim, pools = _run(CS.FIXTURES["retry_lands_after_the_restart"])
    c = pools["client"][0]
    assert c.stats == hs.ClientStats(3, 1, 2, 2, 0) and c._response_times == [0.0] and c.average_response_time == 0.0
    sim, pools = _run(CS.FIXTURES["client_crash_without_restart"])
    c = pools["client"][0]
    assert c.in_flight_count > 0 and c._crashed is True and all(k[0] is None or k[0] > 0 for k in c._in_flight)


@pytest.mark.parametrize("name", CS.TRACED)
def test_record_order_follows_the_trace(name):
    """The record log against the reference's full trace (time ns, kind, node, sort index of every popped Event): every Sink event and
    every `_client_response` that found its key, in the one processing order of the whole graph; and the engine's count of every kind
    equals the trace's."""
    spec = CS.FIXTURES[name]
    ref = CR.get("case", spec)
    trace = ref["trace"]
    sim, pools, g, eng, end_ns, _start, _c = FC.engine(spec)
    with eng:
        eng.run_until(end_ns)
        node, t, v = eng.records()
        by_kind = list(eng.summary().events_by_kind)
        _crashed, internal, _k = eng.faults()
        events = eng.client_events()
    assert by_kind == [int((trace[:, 1] == k).sum()) for k in range(N.EV_KINDS)]
    assert internal.tolist() == [int((trace[:, 1] == N.EV_KINDS + k).sum()) for k in range(4)]
    assert events.tolist() == [int((trace[:, 1] == _FIRST_CLIENT + k).sum()) for k in range(3)] and events.sum() > 0
    want = FC.live_rows(trace)
    at_sink = g.arrays.kind[node] == N.NODE_SINK
    assert np.array_equal(np.stack([t[at_sink], node[at_sink]], axis=1), want[:, [0, 2]])
    # the Clients' rows: response time and start time in ns; start + response time is the time of a `_client_response` of the trace
    at_client = g.arrays.kind[node] == N.NODE_CLIENT
    assert int(at_client.sum()) == int(ref["cl_stats"][:, 1].sum())
    resp_times = trace[trace[:, 1] == _FIRST_CLIENT + 1][:, 0]
    assert np.isin(t[at_client] + v[at_client], resp_times).all() and (np.diff(t[at_client] + v[at_client]) >= 0).all()
    assert len(pools["client"]) == 1 and np.array_equal(t[at_client] / 1e9, ref["cl_response_times"])


def _run_to_ends_with_tables(spec, ends_s, **caps):
    """FC.engine_run and every Client's table capacity at the end."""
    def tables(eng, g):
        return [eng.client(int(i))["table_capacity"] for i in np.nonzero(g.arrays.kind == N.NODE_CLIENT)[0]]

    return FC.engine_run(spec, ends_s, read=tables, **caps)


def test_windows_equal_one_run():
    for name in ("fixed_retry_crash_with_restart", "source_plain_and_send_request_mixed", "probe_on_in_flight_count", "link_delay_equals_timeout",
                 "client_crash_with_restart"):
        spec = CS.FIXTURES[name]
        ends = [0.25, 0.5, 0.5, 1.2, 1.6, 1.9000001, spec["end_s"]]          # 7 uneven windows, ends on tie and fault nanoseconds among them
        sim, pools, _ = _run_to_ends_with_tables(spec, ends)
        _equals_the_recording(spec, sim, pools, CR.get("case", spec))


def test_in_flight_table_grown_from_one_place_equals_the_reference():
    """A Client's table that starts with ONE place: the launch stops in front of every request that would not fit, the host doubles the
    table (the keys in flight and their start times move with it) and the run goes on -- with leaked keys, a crash and retries on the way."""
    for name in ("client_crash_with_restart", "source_plain_and_send_request_mixed", "probe_on_in_flight_count", "two_clients_on_one_server"):
        spec = CS.FIXTURES[name]
        sim, pools, tables = _run_to_ends_with_tables(spec, [spec["end_s"]], table_capacity=1)
        assert tables and max(tables) >= 2, tables                          # (grown from one place)
        got = _equals_the_recording(spec, sim, pools, CR.get("case", spec))
        roomy_sim, roomy_pools, roomy_tables = _run_to_ends_with_tables(spec, [spec["end_s"]], table_capacity=4096)
        assert roomy_tables == [4096] * len(tables)
        FC.same(got, GF.results(spec, roomy_sim, roomy_pools, "client"), name)


def test_growth_from_capacities_of_one_equals_a_run_with_room():
    """Heap, Request pool, record log and in-flight table start at their smallest under a backlog: send_request() ids pile up in
    flight behind a slow link and a paused Server while every buffer is moved several times."""
    spec = CS._g("growth_under_a_backlog", [CS.cl(["link", 0], 0.8, CS.fixed(3, 0.05)), CS.cl(["link", 1], None)], servers=[CS.srv(0.1, cap=None)],
                 links=[CS.link(0, 0.5, "exp", 0.2), CS.link(0, 0.4, "exp", 0.3)], sources=[CS.src(["client", 1], 60.0)],
                 schedule=CS.send(CS.C0, *[round(0.01 * k, 2) for k in range(120)]), faults=[CS.pause(["server", 0], 0.5, 1.5)], end_s=3.0, seed=5)
    grown_sim, grown_pools, tables = _run_to_ends_with_tables(spec, [spec["end_s"]], heap_capacity=1, request_capacity=1, record_capacity=1, table_capacity=1)
    roomy_sim, roomy_pools, _ = _run_to_ends_with_tables(spec, [spec["end_s"]], heap_capacity=1 << 16, request_capacity=1 << 16, record_capacity=1 << 16,
                                                             table_capacity=1 << 12)
    grown, roomy = GF.results(spec, grown_sim, grown_pools, "client"), GF.results(spec, roomy_sim, roomy_pools, "client")
    assert roomy["cl_stats"][0, 0] > 120 and roomy["cl_stats"][0, 1] > 0 and roomy["depth"].sum() + roomy["completed"].sum() > 50 and tables[0] >= 64
    FC.same(grown, roomy)


def test_64_replicas_equal_64_single_runs():
    base = CS.FIXTURES["fixed_retry_crash_with_restart"]
    other = CS.FIXTURES["lossy_link"]
    specs = [dict(base if i % 2 == 0 else other, end_s=2.5) for i in range(64)]
    built = []

    def build_fn():
        sim, pools = GF.build(specs[len(built)])
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 64, base_seed=700)
    assert len(results) == 64
    seen = set()
    for i, (sim, pools) in enumerate(built):
        assert isinstance(sim._graph, GeneralGraph) and sim._graph.arrays.has_clients
        got = GF.results(specs[i], sim, pools, "client")
        one_sim, one_pools = _run(specs[i], seed=700 + i)
        FC.same(got, GF.results(specs[i], one_sim, one_pools, "client"), i)
        seen.add((got["total_events"], tuple(got["cl_stats"].ravel().tolist())))
    assert len(seen) > 48


def test_32_groups_as_parts_equal_one_heap():
    """32 disconnected Source -> Client -> NetworkLink -> Server -> Sink groups, one Server paused per group, in ONE Simulation: the
    parts run side by side (hs_graph_run_parts) and leave what one heap over all of them leaves."""
    import happy_simulator_amd.simulation as S

    spec = CS.groups_spec(32)
    sim, pools = _run(spec)
    assert sim._graph_parts == 32
    old, S.MAX_PARTS = S.MAX_PARTS, 1
    try:
        one_sim, one_pools = _run(spec)
    finally:
        S.MAX_PARTS = old
    assert one_sim._graph_parts == 1
    got = GF.results(spec, sim, pools, "client")
    FC.same(got, GF.results(spec, one_sim, one_pools, "client"))
    assert (got["cl_stats"][:, 2] > 0).all() and (got["cl_stats"][:, 3] > 0).all() and (got["cl_stats"][:, 1] > 0).all()


@pytest.mark.parametrize("names, parts", [(CS.UNION_MEMBERS, 1), (CS.UNION_PARTS, len(CS.UNION_PARTS))])
def test_a_union_of_client_groups_as_parts_equals_the_recordings_of_its_members(names, parts):
    """Recorded fixtures without a random draw, driven by schedule()d requests alone, as the components of ONE Simulation: every
    member's Client, Server, links and Sink are left with what the member's own recording holds.  UNION_PARTS runs as parts, side by
    side; in UNION_MEMBERS a schedule()d request shares its nanosecond with a run-time Event of its part, which the parts leave to
    the one heap."""
    spec, members = CS.union_spec(names)
    sim, pools = _run(spec)
    assert sim._graph_parts == parts and len(members) in (5, 6)
    got = GF.results(spec, sim, pools, "client")
    for name, off in members:
        ref = CR.get("case", CS.FIXTURES[name])
        c, k = off["client"], off["sink"]
        assert np.array_equal(got["cl_stats"][c], ref["cl_stats"][0]), name
        assert np.array_equal(got["cl_keys"][got["cl_keys_off"][c]:got["cl_keys_off"][c + 1]], ref["cl_keys"]), name
        times = got["cl_response_times"][got["cl_response_times_off"][c]:got["cl_response_times_off"][c + 1]]
        assert times.tobytes() == ref["cl_response_times"].tobytes(), name
        lo, hi = got["sink_off"][k], got["sink_off"][k + 1]
        assert np.array_equal(got["sink_t_ns"][lo:hi], ref["sink_t_ns"]) and got["sink_latency_s"][lo:hi].tobytes() == ref["sink_latency_s"].tobytes(), name
        for key, pool in (("accepted", "server"), ("completed", "server"), ("dropped", "server"), ("packets_sent", "link"), ("packets_dropped", "link")):
            assert np.array_equal(got[key][off[pool]:off[pool] + len(ref[key])], ref[key]), (name, key)
    assert got["total_events"] == sum(CR.get("case", CS.FIXTURES[name])["total_events"] for name, _ in members)


def test_a_client_free_handle_in_a_batch_with_a_client_handle():
    """hs_graph_run_many: a graph without faults and without Clients, and a wrapper graph, share the launch (the fifth instantiation of
    the loop) with Client graphs and report what they report alone."""
    import rate_limiter_specs as RS
    import resilience_specs as XS

    plain_spec = RS.FIXTURES["token_constant"]
    wrapped = XS.FIXTURES["timeout_link_jitter"]
    with_client = [CS.FIXTURES["lossy_link"], CS.FIXTURES["source_plain_and_send_request_mixed"]]
    built = []

    def build_fn():
        k = len(built)
        sim, pools = GF.build(with_client[k]) if k < 2 else GF.build(wrapped) if k == 2 else GF.build(plain_spec)
        built.append((sim, pools))
        return sim

    results = hs.ParallelRunner().run_replicas(build_fn, 4, base_seed=40)
    assert len(results) == 4
    for i in range(2):
        one_sim, one_pools = _run(with_client[i], seed=40 + i)
        FC.same(GF.results(with_client[i], *built[i], "client"), GF.results(with_client[i], one_sim, one_pools, "client"), i)
    one_sim, one_pools = GF.build(wrapped, seed=42)
    one_sim.run()
    FC.same(GF.results(wrapped, *built[2], "resilience"), GF.results(wrapped, one_sim, one_pools, "resilience"), "wrapper")
    sim, pools = built[3]
    assert not sim._graph.arrays.has_clients and not sim._graph.arrays.has_wrappers and not sim._faults
    one_sim, one_pools = GF.build(plain_spec, seed=43)
    one_sim.run()
    FC.same(GF.results(plain_spec, sim, pools, "rate_limiter"), GF.results(plain_spec, one_sim, one_pools, "rate_limiter"), "plain")
    assert sim.summary.total_events_processed == one_sim.summary.total_events_processed


def test_a_client_node_that_was_never_configured_is_a_state_error():
    sim, _pools = GF.build(CS.FIXTURES["lossy_link"])
    g = sim.lowered()
    g.arrays.cl_params = None                                                  # (the handle is created without the client call)
    with GraphEngine(g.arrays, seed=1) as eng:
        with pytest.raises(N.EngineError, match="a Client without its parameters") as e:
            eng.run_until(10 ** 9)
        assert e.value.code == N.HS_E_STATE


def test_the_engine_refuses_what_the_host_refuses():
    """hs_graph_create / hs_graph_set_client / hs_graph_schedule_client on hand-made arrays."""
    sim, _pools = GF.build(CS.FIXTURES["two_links"])
    g = sim.lowered()
    a = g.arrays
    node = int(np.nonzero(a.kind == N.NODE_CLIENT)[0][0])
    with GraphEngine(a, seed=1) as eng:
        with pytest.raises(N.EngineError, match="configured already") as e:
            eng._check(eng._lib.hs_graph_set_client(eng._h, node, 0.5, None, 0, 0))
        assert e.value.code == N.HS_E_STATE
        for bad in (-1, 1 << 30):
            with pytest.raises(N.EngineError, match=r"is not in \[0, 2\^30\)") as e:
                eng.schedule(node, 0, bad)
            assert e.value.code == N.HS_E_UNSUPPORTED
        with pytest.raises(N.EngineError, match="is not a Client"):
            eng.schedule(0, 0, 1)
        eng.schedule(node, 0, (1 << 30) - 1)                                  # at the bound: taken
    keep = a.cl_delays_ns.copy()
    a.cl_delays_ns[0] = -1
    with pytest.raises(N.EngineError, match="delay must be >= 0") as e:
        GraphEngine(a, seed=1)
    assert e.value.code == N.HS_E_INVALID
    a.cl_delays_ns[:] = keep
    end = a.target.copy()
    a.target[[i for i in np.nonzero(a.kind == N.NODE_LINK)[0] if a.kind[a.target[i]] != N.NODE_LINK][0]] = node     # ... -> link -> the Client itself
    with pytest.raises(N.EngineError, match="two completion hooks on one Event") as e:
        GraphEngine(a, seed=1)
    assert e.value.code == N.HS_E_UNSUPPORTED
    a.target[:] = end
