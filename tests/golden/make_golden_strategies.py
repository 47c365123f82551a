#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for the WeightedRoundRobin / IPHash / LeastConnections /
WeightedLeastConnections strategies (components/load_balancer/strategies.py) -- the yardstick of tests/test_lb_strategies_host.py and
tests/test_gpu_lb_strategies.py.  Run by hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_strategies.py            # writes tests/golden/live_strategies/part_*.npz

Recorded (tests/recorded.py STRATEGIES reads them back):
  * constructor defaults and `set_weight` errors of the four classes;
  * selection sequences of the live WeightedRoundRobin (strategy_specs.WEIGHT_VECTORS, 2 W + 3 selections each);
  * the live IPHash.select for clients 0 .. n - 1 (strategy_specs.IP_HASH_TABLES);
  * every spec of strategy_specs.all_specs(): the reference's own event loop over its own components, with the Philox stream
    plugs of make_golden.py choosing the random numbers (arrivals, services, client ids, router and loss draws) -- every Sink
    record, per-entity statistics, LoadBalancer stats, BackendInfo.total_requests, the strategies' visible state, probe samples,
    event totals by kind, the first event beyond the end; the named fixtures with their full trace.
"""
from __future__ import annotations

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import strategy_specs as SS  # noqa: E402
import make_golden as MG  # noqa: E402  (the stream plugs and the trace classifier)
import hs_streams_py as hs  # noqa: E402
from happysimulator import ConstantLatency, Instant, Server, Simulation, Sink, Source  # noqa: E402
from happysimulator.components.load_balancer import strategies as ref_strategies  # noqa: E402
from happysimulator.components.load_balancer.load_balancer import LoadBalancer  # noqa: E402
from happysimulator.components.network.link import NetworkLink  # noqa: E402
from happysimulator.core.event import Event  # noqa: E402
from happysimulator.load.profile import ConstantRateProfile  # noqa: E402
from happysimulator.load.providers.constant_arrival import ConstantArrivalTimeProvider  # noqa: E402
from happysimulator.load.source import SimpleEventProvider  # noqa: E402
from recorded import STRATEGIES as SR  # noqa: E402


class _Named:
    def __init__(self, name):
        self.name = name


def strategy_defaults():
    """Constructor state and error messages of the four classes."""
    out = {}
    for kind in ("wrr", "wlc"):
        st = getattr(ref_strategies, RF.REF_STRATEGY[kind])()
        a, b = _Named("a"), _Named("b")
        st.set_weight(a, 4)
        errors = []
        for w in (0, -3):
            try:
                st.set_weight(b, w)
            except ValueError as e:
                errors.append(str(e))
        out[kind] = dict(default_weight=st.get_weight(b), set_weight=st.get_weight(a), weights=dict(st._weights), errors=errors,
                         attrs=sorted(vars(st)))
    ip = ref_strategies.IPHash()
    out["ip_hash"] = dict(fallback=type(ip._fallback).__name__, fallback_index=ip._fallback._index, attrs=sorted(vars(ip)))
    out["least_conn"] = dict(attrs=sorted(vars(ref_strategies.LeastConnections())))
    try:
        LoadBalancer("lb").add_backend(Server("s"), weight=0)
    except ValueError as e:
        out["add_backend_error"] = str(e)
    # how weights reach a strategy: a backend's first add_backend sets it, a repeated one only BackendInfo.weight; the constructor
    # registers its backends with weight 1, over whatever the strategy held
    st = ref_strategies.WeightedRoundRobin()
    a, b = Server("a"), Server("b")
    st.set_weight(a, 7)
    lb = LoadBalancer("lb", backends=[a], strategy=st)
    lb.add_backend(b, weight=9)
    lb.add_backend(b, weight=3)
    out["weights_through_add_backend"] = dict(constructor=st.get_weight(a), first=st.get_weight(b), info=lb.get_backend_info(b).weight)
    return out


def wrr_sequence(weights):
    """2 W + 3 selections of the live WeightedRoundRobin over backends 0 .. n - 1 with these weights, and its `_current_weights`."""
    backends = [_Named(f"b{i}") for i in range(len(weights))]
    st = ref_strategies.WeightedRoundRobin()
    for b, w in zip(backends, weights):
        st.set_weight(b, int(w))
    index = {b.name: i for i, b in enumerate(backends)}
    n = 2 * int(sum(weights)) + 3
    seq = np.array([index[st.select(backends, None).name] for _ in range(n)], np.int32)
    return dict(sequence=seq, current_weights=np.array([st._current_weights[b.name] for b in backends], np.int64))


def ip_hash_table(n_clients, n_backends):
    """The live IPHash.select for clients 0 .. n - 1 over `n_backends` backends; and what key-less Requests get."""
    backends = [_Named(f"b{i}") for i in range(n_backends)]
    index = {b.name: i for i, b in enumerate(backends)}
    st = ref_strategies.IPHash()
    at = Sink("k")
    tab = np.array([index[st.select(backends, Event(time=Instant.Epoch, event_type="Request", target=at,
                                                    context={"metadata": {"client_id": str(c)}})).name]
                    for c in range(n_clients)], np.int32)
    keyless = np.array([index[st.select(backends, Event(time=Instant.Epoch, event_type="Request", target=at, context={})).name]
                        for _ in range(2 * n_backends + 1)], np.int32)
    return dict(table=tab, keyless=keyless, fallback_index=st._fallback._index)


def run_strategy_case(spec, want_trace=False):
    """make_golden.run_graph_case's wiring (`entities=servers + lbs + routers + links + sinks`; streams: Source k ARRIVAL / KEY base k,
    Server s SERVICE base s (+ spec["server_stream_offset"]), link l LINK / LOSS base l, router r ROUTE base r) with the strategies of strategy_specs, constant
    services, Probes, and the event totals by kind.  Trace nodes: Sources, Probes, then the entities in that order."""
    seed = spec["seed"]
    import happysimulator.components.network.link as link_mod

    link_mod.random = MG._PerLinkRandom
    sinks = [Sink(f"sink{j}") for j in range(spec["n_sinks"])]
    base = int(spec.get("server_stream_offset", 0))            # (the numbering of the lowering hs.Simulation takes, strategy_specs)
    servers = [Server(f"srv{i}", concurrency=sv.get("c", 1),
                      service_time=(ConstantLatency(sv["mean"]) if sv.get("svc") == "const" else
                                    MG.PhiloxExponentialLatency(sv["mean"], hs.Stream(seed, base + i, hs.STREAM_SERVICE))),
                      queue_capacity=sv.get("cap")) for i, sv in enumerate(spec["servers"])]
    links = []
    for l, lk in enumerate(spec["links"]):
        jit = None
        if lk.get("jm") is not None and lk.get("jk") == "exp":
            jit = MG.PhiloxExponentialLatency(lk["jm"], hs.Stream(seed, l, hs.STREAM_LINK))
        elif lk.get("jm") is not None and lk.get("jk") == "const":
            jit = ConstantLatency(lk["jm"])
        links.append(NetworkLink(f"link{l}", latency=ConstantLatency(lk["lat"]), jitter=jit, packet_loss_rate=lk.get("loss", 0.0),
                                 egress=servers[lk["to"]]))
        links[l]._loss_stream = hs.Stream(seed, l, hs.STREAM_LOSS)
    routers = [None] * len(spec["routers"])
    lbs = []
    for j, lb in enumerate(spec.get("lbs") or []):
        backends = [servers[b] for b in lb["backends"]]
        lbs.append(SS.make_lb(LoadBalancer, j, lb, backends, RF.ref_strategy(lb)))
    pools = {"sink": sinks, "link": links, "router": routers, "server": servers, "lb": lbs}
    pending = list(range(len(routers)))
    while pending:
        progressed = False
        for r in list(pending):
            tg = spec["routers"][r]["targets"]
            if all(k != "router" or routers[i] is not None for k, i in tg):
                routers[r] = MG.PhiloxRandomRouter(f"router{r}", targets=[pools[k][i] for k, i in tg],
                                                   stream=hs.Stream(seed, r, hs.STREAM_ROUTE))
                pending.remove(r)
                progressed = True
        assert progressed, "router targets form a cycle of routers"
    for i, sv in enumerate(spec["servers"]):
        if sv.get("out") is not None:
            servers[i].downstream = pools[sv["out"][0]][sv["out"][1]]
    sources = []
    for k, sc in enumerate(spec["sources"]):
        prof = ConstantRateProfile(rate=sc["rate"])
        prov = (MG.PhiloxPoissonArrival(prof, Instant.Epoch, hs.Stream(seed, k, hs.STREAM_ARRIVAL)) if sc["kind"] == "poisson"
                else ConstantArrivalTimeProvider(prof, start_time=Instant.Epoch))
        to = servers[sc["to"]] if isinstance(sc["to"], int) else pools[sc["to"][0]][sc["to"][1]]
        ep = (MG.PhiloxClientProvider(to, sc["n_clients"], hs.Stream(seed, k, hs.STREAM_KEY)) if sc.get("n_clients")
              else SimpleEventProvider(to, "Request", None))
        sources.append(Source(f"src{k}", ep, prov))
    pools["source"] = sources
    probes, probe_data = [], []
    for (kind, idx), metric, interval in spec.get("probes") or []:
        probe, data = RF.recording_probe(pools[kind][idx], MG.PROBE_METRICS[metric][1], interval)
        probes.append(probe)
        probe_data.append(data)
    entities = servers + lbs + routers + links + sinks
    sim = Simulation(start_time=MG._start(spec), end_time=MG._at(spec, spec["end_s"]), sources=sources, entities=entities,
                     **({"probes": probes} if probes else {}))
    node_of = {}
    for i, x in enumerate(sources + probes):
        node_of[id(x)] = i
    first = len(sources) + len(probes)
    for i, x in enumerate(entities):
        node_of[id(x)] = first + i
        if isinstance(x, Server):
            for part in (x._queue, x._driver, x._worker):
                node_of[id(part)] = first + i
    cb_probe = {id(p._event_provider.data_sink): len(sources) + j for j, p in enumerate(probes)}
    by_kind = np.zeros(len(MG.EV), np.int64)
    trace = []
    heap = sim._event_heap
    orig_pop = heap.pop

    def pop():
        e = orig_pop()
        k, nd = MG.classify(e, node_of)
        if k == MG.EV["probe"]:
            fn = e.target._fn if hasattr(e.target, "_fn") else e.target.fn
            cells = {id(cell.cell_contents) for cell in (fn.__closure__ or ())}
            nd = next(c for key, c in cb_probe.items() if key in cells)
        by_kind[k] += 1
        if want_trace:
            trace.append((e.time.nanoseconds, k, nd, e._sort_index))
        return e

    heap.pop = pop
    for (kind, idx), t_s in spec.get("schedule") or []:
        sim.schedule(Event(time=MG._at(spec, t_s), event_type="Request", target=pools[kind][idx]))
    summary = sim.run()
    out = dict(total_events=int(summary.total_events_processed), final_ns=int(sim._current_time.nanoseconds), by_kind=by_kind)
    assert int(by_kind.sum()) == out["total_events"], "every popped event was processed (no time travel, nothing cancelled)"
    out["generated"] = np.array([s.generated_count for s in sources], np.int64)
    out["accepted"] = np.array([s.stats_accepted for s in servers], np.int64)
    out["dropped"] = np.array([s.stats_dropped for s in servers], np.int64)
    out["completed"] = np.array([s._requests_completed for s in servers], np.int64)
    out["rejected"] = np.array([s._requests_rejected for s in servers], np.int64)
    out["depth"] = np.array([s.depth for s in servers], np.int64)
    out["active"] = np.array([s.active_requests for s in servers], np.int64)
    out["total_service_s"] = np.array([s._total_service_time for s in servers], np.float64)
    out["received"] = np.array([k.events_received for k in sinks], np.int64)
    out["routed"] = np.array([r.stats_routed for r in routers], np.int64)
    out["packets_sent"] = np.array([l.packets_sent for l in links], np.int64)
    out["packets_dropped"] = np.array([l.packets_dropped for l in links], np.int64)
    out["lb_stats"] = np.array([[lb.stats.requests_received, lb.stats.requests_forwarded, lb.stats.requests_failed,
                                 lb.stats.no_backend_available, len(lb._in_flight)] for lb in lbs], np.int64).reshape(-1, 5)
    tot, toff, index, cw = [], [0], [], []
    for j, lb in enumerate(lbs):
        mine = [servers[b] for b in spec["lbs"][j]["backends"]]
        tot.extend(lb.get_backend_info(b).total_requests for b in mine)
        toff.append(len(tot))
        st = lb.strategy
        index.append(st._fallback._index if hasattr(st, "_fallback") else getattr(st, "_index", -1))
        cw.extend(getattr(st, "_current_weights", {}).get(b.name, 0) for b in mine)
    out["lb_backend_total_requests"] = np.asarray(tot, np.int64)
    out["lb_backend_off"] = np.asarray(toff, np.int64)
    out["lb_rr_index"] = np.asarray(index, np.int64)
    out["lb_current_weights"] = np.asarray(cw, np.int64)
    sink_t, sink_lat, off = [], [], [0]
    for k in sinks:
        sink_t.extend(t.nanoseconds for t in k.completion_times)
        sink_lat.extend(k.latencies_s)
        off.append(len(sink_t))
    out["sink_t_ns"] = np.asarray(sink_t, np.int64)
    out["sink_latency_s"] = np.asarray(sink_lat, np.float64)
    out["sink_off"] = np.asarray(off, np.int64)
    pt, pv, poff = [], [], [0]
    for d in probe_data:
        pt.extend(t for t, _ in d._ns)
        pv.extend(int(v) for _, v in d._ns)
        poff.append(len(pt))
    out["probe_t_ns"], out["probe_v"], out["probe_off"] = np.asarray(pt, np.int64), np.asarray(pv, np.int64), np.asarray(poff, np.int64)
    if want_trace:
        out["trace"] = np.asarray(trace, np.int64).reshape(-1, 4)
    return out


def main():
    cases = {SR.key("defaults"): strategy_defaults()}
    for name, w in SS.WEIGHT_VECTORS.items():
        cases[SR.key("wrr_sequence", w)] = wrr_sequence(w)
    for n, b in SS.IP_HASH_TABLES:
        cases[SR.key("ip_hash_table", n, b)] = ip_hash_table(n, b)
    for spec in SS.all_specs():
        fixture = spec["name"] in SS.FIXTURES
        cases[SR.key("case", spec)] = run_strategy_case(spec, want_trace=fixture and len(spec["servers"]) <= 64)
        print(spec["name"], cases[SR.key("case", spec)]["total_events"], flush=True)
    SR.write(cases)


if __name__ == "__main__":
    main()
