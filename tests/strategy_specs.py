"""Specs for the WeightedRoundRobin / IPHash / LeastConnections / WeightedLeastConnections strategies, in the graph-spec format of
tests/random_specs.py (graph_spec / lb_graph_spec) with two additions: a LoadBalancer's `strategy` may be "wrr" | "ip_hash" |
"least_conn" | "wlc" (next to "chash" | "round_robin" | "random"), with `weights` (per backend, in add_backend order) for the two
weighted ones; a Server may have svc="const"; `server_stream_offset` = n moves Server s to SERVICE stream base n + s -- the
pipeline lowering numbers its backends behind the Sources (lowering.lower_lb: backend j -> len(sources) + j), the single-heap lowering
counts Servers from 0 (graph_engine.lower_general), and a spec is recorded with the numbering of the path `hs.Simulation` takes.
tests/golden/make_golden_strategies.py runs the LIVE reference on every spec listed here and records what it computed
(tests/recorded.py STRATEGIES reads it back); `build()` wires the product's objects the same way.

  FIXTURES        named cases, recorded with their full event trace
  random_spec(k)  150 seeded cases: pipeline shapes (k % 3 == 0) and general graphs (random_specs.lb_graph_spec with the
                  strategies swapped in)
  WEIGHT_VECTORS  WeightedRoundRobin selection sequences, IP_HASH_TABLES IPHash tables
"""
import numpy as np

import happy_simulator_amd as hs
from random_specs import lb_graph_spec

NEW = ("wrr", "ip_hash", "least_conn", "wlc")
N_RANDOM = 150


def _weights(rng, n):
    return [int(rng.choice([1, 1, 2, 3, 5])) for _ in range(n)]


def pipeline_spec(k, strategy=None, n_backends=None, n_sources=None):
    """Sources -> ONE LoadBalancer -> Servers -> Sink(s): the shape the pipeline lowering takes (and the single-heap loop as well)."""
    rng = np.random.default_rng(85_000 + k)
    strategy = strategy or NEW[(k // 3) % 4]
    S = n_sources or int(rng.integers(1, 7))
    B = n_backends or int(rng.integers(1, 13))
    conc = [int(rng.choice([1, 1, 2, 3])) for _ in range(B)]
    mean = float(rng.choice([0.05, 0.1, 0.2]))
    cap = None if rng.random() < 0.5 else int(rng.integers(0, 4))
    shared = bool(rng.random() < 0.6)
    load = float(rng.uniform(0.4, 1.4)) * sum(conc) / mean          # under- and overloaded
    svc = str(rng.choice(["exp", "exp", "const"]))
    keyed = strategy == "ip_hash"
    n_clients = int(rng.choice([1, 13, 1000, 100000]))
    servers = [dict(mean=mean, c=conc[j], cap=cap, out=["sink", 0 if shared else j], svc=svc) for j in range(B)]
    sources = []
    for i in range(S):
        kind = "poisson" if keyed else str(rng.choice(["poisson", "poisson", "constant"]))
        sc = dict(kind=kind, rate=float(np.round(load / S * float(rng.uniform(0.6, 1.4)), 2)), to=["lb", 0])
        if keyed:
            sc["n_clients"] = n_clients
        sources.append(sc)
    lb = dict(strategy=strategy, vnodes=1, backends=list(range(B)))
    if strategy in ("wrr", "wlc"):
        lb["weights"] = _weights(rng, B)
    events = 12.0 * sum(sc["rate"] for sc in sources)
    end_s = float(np.round(min(max(3000.0 / events, 0.5), 40.0), 3))     # a few thousand events
    return dict(name=f"strategy_pipeline_{k}", topology="graph", n_sinks=1 if shared else B, servers=servers, links=[], routers=[],
                lbs=[lb], sources=sources, end_s=end_s, seed=int(rng.integers(1, 10_000)),
                server_stream_offset=S if strategy in ("wrr", "ip_hash") else 0)


def graph_spec(k):
    """random_specs.lb_graph_spec(k) with every LoadBalancer but the Random ones (which choose by the draw of a Source that aims at
    them) given one of the four strategies; all four take key-less Requests (IPHash through its fallback RoundRobin)."""
    spec = lb_graph_spec(k)
    rng = np.random.default_rng(83_000 + k)
    for lb in spec["lbs"]:
        if lb["strategy"] == "random":
            continue
        lb["strategy"] = str(rng.choice(NEW))
        if lb["strategy"] in ("wrr", "wlc"):
            lb["weights"] = _weights(rng, len(lb["backends"]))
    spec["name"] = f"strategy_graph_{k}"
    return spec


def random_spec(k):
    return pipeline_spec(k) if k % 3 == 0 else graph_spec(k)


def _lb_case(name, strategy, B, sources, *, weights=None, c=1, cap=None, mean=0.1, svc="exp", end_s=4.0, seed=7, shared=True,
             schedule=None, probes=None, pipeline=False):
    conc = c if isinstance(c, list) else [c] * B
    servers = [dict(mean=mean, c=conc[j], cap=cap, out=["sink", 0 if shared else j], svc=svc) for j in range(B)]
    lb = dict(strategy=strategy, vnodes=1, backends=list(range(B)))
    if weights is not None:
        lb["weights"] = list(weights)
    spec = dict(name=name, topology="graph", n_sinks=1 if shared else B, servers=servers, links=[], routers=[], lbs=[lb],
                sources=[dict(s, to=["lb", 0]) for s in sources], end_s=end_s, seed=seed,
                server_stream_offset=len(sources) if pipeline else 0)
    if schedule:
        spec["schedule"] = schedule
    if probes:
        spec["probes"] = probes
    return spec


def _poisson(n, rate, n_clients=0):
    return [dict(kind="poisson", rate=rate, **({"n_clients": n_clients} if n_clients else {})) for _ in range(n)]


def _fixtures():
    f = [
        # each strategy alone behind Poisson Sources
        _lb_case("wrr_poisson", "wrr", 4, _poisson(3, 14.0), weights=[5, 1, 1, 2], end_s=5.0, seed=11, pipeline=True),
        _lb_case("ip_hash_poisson", "ip_hash", 5, _poisson(3, 12.0, n_clients=200), shared=False, end_s=5.0, seed=12, pipeline=True),
        _lb_case("lc_poisson", "least_conn", 4, _poisson(3, 13.0), end_s=5.0, seed=13),
        _lb_case("wlc_poisson", "wlc", 4, _poisson(3, 13.0), weights=[3, 1, 2, 1], c=2, end_s=5.0, seed=14),
        # lock-step constant Sources: same-nanosecond selections that see equal `active`
        _lb_case("lc_lockstep_constant", "least_conn", 3, [dict(kind="constant", rate=8.0)] * 4, svc="const", mean=0.25, end_s=4.0,
                 seed=15),
        # concurrency > 1 and bounded queues, overloaded
        _lb_case("lc_conc_bounded", "least_conn", 3, _poisson(4, 20.0), c=[2, 3, 1], cap=2, mean=0.12, end_s=4.0, seed=16),
        # WeightedLeastConnections with ties in the score: 1 / 1 == 2 / 2 == 4 / 4, 1 / 2 == 2 / 4
        _lb_case("wlc_score_ties", "wlc", 4, [dict(kind="constant", rate=10.0)] * 3 + _poisson(1, 6.0), weights=[1, 2, 2, 4], c=4,
                 svc="const", mean=0.5, end_s=4.0, seed=17),
        # schedule()d key-less Requests at an IPHash LoadBalancer (its fallback RoundRobin), next to keyed and plain Sources
        _lb_case("ip_hash_scheduled_keyless", "ip_hash", 3, _poisson(2, 9.0, n_clients=50) + _poisson(1, 4.0), end_s=4.0, seed=18,
                 schedule=[[["lb", 0], t] for t in (0.0, 0.5, 0.5, 1.25, 2.0, 3.999, 4.0, 4.5)]),
        # Probes on active_requests (and depth) of backends
        _lb_case("lc_probe_active", "least_conn", 3, _poisson(3, 11.0), c=2, mean=0.15, end_s=4.0, seed=19,
                 probes=[[["server", 0], "active_requests", 0.1], [["server", 2], "active_requests", 0.25], [["server", 1], "depth", 0.2]]),
        # sizes on both sides of the lane-serial / cooperative crossover
        _lb_case("lc_8_backends", "least_conn", 8, _poisson(4, 25.0), mean=0.06, end_s=3.0, seed=20),
        _lb_case("lc_64_backends", "least_conn", 64, _poisson(4, 90.0), mean=0.15, c=[1, 2] * 32, end_s=1.5, seed=21),
        _lb_case("wlc_8_backends", "wlc", 8, _poisson(4, 25.0), weights=[1, 2, 3, 1, 5, 1, 2, 2], c=3, mean=0.2, end_s=3.0, seed=22),
        _lb_case("wlc_64_backends", "wlc", 64, _poisson(4, 90.0), weights=[1, 2, 3, 5] * 16, c=2, mean=0.4, end_s=1.5, seed=23),
        _lb_case("wrr_2048_backends", "wrr", 2048, _poisson(2, 700.0), weights=[1 + (j % 7 == 0) + 2 * (j % 64 == 5) for j in range(2048)],
                 mean=0.05, end_s=0.4, seed=24, pipeline=True),
    ]
    # a LoadBalancer behind a Server and a router
    f.append(dict(
        name="lb_behind_server_and_router", topology="graph", n_sinks=2,
        servers=[dict(mean=0.03, c=2, cap=None, out=["lb", 0]), dict(mean=0.02, c=1, cap=None, out=["router", 0]),
                 dict(mean=0.08, c=1, cap=3, out=["sink", 0]), dict(mean=0.08, c=2, cap=None, out=["sink", 0]),
                 dict(mean=0.05, c=1, cap=None, out=["sink", 1]), dict(mean=0.1, c=1, cap=2, out=["sink", 1])],
        links=[], routers=[dict(targets=[["lb", 1], ["sink", 1], ["lb", 0]])],
        lbs=[dict(strategy="least_conn", vnodes=1, backends=[2, 3, 4]), dict(strategy="wrr", vnodes=1, backends=[4, 5, 3], weights=[1, 3, 2])],
        sources=[dict(kind="poisson", rate=12.0, to=0), dict(kind="poisson", rate=9.0, to=1), dict(kind="constant", rate=4.0, to=1)],
        end_s=5.0, seed=31))
    # two LoadBalancers sharing backends
    f.append(dict(
        name="two_lbs_shared_backends", topology="graph", n_sinks=1,
        servers=[dict(mean=0.1, c=[1, 2, 1, 3, 1][j], cap=None, out=["sink", 0]) for j in range(5)], links=[], routers=[],
        lbs=[dict(strategy="least_conn", vnodes=1, backends=[0, 1, 2, 3]), dict(strategy="wlc", vnodes=1, backends=[3, 2, 4], weights=[2, 1, 3])],
        sources=[dict(kind="poisson", rate=14.0, to=["lb", 0]), dict(kind="poisson", rate=12.0, to=["lb", 1]),
                 dict(kind="constant", rate=5.0, to=["lb", 0]), dict(kind="constant", rate=5.0, to=["lb", 1])],
        end_s=5.0, seed=32))
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()

# WeightedRoundRobin selection sequences: 2 W + 3 selections of the live class for each vector
WEIGHT_VECTORS = {
    "equal_5": [1] * 5, "equal_w3": [3] * 4, "one_heavy": [1, 1, 10, 1], "heavy_first": [7, 1, 1], "nginx_5_1_1": [5, 1, 1],
    "two_classes": [2, 1, 2, 1, 2], "several_classes": [1, 2, 3, 5, 8, 13], "repeats": [3, 5, 3, 1, 5, 5, 1, 8, 2, 2],
    "single": [4], "pair": [2, 3], "coprime": [7, 11, 13], "descending": [13, 8, 5, 3, 2, 1, 1],
    "b2048": [1 + (j % 7 == 0) + 2 * (j % 64 == 5) + 12 * (j == 1000) for j in range(2048)],
}
# IPHash: (clients 0 .. n - 1, backend count)
IP_HASH_TABLES = [(64, 1), (300, 2), (1000, 3), (1000, 7), (2000, 64), (4096, 1000), (500, 2048)]


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


# ---- the product's objects ------------------------------------------------------------------------------------------------------
def make_strategy(lb):
    kind = lb["strategy"]
    if kind == "chash":
        return hs.ConsistentHash(virtual_nodes=lb["vnodes"])
    if kind == "round_robin":
        return hs.RoundRobin()
    if kind == "random":
        return hs.Random()
    return {"wrr": hs.WeightedRoundRobin, "ip_hash": hs.IPHash, "least_conn": hs.LeastConnections, "wlc": hs.WeightedLeastConnections}[kind]()


def make_lb(cls, j, lb, backends, strategy):
    """LoadBalancer j of a spec (`cls`: the product's or the reference's class).  Weights reach the strategy the two ways the reference
    offers: `add_backend(b, weight=w)` (even j) or `strategy.set_weight(b, w)` once the LoadBalancer exists (odd j) -- the constructor's
    own add_backend registers every backend with weight 1 (load_balancer.py:104-106,203-205)."""
    weights = lb.get("weights")
    if weights is None:
        return cls(f"lb{j}", backends=backends, strategy=strategy)
    if j % 2 == 0:
        out = cls(f"lb{j}", strategy=strategy)
        for b, w in zip(backends, weights):
            out.add_backend(b, weight=w)
        return out
    out = cls(f"lb{j}", backends=backends, strategy=strategy)
    for b, w in zip(backends, weights):
        strategy.set_weight(b, w)
    return out


def build(spec, start_ns=0, seed=None):
    """(Simulation, entities) wired like make_golden_strategies.run_strategy_case wires the reference's:
    `entities=servers + lbs + routers + links + sinks`, Sources and Probes in list order."""
    sinks = [hs.Sink(f"sink{j}") for j in range(spec["n_sinks"])]
    servers = [hs.Server(f"srv{i}", concurrency=sv.get("c", 1),
                         service_time=hs.ConstantLatency(sv["mean"]) if sv.get("svc") == "const" else hs.ExponentialLatency(sv["mean"]),
                         queue_capacity=sv.get("cap")) for i, sv in enumerate(spec["servers"])]
    links = []
    for l, lk in enumerate(spec["links"]):
        jit = None
        if lk.get("jm") is not None and lk.get("jk") == "exp":
            jit = hs.ExponentialLatency(lk["jm"])
        elif lk.get("jm") is not None and lk.get("jk") == "const":
            jit = hs.ConstantLatency(lk["jm"])
        links.append(hs.NetworkLink(f"link{l}", latency=hs.ConstantLatency(lk["lat"]), jitter=jit,
                                    packet_loss_rate=lk.get("loss", 0.0), egress=servers[lk["to"]]))
    routers = [None] * len(spec["routers"])
    lbs = []
    for j, lb in enumerate(spec.get("lbs") or []):
        backends = [servers[b] for b in lb["backends"]]
        lbs.append(make_lb(hs.LoadBalancer, j, lb, backends, make_strategy(lb)))
    pools = {"sink": sinks, "link": links, "router": routers, "server": servers, "lb": lbs}
    pending = list(range(len(routers)))
    while pending:
        for r in list(pending):
            tg = spec["routers"][r]["targets"]
            if all(k != "router" or routers[i] is not None for k, i in tg):
                routers[r] = hs.RandomRouter(f"router{r}", targets=[pools[k][i] for k, i in tg])
                pending.remove(r)
    for i, sv in enumerate(spec["servers"]):
        if sv.get("out") is not None:
            servers[i].downstream = pools[sv["out"][0]][sv["out"][1]]
    sources = []
    for k, sc in enumerate(spec["sources"]):
        make = hs.Source.poisson if sc["kind"] == "poisson" else hs.Source.constant
        to = servers[sc["to"]] if isinstance(sc["to"], int) else pools[sc["to"][0]][sc["to"][1]]
        if sc.get("n_clients"):
            sources.append(make(rate=sc["rate"], event_provider=hs.ClientKeyEventProvider(to, n_clients=sc["n_clients"]), name=f"src{k}"))
        else:
            sources.append(make(rate=sc["rate"], target=to, name=f"src{k}"))
    pools["source"] = sources
    probes = [hs.Probe.on(pools[kind][idx], metric, interval=interval) for (kind, idx), metric, interval in spec.get("probes") or []]

    def at(t_s):
        return hs.Instant(start_ns + hs.Instant.from_seconds(t_s).nanoseconds)

    sim = hs.Simulation(end_time=at(spec["end_s"]), sources=sources, entities=servers + lbs + routers + links + sinks,
                        seed=spec["seed"] if seed is None else seed,
                        **({"start_time": hs.Instant(start_ns)} if start_ns else {}),
                        **({"probes": [p for p, _ in probes]} if probes else {}))
    for (kind, idx), t_s in spec.get("schedule") or []:
        sim.schedule(hs.Event(time=at(t_s), event_type="Request", target=pools[kind][idx]))
    return sim, dict(sources=sources, servers=servers, links=links, routers=routers, sinks=sinks, lbs=lbs, probes=probes)


def lower_single_heap(sim, spec):
    """graph_engine.lower_general of the Simulation with the spec's stream numbering."""
    from happy_simulator_amd import _native as N
    from happy_simulator_amd.graph_engine import lower_general

    g = lower_general(sim._sources, sim._entities, sim._probes)
    g.arrays.stream_base[g.arrays.kind == N.NODE_SERVER] += np.uint64(spec.get("server_stream_offset", 0))
    return g


def force_single_heap(sim, spec):
    """The same Simulation on the single-heap loop, whatever the station engines would take, with the spec's stream numbering."""
    sim._graph = lower_single_heap(sim, spec)
    sim._station_refusal = "forced onto the single-heap loop by the test"
    return sim


def results(spec, sim, ents):
    """What make_golden_strategies.run_strategy_case records, read off the product's objects after run() (without the trace)."""
    s, v, l, r, k = ents["sources"], ents["servers"], ents["links"], ents["routers"], ents["sinks"]
    out = dict(total_events=sim.summary.total_events_processed, final_ns=sim._current_time.nanoseconds,
               by_kind=np.array(list(sim._engine_summary.events_by_kind), np.int64))
    out["generated"] = np.array([x.generated_count for x in s], np.int64)
    out["accepted"] = np.array([x.stats_accepted for x in v], np.int64)
    out["dropped"] = np.array([x.stats_dropped for x in v], np.int64)
    out["completed"] = np.array([x._requests_completed for x in v], np.int64)
    out["rejected"] = np.array([x._requests_rejected for x in v], np.int64)
    out["depth"] = np.array([x.depth for x in v], np.int64)
    out["active"] = np.array([x.active_requests for x in v], np.int64)
    out["total_service_s"] = np.array([x._total_service_time for x in v], np.float64)
    out["received"] = np.array([x.events_received for x in k], np.int64)
    out["routed"] = np.array([x.stats_routed for x in r], np.int64)
    out["packets_sent"] = np.array([x.packets_sent for x in l], np.int64)
    out["packets_dropped"] = np.array([x.packets_dropped for x in l], np.int64)
    lbs = ents["lbs"]
    out["lb_stats"] = np.array([[lb.stats.requests_received, lb.stats.requests_forwarded, lb.stats.requests_failed,
                                 lb.stats.no_backend_available, lb._in_flight_count] for lb in lbs], np.int64).reshape(-1, 5)
    tot, off, cw = [], [0], []
    index = []
    for lb in lbs:
        tot.extend(lb.get_backend_info(b).total_requests for b in lb.all_backends)
        off.append(len(tot))
        st = lb.strategy
        index.append(st._fallback._index if isinstance(st, (hs.ConsistentHash, hs.IPHash)) else getattr(st, "_index", -1))
        cw.extend(st._current_weights.get(b.name, 0) if isinstance(st, hs.WeightedRoundRobin) else 0 for b in lb.all_backends)
    out["lb_backend_total_requests"] = np.asarray(tot, np.int64)
    out["lb_backend_off"] = np.asarray(off, np.int64)
    out["lb_rr_index"] = np.asarray(index, np.int64)
    out["lb_current_weights"] = np.asarray(cw, np.int64)
    sink_t, sink_cr, soff = [], [], [0]
    for x in k:
        sink_t.extend(np.asarray(x.completion_ns).tolist())
        sink_cr.extend(np.asarray(x._created_ns).tolist())
        soff.append(len(sink_t))
    out["sink_t_ns"] = np.asarray(sink_t, np.int64)
    out["sink_created_ns"] = np.asarray(sink_cr, np.int64)
    out["sink_off"] = np.asarray(soff, np.int64)
    out["sink_latency_s"] = np.concatenate([np.asarray(x.latencies_array, np.float64) for x in k]) if k else np.zeros(0)
    pt, pv, poff = [], [], [0]
    for _p, d in ents["probes"]:
        pt.extend(np.asarray(d._t_ns).tolist())
        pv.extend(np.asarray(d._v).tolist())
        poff.append(len(pt))
    out["probe_t_ns"], out["probe_v"], out["probe_off"] = np.asarray(pt, np.int64), np.asarray(pv, np.int64), np.asarray(poff, np.int64)
    return out
