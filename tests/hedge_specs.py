"""Specs of Hedge and Fallback (happy_simulator_amd.entities; the reference's components/resilience/hedge.py, fallback.py) on the
single-heap loop.  The format is the mixed family's (tests/mixed_specs.py, tests/graph_family.py) and the link faults' `networks` and
fault kinds (tests/link_fault_specs.py), with two more lists:

  hedges    = [dict(to=<ref>, delay=<hedge_delay s>, n=<max_hedges>)]            Hedge(f"hg{i}", ref, delay, n)
  fallbacks = [dict(to=<ref of the primary>, fb=<ref of the fallback entity>, timeout=<s | None>)]     Fallback(f"fb{i}", ...)
  every <ref> of the format may be ["hedge", i] or ["fallback", i]; faults and probes may name them.

`wire()` here is graph_family.wire's counterpart for these specs -- both libraries see the same objects in the same order: entities =
servers + routers + links + limiters + sinks + flows + hedges + fallbacks (+ the Networks); a spec of this family holds no LoadBalancer,
Bulkhead, TimeoutWrapper, Client or HealthChecker (the pools exist and are empty, so the other families' result readers apply).

tests/golden/make_golden_hedge.py records every spec listed here from the live reference as family "hedge": what the "mixed" family
records, twenty-one more by_kind rows (39 .. 52: the scaler's and the deployers', always 0; 53 .. 59: HG_EVENTS) and hedge_results
below.  HEDGE reads the recordings back.  Every case has at most a few seconds of simulated time and at most 60 000 Events.

  FIXTURES        named cases; TRACED: recorded with their full event trace
  random_spec(k)  N_RANDOM seeded chains Source(s) -> 2 .. 5 stations over the legal neighbours of a Hedge / Fallback -> Sink
  groups_spec()   16 disconnected groups, one of 48 and one of 49 nodes among them: the parts of hs_graph_run_parts
"""
import numpy as np

import canary_specs as CN
import family_checks as FC
import graph_family as GF
import happy_simulator_amd as hs
import link_fault_specs as LF
import mixed_specs as MX
import rate_limiter_specs as RS
from happy_simulator_amd.graph_engine import GraphEngine
from recorded import Recorded

HEDGE = Recorded("live_hedge", "hedge", "make_golden_hedge.py", part_bytes=640 * 1024, max_part_bytes=900 * 1024)
N_RANDOM = 150
EV_HG_FIRST = CN.N_KINDS                       # the by_kind row of a Request at a Hedge, the first of the seven
HG_EVENTS = ("hg_req", "hg_resp", "hg_send", "fb_req", "fb_prim_resp", "fb_timeout", "fb_fb_resp")
N_KINDS = EV_HG_FIRST + len(HG_EVENTS)
crash, pause, src, plain, srv, link, bp, cv, gt, gate_events = (MX.crash, MX.pause, MX.src, MX.plain, MX.srv, MX.link, MX.bp, MX.cv, MX.gt,
                                                               MX.gate_events)
lat, net = LF.lat, LF.net
SINK, S0, S1, L0, L1, R0, LIM0, F0, H0, H1, FB0, FB1 = (["sink", 0], ["server", 0], ["server", 1], ["link", 0], ["link", 1], ["router", 0],
                                                      ["limiter", 0], ["flow", 0], ["hedge", 0], ["hedge", 1], ["fallback", 0], ["fallback", 1])


def hg(to, delay, n=1):
    return dict(to=to, delay=delay, n=n)


def fb(to, fallback, timeout):
    return dict(to=to, fb=fallback, timeout=timeout)


def keyed(to, rate=10.0, kind="poisson", n_clients=7):
    return dict(src(to, rate, kind), n_clients=n_clients)


def _g(name, *, hedges=(), fallbacks=(), **kw):
    return dict(MX._g(name, **kw), hedges=[dict(h) for h in hedges], fallbacks=[dict(f) for f in fallbacks])


def wire(spec, F, ns):
    """The spec's objects from the factory `F` (graph_family.Product, or the recorder's) and the namespace `ns` (where Hedge, Fallback
    and the flow entities come from): (pools by kind, Sources, Probes, entities)."""
    assert not (spec.get("lbs") or spec.get("wrappers") or spec.get("clients") or spec.get("checkers")), spec["name"]
    sinks = [F.sink(j) for j in range(spec["n_sinks"])]
    servers = [F.server(i, sv) for i, sv in enumerate(spec["servers"])]
    limiters = [F.limiter(i, lm) for i, lm in enumerate(spec.get("limiters") or [])]
    links = [F.link(l, lk) for l, lk in enumerate(spec["links"])]
    pools = {"sink": sinks, "server": servers, "limiter": limiters, "link": links, "lb": [], "wrapper": [], "client": [], "checker": []}
    later = {kind: spec.get(key) or [] for kind, key in (("router", "routers"), ("flow", "flows"), ("hedge", "hedges"), ("fallback", "fallbacks"))}
    for kind, items in later.items():
        pools[kind] = [None] * len(items)

    def ref(r):
        return servers[r] if isinstance(r, int) else pools[r[0]][r[1]]

    def ready(r):
        return isinstance(r, int) or pools[r[0]][r[1]] is not None

    pending = [(kind, i) for kind, items in later.items() for i in range(len(items))]
    while pending:
        progressed = False
        for kind, i in list(pending):
            item = later[kind][i]
            needs = item["targets"] if kind == "router" else [item["to"], item["fb"]] if kind == "fallback" else [item["to"]]
            if not all(ready(t) for t in needs):
                continue
            if kind == "router":
                pools[kind][i] = F.router(i, [ref(t) for t in needs])
            elif kind == "flow":
                pools[kind][i] = GF.make_flow(ns, i, item, ref(item["to"]))
            elif kind == "hedge":
                pools[kind][i] = ns.Hedge(f"hg{i}", ref(item["to"]), item["delay"], item["n"])
            else:
                pools[kind][i] = ns.Fallback(f"fb{i}", ref(item["to"]), ref(item["fb"]), timeout=item["timeout"])
            pending.remove((kind, i))
            progressed = True
        assert progressed, "routers, flows, hedges and fallbacks form a cycle"
    for l, lk in enumerate(spec["links"]):
        links[l].egress = None if lk["to"] is None else ref(lk["to"])
    for i, lm in enumerate(spec.get("limiters") or []):
        limiters[i]._downstream = ref(lm["out"])
    for i, sv in enumerate(spec["servers"]):
        if sv.get("out") is not None:
            servers[i].downstream = ref(sv["out"])
    sources = pools["source"] = [F.source(k, sc, ref(sc["to"])) for k, sc in enumerate(spec["sources"])]
    probes = pools["probe"] = [F.probe(ref(on), metric, interval) for on, metric, interval in spec.get("probes") or []]
    entities = servers + pools["router"] + links + limiters + sinks + pools["flow"] + pools["hedge"] + pools["fallback"]
    return pools, sources, probes, LF.with_networks(spec, pools, entities, ns)


def build(spec, seed=None, **sim_kw):
    """(Simulation, entities by pool) of the product, wired like the recorded reference run."""
    pools, sources, probes, entities = wire(spec, GF.Product, hs)
    start_ns = int(spec.get("start_ns", 0))

    def at(t_s):
        return hs.Instant(start_ns + hs.Instant.from_seconds(t_s).nanoseconds)

    fs, handles = LF.make_schedule(hs, spec, pools)
    sim = hs.Simulation(sources=sources, entities=entities, seed=spec["seed"] if seed is None else seed, max_graph_events=400_000,
                        fault_schedule=fs, **({} if spec.get("auto") else {"end_time": at(spec["end_s"])}),
                        **({"start_time": hs.Instant(start_ns)} if start_ns else {}), **({"probes": [p for p, _ in probes]} if probes else {}),
                        **sim_kw)
    GF.cancel_after(spec, handles)
    GF.schedule_all(spec, pools, sim, hs.Event, at, [])
    pools["probes"] = probes
    pools["fault_schedule"], pools["handles"] = fs, handles
    return sim, pools


def hedge_state(pools):
    """The object state of every Hedge and Fallback, as arrays: the counters, then every `_in_flight` entry in the dict's order."""
    hg_rows, hg_ent, hg_off, fb_rows, fb_ent, fb_off = [], [], [0], [], [], [0]
    for h in pools["hedge"]:
        st = h.stats
        hg_rows.append([st.total_requests, st.primary_wins, st.hedge_wins, st.hedges_sent, st.hedges_cancelled, h._next_request_id,
                        h.in_flight_count, int(bool(getattr(h, "_crashed", False)))])
        hg_ent.extend([int(rid), int(e["start_time"].nanoseconds), int(e["completed"]), int(e["hedges_sent"]), int(e["responses_received"])]
                      for rid, e in h._in_flight.items())
        hg_off.append(len(hg_ent))
    for f in pools["fallback"]:
        st = f.stats
        fb_rows.append([st.total_requests, st.primary_successes, st.primary_failures, st.fallback_invocations, st.fallback_successes,
                        st.fallback_failures, f._next_request_id, len(f._in_flight), int(bool(getattr(f, "_crashed", False)))])
        fb_ent.extend([int(rid), int(e["start_time"].nanoseconds), int(e["state"] == "fallback")] for rid, e in f._in_flight.items())
        assert all(e["state"] in ("primary", "fallback") for e in f._in_flight.values())
        fb_off.append(len(fb_ent))
    return dict(hg_stats=np.asarray(hg_rows, np.int64).reshape(-1, 8), hg_in_flight=np.asarray(hg_ent, np.int64).reshape(-1, 5),
                hg_in_flight_off=np.asarray(hg_off, np.int64), fb_stats=np.asarray(fb_rows, np.int64).reshape(-1, 9),
                fb_in_flight=np.asarray(fb_ent, np.int64).reshape(-1, 3), fb_in_flight_off=np.asarray(fb_off, np.int64))


def window_states(states):
    return {"window_" + k: [s[k] for s in states] for k in states[0]}


def hedge_results(spec, pools):
    """What both libraries' Hedges and Fallbacks show after a run."""
    out = hedge_state(pools)
    out["hg_params"] = [[h.target.name, float(h.hedge_delay), int(h.max_hedges)] for h in pools["hedge"]]
    out["fb_params"] = [[f.primary.name, f.fallback.name, f.timeout] for f in pools["fallback"]]
    out["hg_downstream"] = [[d.name for d in x.downstream_entities()] for x in pools["hedge"] + pools["fallback"]]
    return out


def results(spec, sim, pools):
    """Everything the recorder records for "hedge" except the trace, read off the product's objects after run()."""
    out = MX.results(spec, sim, pools)
    out.update(hedge_results(spec, pools))
    out["idle_by_kind"] = np.zeros(EV_HG_FIRST - MX.BY_KIND_SLICES[-1][1], np.int64)      # the scaler's and the deployers': none here
    for key in ("_autoscaler_by_kind", "_deployer_by_kind", "_canary_by_kind"):
        assert not hasattr(sim, key), key
    out["hedge_by_kind"] = np.asarray(getattr(sim, "_hedge_by_kind", np.zeros(len(HG_EVENTS))), np.int64)
    return out


WINDOW_KEYS = {"window_" + k for k in ("hg_stats", "hg_in_flight", "hg_in_flight_off", "fb_stats", "fb_in_flight", "fb_in_flight_off")}
# (same_ns_pairs / late_primary: what the recorder counts for the coverage checks of tests/test_hedge_host.py)
NOT_COMPARED = MX.NOT_COMPARED | WINDOW_KEYS | {"same_ns_pairs", "late_primary"}
BY_KIND_SLICES = MX.BY_KIND_SLICES + [("idle_by_kind", EV_HG_FIRST), ("hedge_by_kind", N_KINDS)]


def compare(name, got, ref):
    FC.compare(name, got, ref, NOT_COMPARED, BY_KIND_SLICES)


def engine(spec, **caps):
    """The spec on a GraphEngine of its own (not yet run), with its faults and its scheduled Events, as Simulation.run() sets it up."""
    sim, pools = build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, bool(spec.get("auto")))
    eng = GraphEngine(g.arrays, seed=spec["seed"], start_ns=start_ns, **caps)
    eng.add_faults(sim._general_faults(g))
    for entry in sched:
        eng.schedule(*entry)
    return sim, pools, g, eng, end_ns, start_ns, cancelled


def engine_run(spec, ends_s, read=None, **caps):
    """engine(spec), run to every end of `ends_s` in turn (None: the spec's own end); the results bound like Simulation.run() binds
    them.  `read(sim, pools, g, eng)` is called behind every end, with the results of the run so far bound."""
    sim, pools, g, eng, end_ns, start_ns, cancelled = engine(spec, **caps)
    with eng:
        for t in ends_s:
            eng.run_until(end_ns if t is None else start_ns + hs.Instant.from_seconds(t).nanoseconds)
            if read is not None:
                sim._general_finish(g, eng, end_ns, cancelled, 0.0)
                read(sim, pools, g, eng)
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    return sim, pools


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
LAT = 0.05                                     # the ConstantLatency of the link behind the wrappers of the timing fixtures


def hedged_link(name, delay, n=1, lk=None, rate=12.0, kind="poisson", mean=0.02, **kw):
    """Source -> Hedge -> NetworkLink -> Server -> Sink."""
    return _g(name, hedges=[hg(L0, delay, n)], servers=[srv(mean)], links=[link(0, LAT) if lk is None else lk], sources=[src(H0, rate, kind)],
              end_s=kw.pop("end_s", 3.0), **kw)


def guarded(name, timeout, fallback=S1, lk=None, rate=12.0, kind="poisson", servers=None, links=None, **kw):
    """Source -> Fallback -> NetworkLink -> Server 0 -> Sink, the fallback entity Server 1 -> Sink unless `fallback` says otherwise."""
    return _g(name, fallbacks=[fb(L0, fallback, timeout)], servers=[srv(0.02), srv(0.03)] if servers is None else servers,
              links=([link(0, LAT) if lk is None else lk]) + list(links or []), sources=[src(FB0, rate, kind)], end_s=kw.pop("end_s", 3.0), **kw)


def _fixtures():
    f = []
    # ---- hedge_delay below, at and above the link's latency, one to three hedges: at `= L` the send-hedge and the response share a nanosecond
    for n in (1, 2, 3):
        for tag, delay in (("below", 0.03), ("at", LAT), ("above", 0.08)):
            f.append(hedged_link(f"hedge_{n}_delay_{tag}_the_link_latency", delay, n, seed=100 + 10 * n + len(tag), traced=n == 2 or tag == "at"))
    f.append(hedged_link("hedge_constant_source_delay_at_the_link_latency", LAT, 2, kind="constant", rate=8.0, seed=140, traced=True))
    f.append(hedged_link("hedge_delay_half_the_link_latency_three_hedges", 0.025, 3, kind="constant", rate=8.0, seed=141, traced=True))
    f.append(hedged_link("hedge_over_a_jittered_lossy_link", 0.04, 2, lk=link(0, 0.03, "exp", 0.03, 0.25), rate=20.0, seed=142, traced=True))
    f.append(hedged_link("hedge_over_a_lossy_link_every_packet_lost", 0.04, 2, lk=link(0, 0.03, None, None, 1.0), seed=143))
    f.append(hedged_link("hedge_over_a_link_with_constant_jitter", 0.06, 1, lk=link(0, 0.03, "const", 0.03), seed=144))
    # ---- straight in front of a handler: the primary wins on the same nanosecond, the later send-hedge finds nothing
    f.append(_g("hedge_in_front_of_a_server", hedges=[hg(0, 0.05, 2)], servers=[srv(0.04, cap=2)], sources=[src(H0, 20.0, "poisson")], end_s=3.0, seed=150, traced=True))
    f.append(_g("hedge_in_front_of_a_sink", hedges=[hg(SINK, 0.05)], servers=[], sources=[src(H0, 10.0, "constant")], end_s=3.0, seed=151, traced=True))
    f.append(_g("hedge_in_front_of_a_router", hedges=[hg(R0, 0.02, 2)], servers=[srv(0.03)], routers=[dict(targets=[0, SINK])],
                sources=[src(H0, 15.0, "poisson")], end_s=3.0, seed=152, traced=True))
    f.append(_g("hedge_in_front_of_a_limiter", hedges=[hg(LIM0, 0.05)], servers=[srv(0.03)], limiters=[MX.token(3, 0)],
                sources=[src(H0, 15.0, "poisson")], end_s=3.0, seed=153, traced=True))
    # ---- faults: no hook fires at a crashed or paused target, the hedges go out and the entries stay
    f.append(hedged_link("crashed_hedge_target_restarts", 0.04, 3, faults=[crash(L0, 0.8, 1.9)], seed=160, traced=True))
    f.append(hedged_link("paused_hedge_target", 0.04, 2, faults=[pause(L0, 1.0, 1.6)], seed=161))
    f.append(hedged_link("crashed_server_behind_the_link", 0.04, 3, faults=[crash(S0, 0.7, 1.5)], seed=162))
    f.append(hedged_link("crashed_hedge_target_for_good", 0.03, 3, faults=[crash(L0, 1.2)], seed=163))
    f.append(hedged_link("crashed_hedge_restarts", 0.07, 3, lk=link(0, 0.1), faults=[crash(H0, 1.0, 1.8)], seed=164, traced=True))
    f.append(hedged_link("paused_hedge", 0.07, 2, lk=link(0, 0.1), faults=[pause(H0, 0.9, 1.4)], seed=165))
    # ---- the context survives on the duplicate: a client-keyed Source (the key rides in the metadata the Hedge copies)
    f.append(_g("client_keyed_source_through_a_hedge", hedges=[hg(L0, 0.03, 2)], servers=[srv(0.02)], links=[link(0, LAT, "exp", 0.02)],
                sources=[keyed(H0, 12.0)], end_s=3.0, seed=170, traced=True))
    f.append(_g("two_hedges_in_one_graph", hedges=[hg(L0, 0.03, 2), hg(L1, 0.06, 1)], servers=[srv(0.02, out=H1), srv(0.03)],
                links=[link(0, LAT), link(1, 0.04, "exp", 0.03)], sources=[src(H0, 12.0, "poisson")], end_s=3.0, seed=171, traced=True))
    f.append(_g("two_sources_into_two_hedges_over_one_link", hedges=[hg(L0, 0.03, 1), hg(L0, 0.07, 2)], servers=[srv(0.02, c=2)], links=[link(0, LAT)],
                sources=[src(H0, 8.0, "constant"), src(H1, 8.0, "constant")], end_s=3.0, seed=172))
    # ---- many Requests on one nanosecond at a Hedge: behind a Server, behind a batch that leaves its processor
    f.append(_g("hedge_behind_a_server", hedges=[hg(L0, 0.04, 2)], servers=[srv(0.03, c=3, out=H0), srv(0.02)], links=[link(1, LAT)],
                sources=[src(0, 10.0, "constant"), src(0, 10.0, "constant"), src(0, 10.0, "constant")], end_s=3.0, seed=173, traced=True))
    f.append(_g("hedge_behind_a_batch_processor", hedges=[hg(L0, LAT, 2)], flows=[bp(H0, 6, 0.05, 0.4)], servers=[srv(0.02, c=2)], links=[link(0, LAT)],
                sources=[src(F0, 25.0, "poisson")], end_s=3.0, seed=174, traced=True))
    f.append(hedged_link("probe_on_a_hedge_in_flight_count", 0.03, 2, faults=[pause(L0, 1.0, 1.5)], probes=[[H0, "in_flight_count", 0.1]], seed=175, traced=True))
    f.append(hedged_link("hedge_later_start_time", 0.03, 2, start_ns=5 * 10 ** 9, seed=176))
    # ---- Fallback: the timeout below, at and above the primary path's latency; no timeout at all
    for tag, timeout in (("below", 0.03), ("at", LAT), ("above", 0.08), ("none", None)):
        f.append(guarded(f"fallback_timeout_{tag}_the_primary_latency", timeout, seed=200 + len(tag), traced=True))
    f.append(guarded("fallback_constant_source_timeout_at_the_primary_latency", LAT, kind="constant", rate=8.0, seed=210, traced=True))
    # the primary's response comes 20 ms behind the timeout, while the copy is still on the fallback entity's link (state "fallback"): a no-op
    f.append(guarded("late_primary_response_after_the_timeout", 0.03, fallback=L1, links=[link(1, LAT)], seed=211, traced=True))
    f.append(guarded("late_primary_response_behind_a_jittered_link", 0.05, lk=link(0, 0.03, "exp", 0.03), rate=20.0, seed=212))
    # ---- the fallback entity: a Server, a Sink, a NetworkLink in front of a Server (its hook fires twice)
    f.append(guarded("fallback_entity_is_a_sink", 0.03, fallback=SINK, seed=213, traced=True))
    f.append(guarded("fallback_entity_is_a_link_in_front_of_a_server", 0.03, fallback=L1, links=[link(1, 0.02, "exp", 0.01)], seed=214, traced=True))
    f.append(guarded("fallback_entity_is_a_lossy_link", 0.03, fallback=L1, links=[link(1, 0.02, None, None, 0.4)], seed=215))
    f.append(_g("fallback_in_front_of_a_server", fallbacks=[fb(0, S1, 0.05)], servers=[srv(0.05, cap=1), srv(0.02)], sources=[src(FB0, 20.0, "poisson")],
                end_s=3.0, seed=216))
    # ---- faults
    f.append(guarded("crashed_primary", 0.08, faults=[crash(L0, 0.8, 1.9)], seed=220, traced=True))
    f.append(guarded("crashed_primary_without_a_timeout", None, faults=[crash(L0, 0.8, 1.9)], seed=221))
    f.append(guarded("crashed_fallback_entity", 0.03, faults=[crash(S1, 1.0, 2.0)], seed=222, traced=True))
    f.append(guarded("paused_fallback_entity_behind_a_link", 0.03, fallback=L1, links=[link(1, 0.02)], faults=[pause(L1, 1.0, 1.7)], seed=223))
    f.append(guarded("crashed_fallback_wrapper_restarts", 0.03, lk=link(0, 0.1), faults=[crash(FB0, 1.0, 1.8)], seed=224, traced=True))
    # InjectLatency on the primary's link: the run moves from "the primary wins" to "the fallback entity" in mid-run and back
    f.append(guarded("inject_latency_on_the_primary_link", 0.08, networks=[net(links=[0])], faults=[lat(0, 60.0, 1.0, 2.0)], seed=225, traced=True))
    f.append(guarded("inject_latency_while_the_fallback_entity_is_crashed", 0.08, fallback=S1, networks=[net(links=[0])], faults=[lat(0, 45.0, 0.9, 1.8), crash(S1, 1.2, 1.5)],
                     kind="constant", rate=8.0, seed=226))
    # primary and fallback entity share one downstream Sink (a Request that took both ways arrives twice)
    f.append(_g("primary_and_fallback_share_one_sink", fallbacks=[fb(L0, L1, 0.04)], servers=[], links=[link(SINK, LAT, "exp", 0.02), link(SINK, 0.02)],
                sources=[src(FB0, 15.0, "poisson")], end_s=3.0, seed=227, traced=True))
    f.append(_g("client_keyed_source_through_a_fallback", fallbacks=[fb(L0, S1, 0.04)], servers=[srv(0.02), srv(0.03)], links=[link(0, LAT, "exp", 0.02)],
                sources=[keyed(FB0, 12.0)], end_s=3.0, seed=228))
    f.append(_g("hedge_behind_a_fallback_server", hedges=[hg(L1, 0.03, 2)], fallbacks=[fb(L0, S1, 0.04)], servers=[srv(0.02, out=H0), srv(0.03), srv(0.02)],
                links=[link(0, LAT), link(2, 0.04)], sources=[src(FB0, 12.0, "poisson")], end_s=3.0, seed=229, traced=True))
    f.append(_g("two_fallbacks_in_one_graph", fallbacks=[fb(L0, S1, 0.04), fb(2, SINK, 0.02)], servers=[srv(0.02, out=FB1), srv(0.03), srv(0.05, cap=0)],
                links=[link(0, LAT)], sources=[src(FB0, 12.0, "poisson")], end_s=3.0, seed=230))
    by_name = {s["name"]: s for s in f}
    for base, windows in (("hedge_2_delay_at_the_link_latency", [0.31, 0.9, 0.9, 1.75, 2.6]), ("crashed_hedge_target_restarts", [0.5, 0.85, 1.3, 1.95, 2.2]),
                          ("late_primary_response_after_the_timeout", [0.4, 1.0, 1.03, 2.0, 2.9]), ("crashed_fallback_entity", [0.7, 1.0, 1.5, 2.05, 2.5])):
        f.append(dict(by_name[base], name=base + "_in_windows", traced=False, windows=windows))
    for s in f:
        s.setdefault("traced", False)
    return {s["name"]: s for s in f}


FIXTURES = _fixtures()
TRACED = sorted(n for n, s in FIXTURES.items() if s.get("traced"))


def random_spec(k):
    """One chain Source(s) -> 2 .. 5 stations drawn from {Server, link, router, limiter, BatchProcessor, ConveyorBelt, Hedge, Fallback}
    -> Sink, built from the Sink backwards, with 0 .. 2 faults over everything.  What lower_general refuses by name (a Hedge or a
    Fallback whose target is, through links, a flow entity or another of them) is drawn again; the first station in front of the
    Sources is a Hedge or a Fallback where the chain holds none yet.  Every third spec: constant Sources."""
    rng = np.random.default_rng(533_000 + k)
    pools = {p: [] for p in ("server", "link", "router", "limiter", "flow", "hedge", "fallback")}
    constant = k % 3 == 0
    end = float(rng.choice([2.0, 3.0]))

    def add(pool, item):
        pools[pool].append(item)
        return [pool, len(pools[pool]) - 1]

    def server(out):
        return add("server", srv(float(np.round(rng.uniform(0.01, 0.06), 3)), int(rng.integers(1, 3)), None if rng.random() < 0.6 else int(rng.integers(0, 3)), out=out))

    def a_link(to):
        return add("link", link(to, float(rng.choice([0.02, 0.04, 0.05])), *(("exp", float(rng.choice([0.01, 0.03]))) if rng.random() < 0.5 else (None, None)),
                               float(rng.choice([0.0, 0.0, 0.2]))))

    def wrapper(to):
        if rng.random() < 0.55:
            return add("hedge", hg(to, float(rng.choice([0.02, 0.04, 0.05, 0.07])), int(rng.integers(1, 4))))
        which = int(rng.integers(0, 3))
        other = SINK if which == 0 else server(SINK) if which == 1 else a_link(server(SINK))
        return add("fallback", fb(to, other, None if rng.random() < 0.1 else float(rng.choice([0.02, 0.04, 0.05, 0.07]))))

    at, hookable = SINK, True                  # hookable: a Hedge or a Fallback may stand in front of `at`
    n_stations = int(rng.integers(2, 6))
    for j in range(n_stations):
        last = j == n_stations - 1
        while True:
            r = int(rng.integers(0, 8))
            if last and not pools["hedge"] and not pools["fallback"] and hookable:
                r = 6
            if r >= 6 and not hookable:
                continue
            break
        if r == 0:
            at, hookable = server(at), True
        elif r == 1:
            at = a_link(at)
        elif r == 2:
            at, hookable = add("router", dict(targets=[at, SINK])), True
        elif r == 3:
            at, hookable = add("limiter", dict(policy=list(RS.FOUR["token"]), cap=int(rng.choice([0, 1, 3])), out=at)), True
        elif r == 4:
            at, hookable = add("flow", bp(at, int(rng.integers(1, 5)), float(rng.choice([0.0, 0.05])), float(rng.choice([0.0, 0.1, 0.25])))), False
        elif r == 5:
            at, hookable = add("flow", cv(at, float(rng.choice([0.0, 0.1])), int(rng.choice([0, 0, 3])))), False
        else:
            at, hookable = wrapper(at), False
    if not pools["hedge"] and not pools["fallback"]:
        at = wrapper(server(at))               # (the chain ended in front of a flow entity: a Server between them)
    rate = float(rng.choice([4.0, 10.0])) if constant else float(np.round(rng.uniform(6.0, 20.0), 1))
    sources = [src(at, rate, "constant" if constant else "poisson") for _ in range(int(rng.integers(1, 3)) if constant else 1)]
    if k % 5 == 4:
        sources[0] = keyed(at, rate, sources[0]["kind"])
    sizes = dict({p: len(v) for p, v in pools.items()}, sink=1)
    names = [p for p in ("hedge", "fallback", "server", "link", "sink", "router", "limiter", "flow") if sizes[p]]
    faults = []
    for _ in range(int(rng.integers(0, 3))):
        pool = str(rng.choice(names))
        on = [pool, int(rng.integers(0, sizes[pool]))]
        t0 = float(np.round(rng.uniform(0.0, end), 2))
        t1 = float(np.round(rng.uniform(t0, end * 1.05), 2))
        faults.append(pause(on, t0, t1) if rng.random() < 0.5 else crash(on, t0, None if rng.random() < 0.3 else t1))
    schedule = plain(at, *[float(x) for x in np.round(rng.uniform(0.0, end, size=2), 1)]) if k % 2 == 1 else []
    return _g(f"hedge_graph_{k}", hedges=pools["hedge"], fallbacks=pools["fallback"], flows=pools["flow"], servers=pools["server"], links=pools["link"],
              routers=pools["router"], limiters=pools["limiter"], sources=sources, faults=faults, end_s=end, seed=int(rng.integers(1, 10_000)),
              **({"schedule": schedule} if schedule else {}))


def all_specs():
    return list(FIXTURES.values()) + [random_spec(k) for k in range(N_RANDOM)]


def groups_spec(n_groups=16, name="hedge_groups", end_s=2.0, wide=(44, 44)):
    """`n_groups` disconnected groups in ONE Simulation: even groups Source -> Hedge -> link -> Server(s) -> Sink, odd groups Source ->
    Fallback -> link -> Server -> Sink with a Server of its own as the fallback entity.  Group g < len(wide) runs through wide[g]
    Servers in a row: with 44 of them the Hedge group has 48 nodes and the Fallback group, with its fallback Server, 49 -- around the 48
    node rows a side-by-side run keeps in LDS."""
    servers, links, hedges, fallbacks, sources, faults = [], [], [], [], [], []
    for g in range(n_groups):
        first = len(servers)
        tandem = wide[g] if g < len(wide) else 1
        for j in range(tandem):
            servers.append(srv(0.004 + 0.001 * (g % 3), c=2, out=["sink", g] if j == tandem - 1 else ["server", first + j + 1]))
        links.append(link(first, 0.03 + 0.01 * (g % 3), "exp", 0.02, 0.1 if g % 4 == 3 else 0.0))
        if g % 2 == 0:
            hedges.append(hg(["link", g], 0.03 + 0.01 * (g % 4), 1 + g % 3))
            sources.append(src(["hedge", len(hedges) - 1], 10.0 + g % 5, "poisson"))
        else:
            servers.append(srv(0.02, out=["sink", g]))
            fallbacks.append(fb(["link", g], ["server", len(servers) - 1], 0.04 + 0.01 * (g % 3)))
            sources.append(src(["fallback", len(fallbacks) - 1], 10.0 + g % 5, "poisson"))
        if g % 3 == 2:
            faults.append(pause(["link", g], 0.7 + 0.01 * g, 1.1 + 0.02 * g))
    return _g(name, hedges=hedges, fallbacks=fallbacks, servers=servers, links=links, sources=sources, n_sinks=n_groups, faults=faults,
              end_s=end_s, seed=71)


def group_sizes(spec):
    """The node counts of the parts the product splits the spec's graph into."""
    from happy_simulator_amd.graph_arrays import split_parts

    sim, _pools = build(spec)
    return [len(ids) for ids, _pos, _b in split_parts(sim.lowered().arrays)]


def leaked(ref, older_ns=500_000_000):
    """A recorded result holds an entry that stayed: in flight at the end and more than half a second old (no path of these specs
    takes that long)."""
    starts = np.concatenate([ref["hg_in_flight"][:, 1], ref["fb_in_flight"][:, 1]])
    return bool((starts < ref["final_ns"] - older_ns).any())


def leak_spec(rate=400.0, end_s=1.0):
    """A Hedge whose target is crashed from the start: every Request's entry stays (tests/test_gpu_hedge.py grows the table from one place)."""
    return hedged_link("hedge_entries_leak_behind_a_crashed_target", 0.01, 2, rate=rate, kind="constant", faults=[crash(L0, 0.0)], end_s=end_s, seed=81)


def recorded_specs():
    """Everything make_golden_hedge.py records: the fixtures, the random chains, the groups and the leak."""
    return all_specs() + [groups_spec(), leak_spec()]
