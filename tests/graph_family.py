"""The one wiring of the graph-spec families that are recorded from the live reference: rate_limiter, faults, health, resilience,
client (tests/<family>_specs.py hold the specs and each family's own result readers).  A spec's format is the union of theirs:

  n_sinks, servers, links, routers, lbs, sources           tests/strategy_specs.py
  limiters, probes, schedule, auto, windows, start_ns      tests/rate_limiter_specs.py
  faults, names                                            tests/fault_specs.py
  checkers, unhealthy                                      tests/health_specs.py
  wrappers                                                 tests/resilience_specs.py
  clients, the schedule's send / again / cancel modes      tests/client_specs.py
  flows, pre, the schedule's gate mode, a Source's stop_s  tests/flow_specs.py

and a list that a spec does not hold is an empty one.  `wire()` serves both libraries: `build()` hands it the product's classes,
tests/golden/record_family.py the reference's, so both see the same objects in the same order.  Entities: servers + lbs + routers +
links + limiters + sinks + wrappers + clients + flows + checkers -- node numbers in the recorded traces and the process-wide sort counter of
Events depend on that order and on the order of the schedule() calls below.

Each family records what the one before it records and something more; `results(spec, sim, pools, family)` reads a family's keys
off the product's objects and no others.
"""
import numpy as np

import client_specs as CS
import fault_specs as FS
import happy_simulator_amd as hs
import health_specs as HS
import rate_limiter_specs as RS
import resilience_specs as XS
import strategy_specs as SS

FAMILIES = ("rate_limiter", "faults", "health", "resilience", "client")


def make_flow(ns, i, fl, to):
    """The spec's flow entity from the namespace `ns` (the product, or the reference's industrial package)."""
    if fl["kind"] == "batch":
        return ns.BatchProcessor(f"flow{i}", to, batch_size=fl["n"], process_time=fl["pt"], timeout_s=fl["ts"])
    if fl["kind"] == "conveyor":
        return ns.ConveyorBelt(f"flow{i}", to, fl["tt"], capacity=fl["cap"])
    return ns.GateController(f"flow{i}", to, schedule=[tuple(x) for x in fl["sched"]], initially_open=fl["open"], queue_capacity=fl["cap"])


def wire(spec, F, ns):
    """The spec's objects from the factory `F` (sink, server, link, lb, router, limiter, source, probe) and the namespace `ns` (where
    Bulkhead, TimeoutWrapper, Client, the retry policies, HealthChecker and the three flow entities come from): pools by kind, every
    reference resolved once its object exists."""
    sinks = [F.sink(j) for j in range(spec["n_sinks"])]
    servers = [F.server(i, sv) for i, sv in enumerate(spec["servers"])]
    limiters = [F.limiter(i, lm) for i, lm in enumerate(spec.get("limiters") or [])]
    pools = {"sink": sinks, "server": servers, "limiter": limiters}
    links = pools["link"] = [F.link(l, lk) for l, lk in enumerate(spec["links"])]
    lbs = pools["lb"] = [F.lb(j, lb, [servers[b] for b in lb["backends"]]) for j, lb in enumerate(spec.get("lbs") or [])]
    routers = pools["router"] = [None] * len(spec["routers"])
    wrappers = pools["wrapper"] = [None] * len(spec.get("wrappers") or [])
    clients = pools["client"] = [None] * len(spec.get("clients") or [])
    flows = pools["flow"] = [None] * len(spec.get("flows") or [])

    def ref(r):
        return servers[r] if isinstance(r, int) else pools[r[0]][r[1]]

    def ready(r):
        return isinstance(r, int) or pools[r[0]][r[1]] is not None

    pending = ([("router", r) for r in range(len(routers))] + [("wrapper", i) for i in range(len(wrappers))] +
               [("client", i) for i in range(len(clients))] + [("flow", i) for i in range(len(flows))])
    while pending:
        progressed = False
        for kind, i in list(pending):
            if kind == "router" and all(ready(t) for t in spec["routers"][i]["targets"]):
                routers[i] = F.router(i, [ref(t) for t in spec["routers"][i]["targets"]])
            elif kind == "wrapper" and ready(spec["wrappers"][i]["to"]):
                w = spec["wrappers"][i]
                wrappers[i] = (ns.Bulkhead(f"bh{i}", ref(w["to"]), max_concurrent=w["mc"], max_wait_queue=w["mq"], max_wait_time=w["mw"])
                               if w["kind"] == "bulkhead" else ns.TimeoutWrapper(f"tw{i}", ref(w["to"]), timeout=w["timeout"]))
            elif kind == "client" and ready(spec["clients"][i]["to"]):
                c = spec["clients"][i]
                clients[i] = ns.Client(f"cl{i}", ref(c["to"]), timeout=c["timeout"], retry_policy=CS.make_policy(ns, c["policy"]))
            elif kind == "flow" and ready(spec["flows"][i]["to"]):
                flows[i] = make_flow(ns, i, spec["flows"][i], ref(spec["flows"][i]["to"]))
            else:
                continue
            pending.remove((kind, i))
            progressed = True
        assert progressed, "routers, wrappers, clients and flows form a cycle"
    for l, lk in enumerate(spec["links"]):
        links[l].egress = None if lk["to"] is None else ref(lk["to"])
    for i, lm in enumerate(spec.get("limiters") or []):
        limiters[i]._downstream = ref(lm["out"])
    for i, sv in enumerate(spec["servers"]):
        if sv.get("out") is not None:
            servers[i].downstream = ref(sv["out"])
    sources = pools["source"] = [F.source(k, sc, ref(sc["to"])) for k, sc in enumerate(spec["sources"])]
    probes = pools["probe"] = [F.probe(ref(on), metric, interval) for on, metric, interval in spec.get("probes") or []]
    pools["checker"] = [ns.HealthChecker(f"hc{i}", lbs[ck["lb"]], interval=ck["interval"], timeout=ck["timeout"], healthy_threshold=ck["ht"],
                                         unhealthy_threshold=ck["ut"]) for i, ck in enumerate(spec.get("checkers") or [])]
    for j, q in spec.get("unhealthy") or []:
        lbs[j].mark_unhealthy(servers[spec["lbs"][j]["backends"][q]])
    for (pool, idx), name in spec.get("names") or []:
        pools[pool][idx].name = name
    for on, what in spec.get("pre") or []:
        getattr(pools[on[0]][on[1]], what)()
    entities = servers + lbs + routers + links + limiters + sinks + wrappers + clients + flows + pools["checker"]
    return pools, sources, probes, entities


def make_schedule(ns, spec, pools):
    """(FaultSchedule, handles) of the spec from the namespace `ns`; handles marked cancel="before" are cancelled here."""
    fs = ns.FaultSchedule()
    handles = []
    for ft in spec.get("faults") or []:
        on = ft["on"]
        if not isinstance(on, str):
            x = pools[on[0]][on[1]]
            on = (x[0] if isinstance(x, tuple) else x).name           # (the product's Probe.on returns (probe, data))
        fault = ns.CrashNode(on, at=ft["at"], restart_at=ft.get("restart")) if ft["kind"] == "crash" else ns.PauseNode(on, start=ft["at"], end=ft["end"])
        h = fs.add(fault)
        if ft.get("cancel") == "before":
            h.cancel()
        handles.append(h)
    return fs, handles


def cancel_after(spec, handles):
    for ft, h in zip(spec.get("faults") or [], handles):
        if ft.get("cancel") == "after":
            h.cancel()


def fault_targets(pools):
    """Every object a fault can name, in one order for both libraries: Sources, Probes, then the entities."""
    probes = [p[0] if isinstance(p, tuple) else p for p in pools["probe"]]
    return (list(pools["source"]) + probes + list(pools["server"]) + list(pools["lb"]) + list(pools["router"]) + list(pools["link"]) +
            list(pools["limiter"]) + list(pools["sink"]) + list(pools["wrapper"]) + list(pools["client"]) + list(pools["flow"]) +
            list(pools["checker"]))


def early_starts(spec, pools):
    """The start() Events of the checkers with early=True, made before the Simulation exists."""
    return [[hc.start() for _ in range(ck.get("starts", 1))] if ck.get("early") else []
            for ck, hc in zip(spec.get("checkers") or [], pools["checker"])]


def schedule_all(spec, pools, sim, event_cls, at, early_events):
    """The spec's `schedule` list (tests/client_specs.py has the three modes of a Client's entries, tests/flow_specs.py the "gate"
    mode: every Event of the gate's start_events()), then sim.schedule(checker.start()) as the spec says, on `sim`, for either library."""
    last, cancel = None, []
    for on, t_s, *mode in spec.get("schedule") or []:
        target = pools[on[0]][on[1]]
        mode = mode[0] if mode else "plain"
        if mode == "again":
            sim.schedule(last)
            continue
        if mode == "gate":
            for ev in target.start_events():
                sim.schedule(ev)
            continue
        if mode == "start":                              # (tests/mixed_specs.py: a checker started in the middle of the list)
            sim.schedule(target.start())
            continue
        if mode == "plain":
            last = event_cls(time=at(t_s), event_type="Request", target=target)
        else:
            last = target.send_request()
            last.time = at(t_s)
        sim.schedule(last)
        if mode == "cancel":
            cancel.append(last)
    for ev in cancel:
        ev.cancel()
    for ck, hc, early in zip(spec.get("checkers") or [], pools["checker"], early_events):
        for ev in early:
            sim.schedule(ev)
        for _ in range(0 if ck.get("early") else ck.get("starts", 1)):
            sim.schedule(hc.start())
        if ck.get("stop"):
            hc.stop()


class Product:
    """wire()'s factory over the product's classes."""

    @staticmethod
    def sink(j):
        return hs.Sink(f"sink{j}")

    @staticmethod
    def server(i, sv):
        return hs.Server(f"srv{i}", concurrency=sv.get("c", 1), queue_capacity=sv.get("cap"),
                         service_time=hs.ConstantLatency(sv["mean"]) if sv.get("svc") == "const" else hs.ExponentialLatency(sv["mean"]))

    @staticmethod
    def limiter(i, lm):
        return hs.RateLimitedEntity(f"lim{i}", None, RS.make_policy(hs, lm["policy"]), queue_capacity=lm["cap"])

    @staticmethod
    def link(l, lk):
        jit = None
        if lk.get("jm") is not None and lk.get("jk") == "exp":
            jit = hs.ExponentialLatency(lk["jm"])
        elif lk.get("jm") is not None and lk.get("jk") == "const":
            jit = hs.ConstantLatency(lk["jm"])
        return hs.NetworkLink(f"link{l}", latency=hs.ConstantLatency(lk["lat"]), jitter=jit, packet_loss_rate=lk.get("loss", 0.0), egress=None)

    @staticmethod
    def lb(j, lb, backends):
        return SS.make_lb(hs.LoadBalancer, j, lb, backends, SS.make_strategy(lb))

    @staticmethod
    def router(r, targets):
        return hs.RandomRouter(f"router{r}", targets=targets)

    @staticmethod
    def source(k, sc, to):
        make = hs.Source.poisson if sc["kind"] == "poisson" else hs.Source.constant
        if sc.get("n_clients"):
            return make(rate=sc["rate"], event_provider=hs.ClientKeyEventProvider(to, n_clients=sc["n_clients"]), name=f"src{k}")
        return make(rate=sc["rate"], target=to, name=f"src{k}",
                    **({} if sc.get("stop_s") is None else {"stop_after": hs.Instant.from_seconds(sc["stop_s"])}))

    @staticmethod
    def probe(target, metric, interval):
        return hs.Probe.on(target, metric, interval=interval)


def build(spec, seed=None, **sim_kw):
    """(Simulation, entities by pool) of the product, wired like the recorded reference run."""
    pools, sources, probes, entities = wire(spec, Product, hs)
    start_ns = int(spec.get("start_ns", 0))

    def at(t_s):
        return hs.Instant(start_ns + hs.Instant.from_seconds(t_s).nanoseconds)

    fs, handles = make_schedule(hs, spec, pools)          # (without faults: an empty schedule, which the Simulation takes for none)
    early = early_starts(spec, pools)
    # (max_graph_events: a run that never ends -- see rate_limiter_specs._fixtures on FixedWindowPolicy -- is refused after 400 000
    #  events, not minutes)
    sim = hs.Simulation(sources=sources, entities=entities, seed=spec["seed"] if seed is None else seed, max_graph_events=400_000,
                        fault_schedule=fs, **({} if spec.get("auto") else {"end_time": at(spec["end_s"])}),
                        **({"start_time": hs.Instant(start_ns)} if start_ns else {}), **({"probes": [p for p, _ in probes]} if probes else {}),
                        **sim_kw)
    cancel_after(spec, handles)
    schedule_all(spec, pools, sim, hs.Event, at, early)
    pools["probes"] = probes
    pools["fault_schedule"], pools["handles"] = fs, handles
    return sim, pools


def results(spec, sim, pools, family):
    """Everything record_family.run_case records for `family` except the trace, read off the product's objects after run()."""
    level = FAMILIES.index(family)
    ents = dict(sources=pools["source"], servers=pools["server"], links=pools["link"], routers=pools["router"], sinks=pools["sink"],
                lbs=pools["lb"], probes=pools["probes"])
    out = SS.results(spec, sim, ents)
    out.pop("sink_created_ns")
    out.update(RS.limiter_results(pools["limiter"]))
    out["lim_events"] = np.array([x._events for x in pools["limiter"]], np.int64).reshape(-1, 2)
    if family == "rate_limiter":
        return out
    out.update(FS.fault_results(pools["fault_schedule"], fault_targets(pools)))
    if level >= 2:
        out.update(HS.health_results(spec, pools))        # (lb_current_weights with the backends no select() ever saw, and their mask)
    if level >= 3:
        out.update(XS.wrapper_results(pools))
    if level >= 4:
        out.update(CS.client_results(pools))
    if family != "health":
        out["fault_events"] = int(getattr(sim, "_fault_events_processed", 0))
    out["internal_by_kind"] = np.asarray(sim._internal_by_kind, np.int64)            # limiter Requests, limiter polls, fault set, fault clear
    if level >= 2:
        out["health_by_kind"] = np.asarray(getattr(sim, "_health_by_kind", np.zeros(3)), np.int64)              # cycle, response, timeout
    if level >= 3:
        # Bulkhead request / response / timeout, then TimeoutWrapper's
        out["resilience_by_kind"] = np.asarray(getattr(sim, "_resilience_by_kind", np.zeros(6)), np.int64)
    if level >= 4:
        out["client_by_kind"] = np.asarray(sim._client_by_kind, np.int64)            # Client request / response / timeout
    out["events_cancelled"] = int(sim.summary.events_cancelled)
    return out
