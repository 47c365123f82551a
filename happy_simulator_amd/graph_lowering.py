"""`sources` / `entities` / `probes` of a Simulation -> the node arrays of the single-heap engine: lower_general().

It collects the nodes, builds the AutoScalers' and deployers' instance pools, lowers every node with the function of its kind (`_LOWER`)
and assembles what spans nodes; every refusal of the single-heap path (lowering.UnsupportedTopology) is decided here, in that order.

Entity streams (DESIGN.md section 3 -- the one definition that is the engine's own): the k-th Source of `sources=[...]` draws
ARRIVAL from stream base k; the s-th Server / l-th NetworkLink / r-th RandomRouter in node order (entities in `entities=[...]`
order, then whatever is only reachable downstream, in discovery order) draws SERVICE / LINK + LOSS / ROUTE from base s / l / r.
For a graph built station by station this is the numbering of the station engines.  The Servers of an instance pool go on
behind the Simulation's own: instance k draws from base (own Servers) + k - 1.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from .core.temporal import Duration
from .entities import (LIMITER_POLICIES, METRIC_EVALUATORS, QUEUE_POLICIES, SCALING_POLICIES, AdaptiveLIFO, AutoScaler, BatchProcessor,
                       Bulkhead, CanaryDeployer, Client, ClientKeyEventProvider, CoDelQueue, ConsistentHash, ConstantLatency,
                       ConstantRateProfile, ConveyorBelt, Counter, DecorrelatedJitter, Entity, ExponentialBackoff, ExponentialLatency,
                       Fallback, FIFOQueue, FixedRetry, GateController, HealthChecker, Hedge, InventoryBuffer, IPHash, LatencyEvaluator, LatencyTracker,
                       LeastConnections, LinearRampProfile, LoadBalancer, Network, NetworkLink, NoRetry, PooledCycleResource, Probe, Random, RandomRouter,
                       RateLimitedEntity,
                       RollingDeployer, RoundRobin, Server, SimpleEventProvider, Sink, SlidingWindowPolicy, Source, StepScaling,
                       TargetUtilization, TimeoutWrapper, TokenBucketPolicy, WeightedLeastConnections, WeightedRoundRobin)
from .graph_arrays import GraphArrays, _offsets
from .graph_engine import GeneralGraph
from .lowering import UnsupportedTopology

_STRATEGY_CODE = ((ConsistentHash, N.LB_CONSISTENT_HASH), (RoundRobin, N.LB_ROUND_ROBIN), (Random, N.LB_RANDOM),
                  (WeightedRoundRobin, N.LB_WEIGHTED_ROUND_ROBIN), (IPHash, N.LB_IP_HASH), (LeastConnections, N.LB_LEAST_CONNECTIONS),
                  (WeightedLeastConnections, N.LB_WEIGHTED_LEAST_CONNECTIONS))

_SINKS = (Sink, Counter, LatencyTracker)
_FLOWS = (BatchProcessor, ConveyorBelt, GateController)
_STOCK = (PooledCycleResource, InventoryBuffer)
_DEPLOYERS = (RollingDeployer, CanaryDeployer)
_FLOW_METRIC_OF = {"buffer_depth": BatchProcessor, "items_in_transit": ConveyorBelt, "queue_depth": GateController}
_STOCK_METRIC_OF = {"available": PooledCycleResource, "active": PooledCycleResource, "queued": PooledCycleResource, "stock": InventoryBuffer}
_LOWERED = (Server, NetworkLink, RandomRouter, LoadBalancer, RateLimitedEntity, HealthChecker, Bulkhead, TimeoutWrapper, Client,
            BatchProcessor, ConveyorBelt, GateController, AutoScaler, RollingDeployer, CanaryDeployer, Hedge, Fallback) + _STOCK + _SINKS
_FIXED_LIST = (ConsistentHash, IPHash, Random)            # strategies whose selection over a changing backend list is not lowered


def client_delay_table(policy, what: str) -> np.ndarray:
    """Duration.from_seconds(policy.get_delay(a)) in whole nanoseconds for a = 1 .. max_attempts - 1: what a Client's timeout handler
    adds to `now` for the retry of attempt a (client.py:393-410).  The device never evaluates a policy."""
    if type(policy) is NoRetry:
        return np.zeros(0, np.int64)
    if type(policy) is DecorrelatedJitter:
        raise UnsupportedTopology(f"{what}: DecorrelatedJitter draws from the process-wide random generator (not lowered; a follow-up)")
    if type(policy) not in (FixedRetry, ExponentialBackoff):
        raise UnsupportedTopology(f"{what}: retry policy {type(policy).__name__} is not lowered (NoRetry, FixedRetry, ExponentialBackoff are)")
    if type(policy) is ExponentialBackoff and policy.jitter > 0:
        raise UnsupportedTopology(f"{what}: ExponentialBackoff(jitter={policy.jitter}) draws from the process-wide random generator "
                                  "(not lowered; a follow-up)")
    if policy.max_attempts > Client.MAX_ATTEMPTS:
        raise UnsupportedTopology(f"{what}: max_attempts = {policy.max_attempts} is beyond the {Client.MAX_ATTEMPTS} attempts the engine's "
                                  "key holds")
    out = np.zeros(policy.max_attempts - 1, np.int64)
    for k in range(len(out)):
        try:
            ns = Duration.from_seconds(policy.get_delay(k + 1)).nanoseconds
            if not 0 <= ns < (1 << 62):
                raise OverflowError(ns)
        except (OverflowError, ValueError, TypeError) as e:
            raise UnsupportedTopology(f"{what}: the delay of attempt {k + 1} cannot be evaluated as a Duration "
                                      f"({type(e).__name__}: {e})") from None
        out[k] = ns
    return out


def flow_delay_ns(seconds, what: str, name: str) -> int:
    """int(seconds * 1_000_000_000): what `Instant + seconds` adds to `now` (core/temporal.py:213-222) -- it does not depend on `now`,
    so the device gets whole nanoseconds."""
    try:
        ns = int(seconds * 1_000_000_000)
    except (OverflowError, ValueError, TypeError) as e:
        raise UnsupportedTopology(f"{what}: {name} = {seconds!r} cannot be added to an Instant ({type(e).__name__}: {e})") from None
    if not 0 <= ns < (1 << 61):
        raise UnsupportedTopology(f"{what}: {name} = {seconds!r} is outside [0, 2^61) ns")
    return ns


def scaler_pool_size(scaler: "AutoScaler", n_initial: int, start_ns: int, end_ns: int, starts: int = 1) -> int:
    """P: a bound on the instances `scaler` can create in a run from start_ns to end_ns ("AutoScaler").  Evaluations
    happen at the instants start + j * interval; the run processes the ones up to its end and at most one Event beyond it:
    I = (end - start) // interval + 2 instants.  A scale-out adds at most max_instances - current and only managed instances ever
    leave, so current >= n_initial: a run of scale-outs without a scale-in between them adds at most A = max_instances - n_initial.
    A new such run begins only behind a scale-in, which follows the last scale-out by the scale-in cooldown and is followed by the
    next scale-out by the scale-out cooldown: with one action per instant the runs begin at least g_in + g_out instants apart (a
    cooldown of c > 0 seconds keeps max(1, c // interval - 1) instants free, a cooldown <= 0 none -- but one chain of evaluations acts
    once per instant).  R = 1 + (I - 1) // (g_in + g_out) runs, P = R * A.  Several start() Events with a cooldown <= 0 act several
    times per instant: every evaluation may then begin a run, R = I * starts."""
    iv_ns = Duration.from_seconds(scaler._evaluation_interval).nanoseconds
    instants = max(0, end_ns - start_ns) // iv_ns + 2
    most = scaler._max_instances - n_initial
    if most <= 0:
        return 0

    def gap(cooldown):
        return 0 if not cooldown > 0 else max(1, int(cooldown * 1e9) // iv_ns - 1)

    g_out, g_in = gap(scaler._scale_out_cooldown), gap(scaler._scale_in_cooldown)
    if starts <= 1 or (g_out > 0 and g_in > 0):
        runs = 1 + (instants - 1) // (max(g_out, 1) + max(g_in, 1))
    else:
        runs = instants * starts
    return int(runs * most)


def deployer_pool_size(n_initial: int, deploys: int) -> int:
    """P: a bound on the instances a RollingDeployer can create over `deploys` scheduled deploy() Events ("Deployers").
    Every instance takes one entry out of `_old_backends`, and entries come into that list only at a `_rolling_deploy_start`, which
    copies the LoadBalancer's members: deployment j creates at most n_j instances, n_j <= n_initial + n_1 + .. + n_(j-1) (the initial
    backends and every instance made so far), so n_j <= n_initial * 2^(j-1) and P = n_initial * (2^deploys - 1).  No horizon enters."""
    return int(n_initial) * ((1 << min(int(deploys), 62)) - 1)


class _Lowering:
    """What the steps of one lower_general() share: the node list, the pools, the arrays and what spans nodes of several kinds."""

    def __init__(self, start_ns: int, end_ns: int | None, scaler_starts: int, deploys: dict | None):
        self.start_ns, self.end_ns, self.scaler_starts, self.deploys = start_ns, end_ns, scaler_starts, deploys or {}
        self.nodes, self.node_of = [], {}                         # entities by node id; id(entity) -> node id
        self.n_src = self.n_front = 0                             # Sources are nodes 0 .. n_src - 1, Probes n_src .. n_front - 1
        self.n_own = self.n_own_servers = 0                       # the Simulation's own nodes / Servers: the pools stand behind them
        self.scaled: dict[int, tuple] = {}                        # id(LoadBalancer) -> (its scaler or deployer, its initial backends, the pool)
        self.pool_of: dict[int, tuple] = {}                       # pool node -> (its scaler or deployer, its instance id k)
        self.a, self.rt = None, []                                # the GraphArrays once the nodes are known; rt_targets so far
        self.counters = {Server: 0, NetworkLink: 0, RandomRouter: 0}     # the next stream base per kind
        self.weights: dict[int, list[int]] = {}                   # rt offset -> the weights of a weighted strategy's backends
        self.policies_seen: dict[int, str] = {}                   # id(policy) -> the limiter that holds it
        self.checked: dict[int, str] = {}                         # id(LoadBalancer) -> its HealthChecker
        self.unhealthy: dict[int, list[int]] = {}                 # rt offset -> is_healthy of a LoadBalancer's backends, one of them unhealthy
        self.client_delays = None                                 # per node: a Client's delay table in ns

    def add(self, ent) -> int:
        if id(ent) not in self.node_of:
            self.node_of[id(ent)] = len(self.nodes)
            self.nodes.append(ent)
        return self.node_of[id(ent)]

    def stream(self, kind) -> int:
        self.counters[kind] += 1
        return self.counters[kind] - 1


def _ensure(a, name: str, make):
    """`a.name`, made by `make()` when a first node needs it."""
    v = getattr(a, name)
    if v is None:
        v = make()
        setattr(a, name, v)
    return v


def _takes_no_requests(cx: _Lowering, ent) -> bool:
    return isinstance(ent, (Source, Probe, HealthChecker)) or not isinstance(ent, Entity) or id(ent) not in cx.node_of


def _strategy_refusal(what: str, lb, under: str) -> UnsupportedTopology:
    return UnsupportedTopology(f"{what}: strategy {type(lb.strategy).__name__} of '{lb.name}' is not lowered under {under} (its "
                               "selection over a changing backend list is a follow-up: RoundRobin, WeightedRoundRobin, "
                               "LeastConnections and WeightedLeastConnections are)")


def _refuse_unhealthy(what: str, lb, under: str) -> None:
    if lb.unhealthy_backends:
        raise UnsupportedTopology(f"{what}: backend '{lb.unhealthy_backends[0].name}' of '{lb.name}' is marked unhealthy -- health marks "
                                  f"under {under} are not lowered (a follow-up)")


def _refuse_checked(cx: _Lowering, what: str, lb, other: str) -> None:
    """An AutoScaler or a deployer (`other`, with its article) on a LoadBalancer that a HealthChecker watches."""
    if id(lb) in cx.checked:
        raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the HealthChecker '{cx.checked[id(lb)]}' -- a "
                                  f"HealthChecker and {other} on one LoadBalancer are not lowered (a follow-up)")


def _check_receiver(ent, where: str) -> None:
    """`ent` as an entity of the Simulation (`where` = "entities") or as what another one forwards to."""
    if isinstance(ent, Source):
        raise UnsupportedTopology(f"{where}: a Source takes no Requests")
    if isinstance(ent, Network):
        # (routing by an Event's source / destination metadata, Network.handle_event, is not lowered: traffic goes to the links)
        raise UnsupportedTopology(f"{where}: an Event aimed at the Network '{ent.name}' is not lowered (a Network is a registry of "
                                  "links here: send to the link itself)")
    if isinstance(ent, NetworkLink) and ent._reverse_of is not None:
        raise UnsupportedTopology(f"{where}: link '{ent.name}' is the reverse copy add_bidirectional_link made of "
                                  f"'{ent._reverse_of.name}' -- it shares its jitter object and its loss stream with the forward link "
                                  "(not lowered)")
    if isinstance(ent, (HealthChecker, AutoScaler) + _DEPLOYERS) and where != "entities":
        kind_ = "HealthChecker" if isinstance(ent, HealthChecker) else "AutoScaler" if isinstance(ent, AutoScaler) else type(ent).__name__
        raise UnsupportedTopology(f"{where}: the {kind_} '{ent.name}' takes no Requests")
    if not isinstance(ent, _LOWERED):
        raise UnsupportedTopology(f"{where}: {type(ent).__name__} '{getattr(ent, 'name', ent)}' is not lowered to the engine")


def _collect_nodes(cx: _Lowering, sources, entities, probes) -> None:
    """The node list: Sources in `sources=[...]` order, PROBE nodes behind them in `probes=[...]` order, the entities, then whatever
    is only reachable downstream (the reference never needs it listed: events carry their target), in discovery order."""
    nodes, node_of = cx.nodes, cx.node_of
    for what, cls, listed in (("source", Source, sources), ("probe", Probe, probes)):
        for x in listed or []:
            if not isinstance(x, cls):
                raise UnsupportedTopology(f"{what} {type(x).__name__} is not a lowered {cls.__name__}")
            if id(x) in node_of:
                raise UnsupportedTopology(f"{what} '{x.name}' is listed twice")
            cx.add(x)
        if cls is Source:
            cx.n_src = len(nodes)
    cx.n_front = len(nodes)
    for ent in entities or []:
        if isinstance(ent, Source):
            if id(ent) not in node_of:
                raise UnsupportedTopology(f"source '{ent.name}' is listed in entities but not in sources: it would never start")
            continue
        if not isinstance(ent, Entity):
            raise UnsupportedTopology(f"object {ent!r} is not an Entity")
        if isinstance(ent, Network):
            cx.add(ent)                                       # its place in the entity order; nothing forwards to it (_check_receiver)
            continue
        _check_receiver(ent, "entities")
        cx.add(ent)
    k = 0
    while k < len(nodes):
        ent = nodes[k]
        k += 1
        if isinstance(ent, (Probe, HealthChecker, AutoScaler) + _DEPLOYERS):    # (their LoadBalancer has to be part of the Simulation by itself)
            continue
        for d in ent.downstream_entities():
            if d is None:
                continue
            _check_receiver(d, f"'{ent.name}' forwards to it")
            if isinstance(d, Server) and id(d) not in node_of:
                # (the reference hands a clock to what `entities` lists: an unlisted Server would fail on its first event)
                raise UnsupportedTopology(f"'{ent.name}' forwards to server '{d.name}', which is not listed in `entities` of this "
                                          "Simulation (not part of this Simulation)")
            cx.add(d)
    cx.n_own = len(nodes)
    cx.n_own_servers = sum(isinstance(x, Server) for x in nodes)


def _scaler_pool(cx: _Lowering, sc, what: str, lb, n_initial: int) -> int:
    """The refusals of an AutoScaler as the owner of a pool; the pool's size."""
    if id(lb) in cx.scaled:
        raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the scaler '{cx.scaled[id(lb)][0].name}' already (one AutoScaler "
                                  "per LoadBalancer is lowered)")
    if isinstance(lb.strategy, _FIXED_LIST):
        raise _strategy_refusal(what, lb, "an AutoScaler")
    pol = sc.policy
    if type(pol) not in SCALING_POLICIES:
        raise UnsupportedTopology(f"{what}: policy {type(pol).__name__} is not lowered to the engine (lowered: TargetUtilization, "
                                  "StepScaling, QueueDepthScaling)")
    if isinstance(pol, StepScaling) and len(pol._steps) > AutoScaler.MAX_STEPS:
        raise UnsupportedTopology(f"{what}: StepScaling with {len(pol._steps)} steps is beyond the {AutoScaler.MAX_STEPS} the engine "
                                  "holds (AutoScaler.MAX_STEPS)")
    _refuse_unhealthy(what, lb, "an AutoScaler")
    for v, nm in ((sc._min_instances, "min_instances"), (sc._max_instances, "max_instances")):
        if type(v) is not int or not -(1 << 30) < v < (1 << 30):
            raise UnsupportedTopology(f"{what}: {nm} must be an int below 2^30, got {v!r}")
    try:
        ok = np.isfinite(sc._evaluation_interval) and sc._evaluation_interval * 1e9 >= 1.0
        float(sc._scale_out_cooldown), float(sc._scale_in_cooldown)
    except (TypeError, ValueError):
        ok = False
    if not ok or sc._scale_out_cooldown != sc._scale_out_cooldown or sc._scale_in_cooldown != sc._scale_in_cooldown:
        raise UnsupportedTopology(f"{what}: evaluation_interval = {sc._evaluation_interval!r} (below one nanosecond or not finite) or "
                                  "a cooldown that is no number is not lowered")
    if cx.end_ns is None:
        raise UnsupportedTopology(f"{what}: end_time = Infinity leaves no horizon to size its instance pool by; pass end_time/duration")
    size = scaler_pool_size(sc, n_initial, cx.start_ns, cx.end_ns, cx.scaler_starts)
    if size > AutoScaler.MAX_POOL:
        raise UnsupportedTopology(f"{what}: the run could create up to {size} instances, beyond the pool of {AutoScaler.MAX_POOL} "
                                  "per scaler (AutoScaler.MAX_POOL): a longer interval or cooldown, or a shorter run")
    return size


def _canary_refusals(cx: _Lowering, dp, what: str) -> None:
    ev = dp._metric_evaluator
    if type(ev) not in METRIC_EVALUATORS:
        raise UnsupportedTopology(f"{what}: metric evaluator {type(ev).__name__} is not lowered to the engine (lowered: "
                                  "ErrorRateEvaluator, LatencyEvaluator)")
    if len(dp._stages) > CanaryDeployer.MAX_STAGES:
        raise UnsupportedTopology(f"{what}: {len(dp._stages)} stages are beyond the {CanaryDeployer.MAX_STAGES} the engine holds "
                                  "(CanaryDeployer.MAX_STAGES)")
    for k, st_ in enumerate(dp._stages):
        try:
            ok = bool(np.isfinite(st_.traffic_percentage)) and bool(np.isfinite(st_.evaluation_period))
        except (TypeError, ValueError, AttributeError):
            ok = False
        if not ok:
            raise UnsupportedTopology(f"{what}: stage {k} has a traffic_percentage or evaluation_period that is no finite number")
    try:
        ok = bool(np.isfinite(dp._evaluation_interval)) and dp._evaluation_interval > 0 and dp._evaluation_interval * 1e9 >= 1.0
        lim_, mult_ = ((ev._max_latency if isinstance(ev, LatencyEvaluator) else ev._max_error_rate), ev._threshold_multiplier)
        ok = ok and float(lim_) == float(lim_) and float(mult_) == float(mult_)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise UnsupportedTopology(f"{what}: evaluation_interval = {dp._evaluation_interval!r} must be a finite number of at least one "
                                  "nanosecond (and the evaluator's limits numbers)")
    if cx.deploys.get(id(dp), 1) > 1:
        raise UnsupportedTopology(f"{what}: {cx.deploys.get(id(dp), 1)} deploy() Events are scheduled -- a second canary of the same name is never "
                                  "registered by the LoadBalancer (one deploy() per CanaryDeployer is lowered)")


def _rolling_refusals(dp, what: str) -> None:
    for v, nm, least in ((dp._batch_size, "batch_size", 1), (dp._healthy_threshold, "healthy_threshold", 1), (dp._max_failures, "max_failures", None)):
        if type(v) is not int or not -(1 << 30) < v < (1 << 30) or (least is not None and v < least):
            raise UnsupportedTopology(f"{what}: {nm} must be an int{'' if least is None else f' of at least {least}'} below 2^30, got {v!r}")
    try:
        ok = bool(np.isfinite(dp._health_check_interval)) and dp._health_check_interval > 0 and dp._health_check_interval * 1e9 >= 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise UnsupportedTopology(f"{what}: health_check_interval = {dp._health_check_interval!r} must be a finite number of at least "
                                  "one nanosecond")


def _deployer_pool(cx: _Lowering, dp, what: str, lb, n_initial: int) -> int:
    """The refusals of a RollingDeployer or a CanaryDeployer as the owner of a pool; the pool's size (a canary is one instance)."""
    if id(lb) in cx.scaled:
        other = cx.scaled[id(lb)][0]
        raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the {type(other).__name__} '{other.name}' already (a deployer next "
                                  "to an AutoScaler or another deployer on one LoadBalancer is not lowered: a follow-up)")
    if not isinstance(lb.strategy, (RoundRobin, WeightedRoundRobin, LeastConnections, WeightedLeastConnections)):
        raise _strategy_refusal(what, lb, "a deployer")
    _refuse_unhealthy(what, lb, "a deployer")
    if not isinstance(dp, RollingDeployer):
        _canary_refusals(cx, dp, what)
        return 1
    _rolling_refusals(dp, what)
    n_deploys = cx.deploys.get(id(dp), 1)
    size = deployer_pool_size(n_initial, n_deploys)
    if size > RollingDeployer.MAX_POOL:
        raise UnsupportedTopology(f"{what}: {n_deploys} deploy() Events over {n_initial} backends could create up to {size} instances, "
                                  f"beyond the pool of {RollingDeployer.MAX_POOL} per deployer (RollingDeployer.MAX_POOL)")
    return size


def _build_pools(cx: _Lowering) -> None:
    """The instance pools of the AutoScalers, then of the deployers: the factory's results for instances 1 .. P, dormant Server nodes
    behind all of the Simulation's own nodes (node numbers keep their meaning), targets of their LoadBalancer behind its initial
    backends."""
    node_of = cx.node_of
    owners = [x for x in cx.nodes if isinstance(x, AutoScaler)] + [x for x in cx.nodes if isinstance(x, _DEPLOYERS)]
    for owner in owners:
        what, size_of = ((f"auto scaler '{owner.name}'", _scaler_pool) if isinstance(owner, AutoScaler) else
                         (f"{'rolling' if isinstance(owner, RollingDeployer) else 'canary'} deployer '{owner.name}'", _deployer_pool))
        lb = owner.load_balancer
        if not isinstance(lb, LoadBalancer) or id(lb) not in node_of:
            raise UnsupportedTopology(f"{what}: its LoadBalancer is not an entity of this Simulation")
        initial = lb.all_backends
        pool = []
        for k in range(1, size_of(cx, owner, what, lb, len(initial)) + 1):
            inst = owner._instance(k)
            if not isinstance(inst, Server):
                raise UnsupportedTopology(f"{what}: server_factory returned a {type(inst).__name__} for instance {k}: only Servers may stand "
                                          "as a LoadBalancer's backends")
            if id(inst) in node_of:
                raise UnsupportedTopology(f"{what}: server_factory returned '{inst.name}' for instance {k}, which is an entity of this "
                                          "Simulation or another instance already (one new Server per call)")
            d = inst.downstream
            if d is not None and (id(d) not in node_of or node_of[id(d)] >= cx.n_own):
                raise UnsupportedTopology(f"{what}: the downstream '{getattr(d, 'name', d)}' of instance {k} is not an entity of this "
                                          "Simulation")
            cx.pool_of[cx.add(inst)] = (owner, k)
            pool.append(inst)
        cx.scaled[id(lb)] = (owner, initial, pool)


def _lower_source(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    ep, prov = ent._event_provider, ent._time_provider
    if not isinstance(ep, (SimpleEventProvider, ClientKeyEventProvider)):
        raise UnsupportedTopology(f"source '{ent.name}': event provider {type(ep).__name__} is not lowered on a general graph")
    tgt = ep._target
    n_clients = getattr(ep, "_n_clients", 0)
    if isinstance(tgt, LoadBalancer) and isinstance(tgt.strategy, Random):
        n_clients = len(tgt.all_backends)             # the Request's draw IS the choice: backends[int(u * len)] (entities.Random)
    if n_clients:
        _ensure(a, "src_n_clients", lambda: np.zeros(a.n, np.int64))[i] = n_clients
    if not (ent.rate > 0):
        raise UnsupportedTopology(f"source '{ent.name}': rate must be > 0")
    if not isinstance(tgt, Entity) or id(tgt) not in cx.node_of:
        raise UnsupportedTopology(f"source '{ent.name}' has no lowered target")
    a.kind[i] = N.NODE_SOURCE
    a.target[i] = cx.node_of[id(tgt)]
    a.stream_base[i] = i                              # (Sources are nodes 0 .. n_src - 1, in `sources` order)
    a.src_kind[i] = N.SRC_POISSON if prov.kind == "poisson" else N.SRC_CONSTANT
    a.src_rate[i] = float(prov.profile.peak_rate)
    a.src_stop_after_ns[i] = -1 if ep._stop_after is None else ep._stop_after.nanoseconds
    pr = prov.profile
    if not isinstance(pr, ConstantRateProfile):        # its ticks come from the tick-table kernel, like the station engines'
        kinds = _ensure(a, "src_profile_kind", lambda: np.zeros(a.n, np.uint8))
        params = _ensure(a, "src_profile_params", lambda: np.zeros((a.n, 4), np.float64))
        if isinstance(pr, LinearRampProfile):
            kinds[i] = N.PROF_LINEAR_RAMP
            params[i, :3] = (pr.duration_s, pr.start_rate, pr.end_rate)
        else:
            kinds[i] = N.PROF_SPIKE
            params[i] = (pr.baseline_rate, pr.spike_rate, pr.warmup_s, pr.spike_duration_s)


def _lower_probe(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    m = Probe.engine_metric(ent.metric)
    tgt = ent.target
    on_wrapper = isinstance(tgt, (Bulkhead, TimeoutWrapper)) and m in N.PROBE_WRAPPER_METRICS
    on_client = isinstance(tgt, Client) and m in N.PROBE_CLIENT_METRICS
    on_hedge = isinstance(tgt, Hedge) and m in N.PROBE_HEDGE_METRICS
    want = None                                       # the class whose attribute the metric is, where the metric alone does not say
    if isinstance(tgt, AutoScaler) and m in N.PROBE_SCALER_METRICS:
        codes = N.PROBE_SCALER_METRICS
    elif on_hedge:
        codes = N.PROBE_HEDGE_METRICS
    elif isinstance(tgt, _FLOW_METRIC_OF.get(m, ())):
        codes = N.PROBE_FLOW_METRICS
    elif isinstance(tgt, _STOCK_METRIC_OF.get(m, ())):
        codes = N.PROBE_STOCK_METRICS
    else:
        if m not in N.PROBE_METRICS and not on_wrapper and not on_client:
            raise UnsupportedTopology(f"probe '{ent.name}': metric '{ent.metric}' is not sampled on the engine")
        codes = N.PROBE_CLIENT_METRICS if on_client else N.PROBE_WRAPPER_METRICS if on_wrapper else N.PROBE_METRICS
        want = (Client if on_client else (TimeoutWrapper if m == "in_flight_count" else Bulkhead) if on_wrapper
                else Source if m == "generated_count" else _SINKS if m == "events_received"
                else RateLimitedEntity if m == "queue_depth" else Server)
    if id(tgt) not in cx.node_of:
        raise UnsupportedTopology(f"probe '{ent.name}': its target is not an entity of this Simulation")
    if want is not None and not isinstance(tgt, want):
        raise UnsupportedTopology(f"probe '{ent.name}': metric '{ent.metric}' is not an attribute of {type(tgt).__name__}")
    a.kind[i] = N.NODE_PROBE
    a.target[i] = cx.node_of[id(tgt)]
    _ensure(a, "probe_metric", lambda: np.full(a.n, N.PROBE_NONE, np.uint8))[i] = codes[m]
    _ensure(a, "probe_interval_s", lambda: np.ones(a.n, np.float64))[i] = ent.interval


def _lower_server(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    svc = ent.service_time
    if not isinstance(svc, (ExponentialLatency, ConstantLatency)):
        raise UnsupportedTopology(f"server '{ent.name}': service distribution {type(svc).__name__} is not lowered")
    a.kind[i] = N.NODE_SERVER
    # instance k of a pool: the Servers' numbering goes on behind the Simulation's own
    a.stream_base[i] = cx.n_own_servers + cx.pool_of[i][1] - 1 if i in cx.pool_of else cx.stream(Server)
    a.concurrency[i] = ent.concurrency
    a.lat_kind[i] = N.LAT_EXPONENTIAL if isinstance(svc, ExponentialLatency) else N.LAT_CONSTANT
    a.lat_mean_s[i] = svc.mean
    pol = ent._policy
    cap = pol.capacity
    a.queue_cap[i] = -1 if cap == float("inf") else int(cap)
    if isinstance(pol, QUEUE_POLICIES):
        params = _ensure(a, "qp_params", lambda: np.zeros((a.n, 5), np.float64))
        if len(pol):
            raise UnsupportedTopology(f"server '{ent.name}': {len(pol)} items are still queued in its {type(pol).__name__} from an "
                                      "earlier run (not lowered)")
        if cap != float("inf") and not (type(cap) is int and 0 <= cap < (1 << 31)):
            raise UnsupportedTopology(f"server '{ent.name}': the capacity {cap!r} of its {type(pol).__name__} is not an int below 2^31")
        if isinstance(pol, AdaptiveLIFO):
            if type(pol.congestion_threshold) is not int:
                raise UnsupportedTopology(f"server '{ent.name}': congestion_threshold must be an int, got {pol.congestion_threshold!r}")
            params[i] = (N.QUEUE_ADAPTIVE_LIFO, a.queue_cap[i], min(pol.congestion_threshold, 1 << 40), 0.0, 0.0)
        elif isinstance(pol, CoDelQueue):
            target, interval = float(pol.target_delay), float(pol.interval)
            if not (target < float("inf") and interval <= 4.0e9):
                raise UnsupportedTopology(f"server '{ent.name}': CoDelQueue(target_delay={target!r}, interval={interval!r}) is beyond "
                                          "4e9 s or not finite")
            params[i] = (N.QUEUE_CODEL, a.queue_cap[i], 0, target, interval)
        else:
            params[i] = (N.QUEUE_LIFO, a.queue_cap[i], 0, 0.0, 0.0)
    elif not isinstance(pol, FIFOQueue):
        raise UnsupportedTopology(f"server '{ent.name}': queue policy {type(pol).__name__} is not lowered")
    d = ent.downstream
    a.target[i] = -1 if d is None else cx.node_of[id(d)]


def _lower_link(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    if not isinstance(ent.latency, ConstantLatency) or not (ent.latency.mean >= 0):
        raise UnsupportedTopology(f"link '{ent.name}': the base latency must be a ConstantLatency >= 0")
    if ent.jitter is not None and not isinstance(ent.jitter, (ExponentialLatency, ConstantLatency)):
        raise UnsupportedTopology(f"link '{ent.name}': jitter {type(ent.jitter).__name__} is not lowered")
    a.kind[i] = N.NODE_LINK
    a.stream_base[i] = cx.stream(NetworkLink)
    a.link_lat_min_s[i] = ent.latency.mean
    if ent.jitter is not None:
        a.lat_kind[i] = N.LAT_EXPONENTIAL if isinstance(ent.jitter, ExponentialLatency) else N.LAT_CONSTANT
        a.lat_mean_s[i] = ent.jitter.mean
    a.link_loss_rate[i] = ent.packet_loss_rate
    a.target[i] = -1 if ent.egress is None else cx.node_of[id(ent.egress)]


def _lower_load_balancer(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    rt = cx.rt
    backends = ent.all_backends
    if id(ent) in cx.scaled:
        backends = cx.scaled[id(ent)][1] + cx.scaled[id(ent)][2]       # the candidate list: the initial backends, then the pool
    for b in backends:
        if not isinstance(b, Server):
            raise UnsupportedTopology(f"backend '{b.name}' of '{ent.name}' is a {type(b).__name__}: only Server backends are lowered")
    st = ent.strategy
    a.kind[i] = N.NODE_LB
    code = next((c for cls, c in _STRATEGY_CODE if isinstance(st, cls)), None)
    if code is None:
        raise UnsupportedTopology(f"strategy {type(st).__name__} of '{ent.name}' is not lowered to the engine")
    _ensure(a, "lb_strategy", lambda: np.full(a.n, N.LB_ROUND_ROBIN, np.uint8))[i] = code
    _ensure(a, "lb_vnodes", lambda: np.zeros(a.n, np.int32))[i] = getattr(st, "virtual_nodes", 0)
    a.rt_off[i] = len(rt)
    a.rt_cnt[i] = len(backends)
    if isinstance(st, (WeightedRoundRobin, WeightedLeastConnections)):
        n_init = len(ent.all_backends)                         # (an instance joins at weight 1: add_backend's default)
        ws = [int(st.get_weight(b)) if q < n_init else 1 for q, b in enumerate(backends)]
        if isinstance(st, WeightedRoundRobin) and sum(ws) > WeightedRoundRobin.MAX_TOTAL_WEIGHT:
            raise UnsupportedTopology(f"'{ent.name}': WeightedRoundRobin with a total weight of {sum(ws)} needs a selection table "
                                      "beyond 2^24 entries (not lowered)")
        cx.weights[len(rt)] = ws
    flags = [int(ent.get_backend_info(b).is_healthy) if ent.get_backend_info(b) is not None else 1 for b in backends]
    if not all(flags):
        if isinstance(st, _FIXED_LIST):
            raise UnsupportedTopology(f"'{ent.name}': strategy {type(st).__name__} with an unhealthy backend ('"
                                      f"{ent.unhealthy_backends[0].name}') is not lowered (its selection over a changing backend list "
                                      "is a follow-up)")
        cx.unhealthy[len(rt)] = flags
    rt.extend(cx.node_of[id(b)] for b in backends)


def _lower_health_checker(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"health checker '{ent.name}'"
    lb = ent.load_balancer
    if not isinstance(lb, LoadBalancer) or id(lb) not in cx.node_of:
        raise UnsupportedTopology(f"{what}: its LoadBalancer is not an entity of this Simulation")
    if id(lb) in cx.scaled:
        other = cx.scaled[id(lb)][0]
        kind_ = type(other).__name__
        raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the {kind_} '{other.name}' "
                                  f"-- a HealthChecker and {'an' if kind_ == 'AutoScaler' else 'a'} {kind_} on one LoadBalancer are not lowered (a follow-up)")
    if id(lb) in cx.checked:
        raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the checker '{cx.checked[id(lb)]}' already "
                                  "(one HealthChecker per LoadBalancer is lowered)")
    cx.checked[id(lb)] = ent.name
    if isinstance(lb.strategy, _FIXED_LIST):
        raise _strategy_refusal(what, lb, "a HealthChecker")
    if not (ent.interval * 1e9 >= 1.0):
        raise UnsupportedTopology(f"{what}: an interval of {ent.interval} s is below one nanosecond")
    a.kind[i] = N.NODE_HEALTH_CHECKER
    a.target[i] = cx.node_of[id(lb)]
    _ensure(a, "hc_params", lambda: np.zeros((a.n, 5), np.float64))[i] = (
        ent.interval, ent.timeout, ent.healthy_threshold, ent.unhealthy_threshold, 1.0 if ent.is_running else 0.0)


def _lower_auto_scaler(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    lb, pol = ent.load_balancer, ent.policy
    _refuse_checked(cx, f"auto scaler '{ent.name}'", lb, "an AutoScaler")
    params = _ensure(a, "as_params", lambda: np.zeros((a.n, 10), np.float64))
    steps = _ensure(a, "as_steps", lambda: [None] * a.n)
    a.kind[i] = N.NODE_AUTO_SCALER
    a.target[i] = cx.node_of[id(lb)]
    if isinstance(pol, TargetUtilization):
        code, p0, p1 = N.AUTOSCALER_TARGET_UTILIZATION, pol._target, 0.0
    elif isinstance(pol, StepScaling):
        code, p0, p1 = N.AUTOSCALER_STEP, 0.0, 0.0
        try:
            steps[i] = [(float(t), int(d)) for t, d in pol._steps]
        except (TypeError, ValueError):
            raise UnsupportedTopology(f"auto scaler '{ent.name}': StepScaling steps must be (number, int) pairs") from None
    else:
        code, p0, p1 = N.AUTOSCALER_QUEUE_DEPTH, pol._scale_out_threshold, pol._scale_in_threshold
    params[i] = (code, p0, p1, ent._min_instances, ent._max_instances, ent._evaluation_interval, ent._scale_out_cooldown,
                 ent._scale_in_cooldown, len(cx.scaled[id(lb)][2]), 1.0 if ent.is_running else 0.0)


def _lower_canary_deployer(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    lb, ev = ent.load_balancer, ent._metric_evaluator
    _refuse_checked(cx, f"canary deployer '{ent.name}'", lb, "a CanaryDeployer")
    a.kind[i] = N.NODE_CANARY_DEPLOYER
    a.target[i] = cx.node_of[id(lb)]
    latency = isinstance(ev, LatencyEvaluator)
    _ensure(a, "cn_params", lambda: [None] * a.n)[i] = (
        [(float(s_.traffic_percentage), float(s_.evaluation_period)) for s_ in ent._stages],
        N.CANARY_LATENCY if latency else N.CANARY_ERROR_RATE, float(ev._max_latency if latency else ev._max_error_rate),
        float(ev._threshold_multiplier), float(ent._evaluation_interval))


def _lower_rolling_deployer(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    lb = ent.load_balancer
    _refuse_checked(cx, f"rolling deployer '{ent.name}'", lb, "a RollingDeployer")
    a.kind[i] = N.NODE_ROLLING_DEPLOYER
    a.target[i] = cx.node_of[id(lb)]
    _ensure(a, "rd_params", lambda: np.zeros((a.n, 5), np.float64))[i] = (
        ent._batch_size, ent._health_check_interval, ent._healthy_threshold, ent._max_failures, len(cx.scaled[id(lb)][2]))


def _hook_target(cx: _Lowering, what: str, ent, tgt=None, role: str = "target") -> int:
    """The node a Client or a wrapper sends to (`tgt`: a Hedge's target, a Fallback's primary or fallback entity, named by `role`).
    Its completion hook rides on the Event to the end of the NetworkLinks behind that target: what holds the item back there, or
    hangs a hook of its own on it, is refused."""
    tgt = ent.target if tgt is None else tgt
    if _takes_no_requests(cx, tgt):
        raise UnsupportedTopology(f"{what}: its {role} {type(tgt).__name__} '{getattr(tgt, 'name', tgt)}' takes no Requests")
    end, hops = tgt, 0
    while isinstance(end, NetworkLink) and end.egress is not None and hops <= cx.a.n:
        end, hops = end.egress, hops + 1
    via = " (through its NetworkLinks)" if end is not tgt else ""
    if isinstance(end, (Hedge, Fallback)) or (isinstance(ent, (Hedge, Fallback)) and isinstance(end, (LoadBalancer, Bulkhead, TimeoutWrapper, Client))):
        raise UnsupportedTopology(f"{what}: its {role}{via} is the {type(end).__name__} '{end.name}' -- two completion hooks on one Event "
                                  "are not lowered (a follow-up)")
    if isinstance(end, _STOCK):
        raise UnsupportedTopology(f"{what}: its {role}{via} is the {type(end).__name__} '{end.name}' -- a completion hook on an item that "
                                  "a PooledCycleResource or an InventoryBuffer holds or forwards is not lowered (a follow-up)")
    if isinstance(end, _FLOWS) and isinstance(ent, (Hedge, Fallback)):
        raise UnsupportedTopology(f"{what}: its {role}{via} is the {type(end).__name__} '{end.name}' -- a completion hook on an item that "
                                  "a BatchProcessor, ConveyorBelt or GateController holds is not lowered (a follow-up)")
    if isinstance(end, _FLOWS):
        raise UnsupportedTopology(f"{what}: its target{via} is the {type(end).__name__} '{end.name}' -- a completion hook on an item that "
                                  "a BatchProcessor, ConveyorBelt or GateController holds is not lowered (a follow-up)")
    if isinstance(end, (LoadBalancer, Bulkhead, TimeoutWrapper, Client)):
        # (a wrapper names any Client "the Client", a Client names it by its class)
        kind_ = "Client" if isinstance(end, Client) and not isinstance(ent, Client) else type(end).__name__
        raise UnsupportedTopology(f"{what}: its target{via} is the {kind_} '{end.name}' -- two completion hooks on one Event are not "
                                  "lowered (a follow-up)")
    return cx.node_of[id(tgt)]


def _lower_wrapper(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"{type(ent).__name__} '{ent.name}'"
    target = _hook_target(cx, what, ent)
    params = _ensure(a, "wrap_params", lambda: np.zeros((a.n, 5), np.float64))
    a.target[i] = target
    if isinstance(ent, Bulkhead):
        if ent.max_concurrent > Bulkhead.MAX_CONCURRENT:
            raise UnsupportedTopology(f"{what}: max_concurrent = {ent.max_concurrent} is beyond the {Bulkhead.MAX_CONCURRENT} request "
                                      "ids the engine's in-flight table holds")
        if ent.max_wait_queue > (1 << 30):
            raise UnsupportedTopology(f"{what}: max_wait_queue = {ent.max_wait_queue} is beyond 2^30")
        if ent.max_wait_time is not None and not np.isfinite(ent.max_wait_time):
            raise UnsupportedTopology(f"{what}: max_wait_time must be finite or None")
        a.kind[i] = N.NODE_BULKHEAD
        params[i, :3] = (ent.max_concurrent, ent.max_wait_queue, -1.0 if ent.max_wait_time is None else ent.max_wait_time)
    else:
        if ent._on_timeout is not None:
            raise UnsupportedTopology(f"{what}: on_timeout= is a host callable (not lowered)")
        if not np.isfinite(ent.timeout):
            raise UnsupportedTopology(f"{what}: timeout must be finite")
        a.kind[i] = N.NODE_TIMEOUT_WRAPPER
        params[i, 3] = ent.timeout


def _wrapper_delay_ns(what: str, name: str, seconds) -> int:
    """Duration.from_seconds(seconds) in whole nanoseconds: what a Hedge / Fallback handler adds to `now`."""
    try:
        ns = Duration.from_seconds(seconds).nanoseconds
        if not 0 <= ns < (1 << 61):
            raise OverflowError(ns)
    except (OverflowError, ValueError, TypeError) as e:
        raise UnsupportedTopology(f"{what}: {name} = {seconds!r} cannot be evaluated as a Duration ({type(e).__name__}: {e})") from None
    return ns


def _lower_hedge(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"Hedge '{ent.name}'"
    target = _hook_target(cx, what, ent)
    if type(ent.max_hedges) is not int or ent.max_hedges > Hedge.MAX_HEDGES:
        raise UnsupportedTopology(f"{what}: max_hedges = {ent.max_hedges!r} is beyond the {Hedge.MAX_HEDGES} hedges a request's entry "
                                  "counts on the engine (Hedge.MAX_HEDGES)")
    a.kind[i] = N.NODE_HEDGE
    a.target[i] = target
    _ensure(a, "hg_params", lambda: np.zeros((a.n, 4), np.int64))[i] = (_wrapper_delay_ns(what, "hedge_delay", ent.hedge_delay),
                                                                        ent.max_hedges, -1, 0)


def _lower_fallback(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"Fallback '{ent.name}'"
    if ent._failure_predicate is not None:
        raise UnsupportedTopology(f"{what}: failure_predicate= is a host callable (not lowered)")
    if not isinstance(ent.fallback, Entity):
        raise UnsupportedTopology(f"{what}: fallback= is a host callable, not an Entity (not lowered)")
    primary = _hook_target(cx, what, ent, ent.primary, "primary")
    fallback = _hook_target(cx, what, ent, ent.fallback, "fallback entity")
    a.kind[i] = N.NODE_FALLBACK
    a.target[i] = primary
    _ensure(a, "hg_params", lambda: np.zeros((a.n, 4), np.int64))[i] = (
        -1 if ent.timeout is None else _wrapper_delay_ns(what, "timeout", ent.timeout), 0, fallback, 0)


def _lower_client(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"Client '{ent.name}'"
    target = _hook_target(cx, what, ent)
    if ent._on_success is not None or ent._on_failure is not None:
        raise UnsupportedTopology(f"{what}: on_success= / on_failure= are host callables (not lowered)")
    if ent.timeout is not None and not np.isfinite(ent.timeout):
        raise UnsupportedTopology(f"{what}: timeout must be finite or None")
    delays = client_delay_table(ent.retry_policy, what)
    a.kind[i] = N.NODE_CLIENT
    a.target[i] = target
    _ensure(a, "cl_params", lambda: np.zeros((a.n, 2), np.float64))[i, 0] = -1.0 if ent.timeout is None else float(ent.timeout)
    _ensure(cx, "client_delays", lambda: [np.zeros(0, np.int64) for _ in range(a.n)])[i] = delays


def _lower_flow(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"{type(ent).__name__} '{ent.name}'"
    d = ent.downstream
    if _takes_no_requests(cx, d):
        raise UnsupportedTopology(f"{what}: its downstream {type(d).__name__} '{getattr(d, 'name', d)}' takes no Requests")
    params = _ensure(a, "flow_params", lambda: np.zeros((a.n, 4), np.int64))
    a.target[i] = cx.node_of[id(d)]
    if isinstance(ent, BatchProcessor):
        if type(ent.batch_size) is not int:
            raise UnsupportedTopology(f"{what}: batch_size must be an int, got {ent.batch_size!r}")
        if ent.batch_size > BatchProcessor.MAX_BATCH_SIZE:
            raise UnsupportedTopology(f"{what}: batch_size = {ent.batch_size} is beyond the {BatchProcessor.MAX_BATCH_SIZE} items of "
                                      "one batch on the engine (BatchProcessor.MAX_BATCH_SIZE)")
        a.kind[i] = N.NODE_BATCH_PROCESSOR
        # the generator's `yield process_time` is float(process_time) added to an Instant, `now + timeout_s` the number itself
        params[i] = (ent.batch_size, flow_delay_ns(float(ent.process_time), what, "process_time"),
                     flow_delay_ns(ent.timeout_s, what, "timeout_s") if ent.timeout_s > 0 else 0, 0)
    elif isinstance(ent, ConveyorBelt):
        a.kind[i] = N.NODE_CONVEYOR
        cap = ent._capacity
        params[i] = (0 if not cap > 0 else min(int(cap), (1 << 31) - 1), flow_delay_ns(float(ent.transit_time), what, "transit_time"), 0, 0)
    else:
        cap = ent._queue_capacity
        if cap > GateController.MAX_QUEUE_CAPACITY:
            raise UnsupportedTopology(f"{what}: queue_capacity = {cap} is beyond the {GateController.MAX_QUEUE_CAPACITY} items of a "
                                      "bounded queue on the engine (GateController.MAX_QUEUE_CAPACITY; 0 is unbounded)")
        if ent._queue_depth:
            raise UnsupportedTopology(f"{what}: {ent._queue_depth} items are still queued from an earlier run (not lowered)")
        a.kind[i] = N.NODE_GATE
        params[i] = (max(int(cap), 0), 0, int(ent._open_cycles), 1 if ent._is_open else 0)


def _stock_int(what: str, name: str, value, least: int, most: int, limit: str) -> int:
    """An integer parameter of a pool or a buffer within [least, most], or the refusal that names it."""
    if type(value) is not int:
        raise UnsupportedTopology(f"{what}: {name} must be an int, got {value!r}")
    if not least <= value <= most:
        raise UnsupportedTopology(f"{what}: {name} = {value} is beyond {limit}")
    return value


def _stock_seconds(what: str, name: str, value) -> float:
    try:
        ok = bool(np.isfinite(value)) and value >= 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise UnsupportedTopology(f"{what}: {name} = {value!r} is not a finite number >= 0")
    return float(value)


def _lower_stock(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    what = f"{type(ent).__name__} '{ent.name}'"
    # (a buffer's `supplier` is a node like any entity of downstream_entities(), but nothing is ever sent to it)
    for role, d in (("downstream", ent.downstream), ("stockout_target", getattr(ent, "stockout_target", None))):
        if d is not None and _takes_no_requests(cx, d):
            raise UnsupportedTopology(f"{what}: its {role} {type(d).__name__} '{getattr(d, 'name', d)}' takes no Requests")
    params = _ensure(a, "st_params", lambda: np.zeros((a.n, 5), np.int64))
    a.target[i] = -1 if ent.downstream is None else cx.node_of[id(ent.downstream)]
    if isinstance(ent, PooledCycleResource):
        units = f"the {PooledCycleResource.MAX_POOL_SIZE} the engine holds (PooledCycleResource.MAX_POOL_SIZE)"
        size = _stock_int(what, "pool_size", ent.pool_size, 1, PooledCycleResource.MAX_POOL_SIZE, units)
        cap = _stock_int(what, "queue_capacity", ent._queue_capacity, -(1 << 62), PooledCycleResource.MAX_POOL_SIZE, units + "; 0 is unbounded")
        if len(ent._queue) or ent._active:
            raise UnsupportedTopology(f"{what}: {len(ent._queue)} Requests wait and {ent._active} cycles run from an earlier run (not lowered)")
        a.kind[i] = N.NODE_POOLED_CYCLE
        # the generator's `yield cycle_time` is the number added to an Instant: int(cycle_time * 1e9) nanoseconds whatever `now` is
        params[i] = (size, flow_delay_ns(_stock_seconds(what, "cycle_time", ent.cycle_time), what, "cycle_time"), max(cap, 0), 0, -1)
    else:
        limit = "2^62 (InventoryBuffer.MAX_STOCK)"
        stock = _stock_int(what, "initial_stock", ent._stock, 0, InventoryBuffer.MAX_STOCK, limit)
        point = _stock_int(what, "reorder_point", ent.reorder_point, 0, InventoryBuffer.MAX_STOCK, limit)
        order = _stock_int(what, "order_quantity", ent.order_quantity, 1, InventoryBuffer.MAX_STOCK, limit)
        if point + order > InventoryBuffer.MAX_LEVEL:
            # the stock never passes max(initial_stock, reorder_point + order_quantity): beyond this a 64-bit counter would wrap
            raise UnsupportedTopology(f"{what}: reorder_point + order_quantity = {point + order} is beyond 2^63 - 2^48, the level a 64-bit "
                                      "stock holds (InventoryBuffer.MAX_LEVEL; the reference's integers are unbounded)")
        lead = _stock_seconds(what, "lead_time", ent.lead_time)
        if lead > 2.0e9:
            raise UnsupportedTopology(f"{what}: lead_time = {lead!r} is beyond 2e9 s")
        if ent._order_pending:
            raise UnsupportedTopology(f"{what}: an order is pending from an earlier run (not lowered)")
        a.kind[i] = N.NODE_INVENTORY
        so = ent.stockout_target
        params[i] = (stock, point, order, int(np.float64(lead).view(np.int64)), -1 if so is None else cx.node_of[id(so)])


def _lower_limiter(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    pol = ent.policy
    if type(pol) not in LIMITER_POLICIES:
        raise UnsupportedTopology(f"limiter '{ent.name}': policy {type(pol).__name__} is not lowered to the engine (lowered: "
                                  "TokenBucketPolicy, LeakyBucketPolicy, SlidingWindowPolicy, FixedWindowPolicy)")
    if id(pol) in cx.policies_seen:
        raise UnsupportedTopology(f"limiter '{ent.name}' shares its policy object with '{cx.policies_seen[id(pol)]}': one policy per "
                                  "limiter is lowered")
    cx.policies_seen[id(pol)] = ent.name
    if not pol._pristine():
        raise UnsupportedTopology(f"limiter '{ent.name}': its policy has been used already (a run starts from the policy as constructed)")
    kind, p0, p1, p2, count = pol._engine_params()
    if isinstance(pol, TokenBucketPolicy) and not (p1 > 0):
        raise UnsupportedTopology(f"limiter '{ent.name}': refill_rate must be > 0, got {p1} (the reference divides by it in mid-run)")
    if kind == N.LIMITER_LEAKY_BUCKET and not (p0 > 0):
        raise UnsupportedTopology(f"limiter '{ent.name}': leak_rate must be > 0, got {p0} (the reference never lets a queued Request go)")
    if isinstance(pol, SlidingWindowPolicy):
        if count < 1:
            raise UnsupportedTopology(f"limiter '{ent.name}': max_requests must be >= 1, got {count} (the reference fails in mid-run)")
        if count > N.LIMITER_MAX_SLIDING_LOG:
            raise UnsupportedTopology(f"limiter '{ent.name}': a SlidingWindowPolicy log of {count} entries is beyond the "
                                      f"{N.LIMITER_MAX_SLIDING_LOG} the engine keeps")
    if not all(np.isfinite((p0, p1, p2))):
        raise UnsupportedTopology(f"limiter '{ent.name}': the policy's parameters must be finite")
    if kind in (N.LIMITER_SLIDING_WINDOW, N.LIMITER_FIXED_WINDOW) and not (p0 >= 1e-9):
        raise UnsupportedTopology(f"limiter '{ent.name}': a window of {p0} s is below one nanosecond")
    cap = ent._queue.capacity
    a.kind[i] = N.NODE_RATE_LIMITER
    a.target[i] = cx.node_of[id(ent.downstream)]
    a.queue_cap[i] = -1 if cap == float("inf") else int(cap)
    _ensure(a, "lim_policy", lambda: np.full(a.n, N.LIMITER_NONE, np.uint8))[i] = kind
    _ensure(a, "lim_params", lambda: np.zeros((a.n, 3), np.float64))[i] = (p0, p1, p2)
    _ensure(a, "lim_count", lambda: np.zeros(a.n, np.int64))[i] = count


def _lower_router(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    if not ent.targets:
        raise UnsupportedTopology(f"router '{ent.name}' has no targets")
    a.kind[i] = N.NODE_ROUTER
    a.stream_base[i] = cx.stream(RandomRouter)
    a.rt_off[i] = len(cx.rt)
    a.rt_cnt[i] = len(ent.targets)
    cx.rt.extend(cx.node_of[id(t)] for t in ent.targets)


def _lower_sink(cx: _Lowering, a: GraphArrays, i: int, ent) -> None:
    a.kind[i] = N.NODE_SINK                            # (a Network too: a node that no Event reaches)


# the first class a node is an instance of decides (a pool's Servers before all, the wrappers before the Client ...)
_LOWER = ((Source, _lower_source), (Probe, _lower_probe), (Server, _lower_server), (NetworkLink, _lower_link),
          (LoadBalancer, _lower_load_balancer), (HealthChecker, _lower_health_checker), (AutoScaler, _lower_auto_scaler),
          (CanaryDeployer, _lower_canary_deployer), (RollingDeployer, _lower_rolling_deployer), ((Bulkhead, TimeoutWrapper), _lower_wrapper),
          (Hedge, _lower_hedge), (Fallback, _lower_fallback), (Client, _lower_client), (_FLOWS, _lower_flow), (_STOCK, _lower_stock), (RateLimitedEntity, _lower_limiter), (RandomRouter, _lower_router))


def _assemble(cx: _Lowering) -> GeneralGraph:
    a, nodes, node_of = cx.a, cx.nodes, cx.node_of
    a.rt_targets = np.array(cx.rt, np.int32)
    if a.cl_params is not None:
        a.cl_delay_off = _offsets(cx.client_delays, np.int64)
        a.cl_delays_ns = np.concatenate(cx.client_delays).astype(np.int64)
    if cx.weights:
        a.lb_weights = np.ones(len(cx.rt), np.int32)
        for off, ws in cx.weights.items():
            a.lb_weights[off:off + len(ws)] = ws
    # (a scaled or deployed LoadBalancer's member list is the healthy list)
    if cx.unhealthy or a.hc_params is not None or a.as_params is not None or a.rd_params is not None or a.cn_params is not None:
        a.lb_healthy = np.ones(len(cx.rt), np.uint8)
        for off, flags in cx.unhealthy.items():
            a.lb_healthy[off:off + len(flags)] = flags
    if a.lb_strategy is not None:
        _check_keys(nodes, node_of, a)
        blobs = [(x.name.encode() if isinstance(x, Server) else b"") for x in nodes]     # (only an LB's backends need their name)
        a.names = b"".join(blobs)
        a.name_off = _offsets(blobs, np.int32)
    assert all(a.kind[i] == N.NODE_SOURCE for i in range(cx.n_src)) and all(a.kind[i] == N.NODE_PROBE for i in range(cx.n_src, cx.n_front))
    g = GeneralGraph(nodes, a, node_of)
    g.n_own, g.scaler_starts = cx.n_own, cx.scaler_starts
    for lb_id, (owner, initial, pool) in cx.scaled.items():
        (g.scaled if isinstance(owner, AutoScaler) else g.deployed)[node_of[lb_id]] = (node_of[id(owner)], initial, pool)
        if not isinstance(owner, AutoScaler):
            g.deploys[node_of[id(owner)]] = cx.deploys.get(id(owner), 1)
    for i, (owner, k) in cx.pool_of.items():
        (g.pool_of if isinstance(owner, AutoScaler) else g.dpool_of)[i] = (node_of[id(owner)], k)
    g.rr_base = {i: nodes[i].strategy._index for i in list(g.scaled) + list(g.deployed) if isinstance(nodes[i].strategy, RoundRobin)}
    return g


def lower_general(sources: list, entities: list, probes=None, *, start_ns: int = 0, end_ns: int | None = None,
                  scaler_starts: int = 1, deploys: dict | None = None) -> GeneralGraph:
    """`sources` / `entities` of a Simulation -> the node arrays of the single-heap engine.  Refuses by name what that engine
    does not run either (lowering.UnsupportedTopology).  `start_ns` / `end_ns` (None: Infinity) / `scaler_starts` (the start() Events
    scheduled per scaler) size the instance pools of the AutoScalers, `deploys` (id(deployer) -> its deploy() Events) the deployers'."""
    cx = _Lowering(start_ns, end_ns, scaler_starts, deploys)
    _collect_nodes(cx, sources, entities, probes)
    _build_pools(cx)
    cx.a = GraphArrays(len(cx.nodes))
    for i, ent in enumerate(cx.nodes):
        lower = next((f for cls, f in _LOWER if isinstance(ent, cls)), _lower_sink)
        lower(cx, cx.a, i, ent)
    return _assemble(cx)


def _reaches(nodes, node_of, start) -> set:
    """Node ids a Request that enters `start` can visit."""
    seen, todo = set(), [node_of[id(start)]]
    while todo:
        i = todo.pop()
        if i in seen:
            continue
        seen.add(i)
        todo.extend(node_of[id(d)] for d in nodes[i].downstream_entities() if d is not None)
    return seen


def _check_keys(nodes, node_of, a) -> None:
    """A Random LoadBalancer takes its Requests from Sources that aim at it directly (their KEY draw is the choice; a Request
    without one would ask the process-wide `random`, which the engine's streams do not define).  A key-less Request at a
    ConsistentHash LoadBalancer is the reference's own case: the strategy's fallback RoundRobin (strategies.py:362,420-421)."""
    rnd = [i for i, x in enumerate(nodes) if isinstance(x, LoadBalancer) and isinstance(x.strategy, Random)]
    if not rnd:
        return
    for src in nodes:
        if not isinstance(src, Source):
            continue
        tgt = src._event_provider._target
        reach = _reaches(nodes, node_of, tgt)
        for j in rnd:
            if j in reach and tgt is not nodes[j]:
                raise UnsupportedTopology(f"source '{src.name}' reaches the Random LoadBalancer '{nodes[j].name}' through other entities: "
                                          "only Sources that aim at it directly carry the draw it chooses by")


def keyless_hazard(g: GeneralGraph, target) -> str | None:
    """Simulation.schedule(): a scheduled Request carries no client id -- the name of a Random LoadBalancer it could reach."""
    for j in _reaches(g.nodes, g.node_of, target):
        x = g.nodes[j]
        if isinstance(x, LoadBalancer) and isinstance(x.strategy, Random):
            return x.name
    return None
