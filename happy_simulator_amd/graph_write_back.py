"""A single-heap run's results onto the user's objects, under the attribute names the reference uses: write_back_general(), one
function per entity kind (`_WRITE_BACK`)."""
from __future__ import annotations

import numpy as np

from . import _native as N
from .core.temporal import Duration, Instant
from .entities import (QUEUE_POLICIES, AdaptiveLIFO, AutoScaler, BackendHealthState, BackendInfo, BatchProcessor, Bulkhead, CanaryDeployer,
                       CanaryState, Client, CoDelQueue, ConsistentHash, ConveyorBelt, DeploymentState, Fallback, GateController, HealthChecker, Hedge,
                       InventoryBuffer, IPHash, LoadBalancer, Network, NetworkLink, PooledCycleResource, Probe, RandomRouter, RateLimitedEntity, RollingDeployer, RoundRobin,
                       ScalingEvent, Server, Source, TimeoutWrapper, WeightedRoundRobin)
from .graph_engine import GeneralGraph, GraphEngine


class _Results:
    """What the per-kind functions read: the graph, the run's stats and records, and the engine for what only a family's own
    reader returns (GraphEngine and PartRun offer the same readers; a graph without such a family needs no engine)."""

    def __init__(self, g: GeneralGraph, stats: dict, rec_node, rec_t, rec_cr, device: int, engine):
        self.g, self.a, self.stats, self.rec_t, self.rec_cr, self.device, self.engine = g, g.arrays, stats, rec_t, rec_cr, device, engine
        self.order = np.argsort(rec_node, kind="stable")          # per node, still in processing order
        self.bounds = np.searchsorted(rec_node[self.order], np.arange(g.arrays.n + 1))
        self.scalers = {sn: engine.scaler(sn) for sn, _initial, _pool in g.scaled.values()}      # GraphEngine.scaler(node) per AutoScaler
        # GraphEngine.deployer(node) per RollingDeployer, GraphEngine.canary(node) per CanaryDeployer (its one instance: id 1 once it is set)
        self.deployers = {dn: (engine.deployer(dn) if isinstance(g.nodes[dn], RollingDeployer) else engine.canary(dn))
                          for dn, _initial, _pool in g.deployed.values()}
        for w in self.deployers.values():
            if "has_canary" in w:
                w.update(next_instance_id=w["has_canary"], readded=[])

    def rows(self, i: int) -> np.ndarray:
        """The records of node `i`, in processing order."""
        return self.order[self.bounds[i]:self.bounds[i + 1]]

    def dormant(self, i: int) -> bool:
        """A pool's instance that the run never activated: it is left untouched."""
        g = self.g
        if i in g.pool_of and g.pool_of[i][1] > self.scalers[g.pool_of[i][0]]["next_instance_id"]:
            return True
        return i in g.dpool_of and g.dpool_of[i][1] > self.deployers[g.dpool_of[i][0]]["next_instance_id"]


def _write_source(r: _Results, i: int, ent) -> None:
    ent._generated_count = int(r.stats["generated"][i])
    ent._event_provider._generated = int(r.stats["payloads"][i])


def _write_server(r: _Results, i: int, ent) -> None:
    stats = r.stats
    ent._queue.stats_accepted = int(stats["accepted"][i])
    ent._queue.stats_dropped = int(stats["dropped"][i])
    ent._queue.depth = int(stats["queue_depth"][i])
    ent._requests_completed = int(stats["completed"][i])
    ent._requests_rejected = int(stats["rejected"][i])
    ent._total_service_time = float(stats["total_service_s"][i])
    ent._active = int(stats["active"][i])
    pol = ent._policy
    if isinstance(pol, QUEUE_POLICIES):
        w = r.engine.queue_policy(i)
        pol._len = w["len"]
        if isinstance(pol, AdaptiveLIFO):
            (pol._enqueued, pol._dequeued_fifo, pol._dequeued_lifo, pol._capacity_rejected, pol._mode_switches) = (
                w["enqueued"], w["dequeued_fifo"], w["dequeued_lifo"], w["capacity_rejected"], w["switches"])
            pol._was_congested = bool(w["flag"])
        elif isinstance(pol, CoDelQueue):
            (pol._enqueued, pol._dequeued, pol._dropped, pol._capacity_rejected, pol._drop_intervals) = (
                w["enqueued"], w["dequeued_fifo"], w["dropped"], w["capacity_rejected"], w["switches"])
            pol._dropping, pol._count, pol._last_count = bool(w["flag"]), w["count"], w["last_count"]
            pol._first_above_time = Instant(w["first_above_ns"]) if w["has_first_above"] else None
            pol._drop_next = Instant(w["drop_next_ns"]) if w["has_drop_next"] else None


def _write_link(r: _Results, i: int, ent) -> None:
    ent.packets_sent = int(r.stats["packets_sent"][i])
    ent.packets_dropped = int(r.stats["packets_dropped"][i])
    ent._entered = int(r.stats["entered"][i])
    # (a graph with link faults: Simulation._general_finish puts the count of the engine's own word here)
    ent._loss_draws = ent._entered if ent.packet_loss_rate > 0 else 0


def _rebuild_backends(r: _Results, i: int, ent, cand: list, slots, keeps, selections: int) -> None:
    """A LoadBalancer whose backends joined and left during the run: `_backends` as the entries of `slots` (of `cand`, the initial
    backends and the pool), in that order.  An entry goes on with its BackendInfo where `keeps(slot, info)`; a backend that left has
    no entry any more, the strategy keeps what it learned of every name (its weight, its current weight)."""
    off = int(r.a.rt_off[i])
    old = ent._backends
    ent._backends = {}
    for q in slots:
        b = cand[q]
        info = old.get(b.name)
        if info is None or info.backend is not b or not keeps(q, info):
            info = BackendInfo(backend=b, weight=1)
        ent._backends[b.name] = info
        info.total_requests = int(r.stats["rt_taken"][off + q])
    if i in r.g.rr_base:
        ent.strategy._index = r.g.rr_base[i] + selections          # (bound behind every window: absolute, not added once more)
    h = r.engine.health(i)
    if isinstance(ent.strategy, WeightedRoundRobin) and h["current_weights"] is not None:
        ent.strategy._selections = selections
        ent.strategy._current_weights = {cand[q].name: v for q, v in sorted(h["current_weights"].items())}


def _write_scaled_lb(r: _Results, i: int, ent, selections: int) -> None:
    """`_backends` is the initial backends, then the live managed instances in id order."""
    sn, initial, pool = r.g.scaled[i]
    w = r.scalers[sn]
    slots = [q for q in range(len(initial) + len(pool)) if w["member"][q]]
    _rebuild_backends(r, i, ent, initial + pool, slots, lambda q, info: q < len(initial), selections)
    if hasattr(ent.strategy, "set_weight"):
        for b in pool[:w["next_instance_id"]]:
            ent.strategy._weights[b.name] = 1                        # add_backend's set_weight(backend, 1)


def _write_deployed_lb(r: _Results, i: int, ent, selections: int) -> None:
    """`_backends` in insertion order, as the device's member list holds it; a backend that came back has a new BackendInfo (the
    device counts its total_requests from 0 again)."""
    dn, initial, pool = r.g.deployed[i]
    w = r.deployers[dn]
    cand = initial + pool
    _rebuild_backends(r, i, ent, cand, w["members"], lambda q, info: not (q in w["readded"] and info.weight != 1), selections)
    if hasattr(ent.strategy, "set_weight") and "weight_set" in w:
        for q in w["weight_set"]:                                    # a canary deployer's set_weight calls: the device's weights
            ent.strategy._weights[cand[q].name] = int(w["weights"][q])
    elif hasattr(ent.strategy, "set_weight"):
        for b in pool[:w["next_instance_id"]] + [cand[q] for q in w["readded"]]:
            ent.strategy._weights[b.name] = 1                        # add_backend's set_weight(backend, 1)


def _write_load_balancer(r: _Results, i: int, ent) -> None:
    stats = r.stats
    (ent._requests_received, ent._requests_forwarded, ent._requests_failed, ent._no_backend_available,
     ent._in_flight_count, selections) = (int(v) for v in stats["lb"][i])
    if isinstance(ent.strategy, RoundRobin):
        ent.strategy._index += selections                  # one select per forwarded Request (strategies.py:66-67)
    elif isinstance(ent.strategy, (ConsistentHash, IPHash)):
        ent.strategy._fallback._index += selections        # ... per KEY-LESS Request (strategies.py:309,362,420-421)
    if i in r.g.scaled:
        return _write_scaled_lb(r, i, ent, selections)
    if i in r.g.deployed:
        return _write_deployed_lb(r, i, ent, selections)
    off = int(r.a.rt_off[i])
    for q, b in enumerate(ent.all_backends):
        ent._backends[b.name].total_requests = int(stats["rt_taken"][off + q])
    if r.engine is not None and r.a.has_health:
        h = r.engine.health(i)
        for q, b in enumerate(ent.all_backends):
            ent._backends[b.name].is_healthy = bool(h["healthy"][q])
        ent._backends_marked_unhealthy += int(h["marks"][0])
        ent._backends_marked_healthy += int(h["marks"][1])
        if isinstance(ent.strategy, WeightedRoundRobin) and h["current_weights"] is not None:
            # the live algorithm ran (csrc/hs_graph.hip): what it left, for every backend a select() ever saw (strategies.py:117-119)
            ent.strategy._selections = selections
            ent.strategy._current_weights = {b.name: h["current_weights"][q] for q, b in enumerate(ent.all_backends)
                                             if q in h["current_weights"]}
            return
    if isinstance(ent.strategy, WeightedRoundRobin) and ent.all_backends:
        # what select() leaves in `_current_weights` after t selections of which n_i went to backend i: w_i * t - W * n_i
        # (strategies.py:125-132; a run starts from a fresh strategy, as every engine run starts from time zero)
        st = ent.strategy
        ws = [int(st.get_weight(b)) for b in ent.all_backends]
        st._selections = selections
        st._current_weights = ({b.name: w * selections - sum(ws) * int(stats["rt_taken"][off + q])
                                for q, (b, w) in enumerate(zip(ent.all_backends, ws))} if selections else {})


def _write_canary_deployer(r: _Results, i: int, ent) -> None:
    w = r.deployers[i]
    (ent._deployments_started, ent._deployments_completed, ent._deployments_rolled_back, ent._stages_completed,
     ent._evaluations_performed, ent._evaluations_passed, ent._evaluations_failed) = (w[k] for k in GraphEngine._CANARY_NAMES[:7])
    ent.state = CanaryState(status=N.CANARY_STATUS[w["status"]], current_stage=w["current_stage"], total_stages=w["total_stages"],
                            canary_traffic_pct=w["traffic_pct"])
    _dn, initial, pool = r.g.deployed[int(r.a.target[i])]
    cand = initial + pool
    ent._canary = pool[0] if w["has_canary"] else None
    ent._baseline_backends = [cand[q] for q in w["baseline"]]
    ent._stage_start_time = Instant(w["stage_start_ns"]) if w["stage_start_ns"] >= 0 else None


def _write_rolling_deployer(r: _Results, i: int, ent) -> None:
    w = r.deployers[i]
    (ent._deployments_started, ent._deployments_completed, ent._deployments_rolled_back, ent._instances_replaced,
     ent._health_checks_performed, ent._health_checks_passed, ent._health_checks_failed) = (w[k] for k in GraphEngine._DEPLOYER_NAMES[:7])
    ent.state = DeploymentState(status=N.DEPLOYMENT_STATUS[w["status"]], total_instances=w["total_instances"], replaced=w["replaced"],
                                failed=w["failed"], current_batch=w["current_batch"])
    ent._next_instance_id, ent._health_fail_count = w["next_instance_id"], w["health_fail_count"]
    _dn, initial, pool = r.g.deployed[int(r.a.target[i])]
    cand = initial + pool
    ent._old_backends, ent._new_backends = [cand[q] for q in w["old"]], [cand[q] for q in w["new"]]
    ent._current_batch_old, ent._current_batch_new = [cand[q] for q in w["batch_old"]], [cand[q] for q in w["batch_new"]]
    ent._health_pass_count = {cand[q].name: v for q, v in sorted(w["pass_count"].items())}


def _write_auto_scaler(r: _Results, i: int, ent) -> None:
    w = r.scalers[i]
    (ent._evaluations, ent._scale_out_count, ent._scale_in_count, ent._instances_added, ent._instances_removed,
     ent._cooldown_blocks, ent._next_instance_id) = (w[k] for k in GraphEngine._SCALER_NAMES[:7])
    ent._last_scale_action = (None, "scale_out", "scale_in")[w["last_action"]]
    ent._last_scale_time = Instant(w["last_time_ns"]) if w["last_action"] else None
    ent.scaling_history = [ScalingEvent(Instant(int(t)), "scale_out" if act == 1 else "scale_in", int(c0), int(c1),
                                        f"{'Added' if act == 1 else 'Removed'} {int(cnt)} instances")
                           for t, act, c0, c1, cnt in w["history"].tolist()]
    _sn, initial, pool = r.g.scaled[int(r.a.target[i])]
    ent._managed_servers = [pool[q - len(initial)] for q in range(len(initial), len(initial) + len(pool)) if w["member"][q]]


def _write_health_checker(r: _Results, i: int, ent) -> None:
    h = r.engine.health(i)
    (ent._checks_performed, ent._checks_passed, ent._checks_failed, ent._checks_timed_out, ent._backends_marked_healthy,
     ent._backends_marked_unhealthy) = (int(v) for v in h["stats"])
    ent._next_check_id = ent._checks_performed               # one id per check performed (health_check.py:293-297)
    ent._backend_states, ent._pending_checks = {}, {}
    for b, (succ, fail, last_ns, passed, checking, pending) in zip(ent.load_balancer.all_backends, h["states"].tolist()):
        if last_ns < 0:
            continue                                          # (never checked: the reference has no entry for it)
        ent._backend_states[b.name] = BackendHealthState(succ, fail, Instant(last_ns), None if passed < 0 else bool(passed), bool(checking))
        if pending:
            ent._pending_checks[b.name] = pending


def _write_bulkhead(r: _Results, i: int, ent) -> None:
    w = r.engine.wrapper(i)
    (ent._total_requests, ent._accepted_requests, ent._rejected_requests, ent._timed_out_requests, ent._queued_requests,
     ent._peak_concurrent, ent._peak_queue_depth, ent._active_count) = (w[k] for k in (
         "total", "accepted", "rejected", "timed_out", "queued", "peak_concurrent", "peak_queue_depth", "active_count"))
    ent._next_request_id = w["next_request_id"]
    ent._wait_queue = [int(x) for x in w["queue_ids"]]
    ent._in_flight = {int(x): {} for x in w["in_flight_ids"]}


def _write_flow(r: _Results, i: int, ent) -> None:
    w = r.engine.flow(i)
    if isinstance(ent, BatchProcessor):
        ent._batches_processed, ent._items_processed, ent._timeouts, ent._buffer_depth = (
            w["batches_processed"], w["items_processed"], w["timeouts"], w["buffer_depth"])
    elif isinstance(ent, ConveyorBelt):
        ent._items_transported, ent._items_rejected, ent._items_in_transit = w["items_transported"], w["items_rejected"], w["items_in_transit"]
    else:
        ent._passed_through, ent._queued_while_closed, ent._rejected, ent._open_cycles, ent._queue_depth = (
            w["passed_through"], w["queued_while_closed"], w["rejected"], w["open_cycles"], w["queue_depth"])
        ent._is_open = bool(w["is_open"])


def _write_client(r: _Results, i: int, ent) -> None:
    w = r.engine.client(i)
    (ent._requests_sent, ent._responses_received, ent._timeouts, ent._retries, ent._failures) = (w[k] for k in (
        "requests_sent", "responses_received", "timeouts", "retries", "failures"))
    ent._in_flight = {(int(rid) or None, int(att)): {} for rid, att in w["in_flight_keys"]}
    # _response_times: (now - start_time).to_seconds() of every response, in order -- the rows hold both in nanoseconds
    ent._response_times = [Duration(int(ns)).to_seconds() for ns in r.rec_t[r.rows(i)]]


def _write_timeout_wrapper(r: _Results, i: int, ent) -> None:
    w = r.engine.wrapper(i)
    ent._total_requests, ent._successful_requests, ent._timed_out_requests = w["total"], w["successful"], w["timed_out"]
    ent._next_request_id = w["next_request_id"]
    ent._in_flight = {int(x): {} for x in w["in_flight_ids"]}


def _write_hedge(r: _Results, i: int, ent) -> None:
    w = r.engine.hedge(i)
    (ent._total_requests, ent._primary_wins, ent._hedge_wins, ent._hedges_sent, ent._hedges_cancelled) = (
        w["total_requests"], w["primary_wins"], w["hedge_wins"], w["hedges_sent"], w["hedges_cancelled"])
    ent._next_request_id = w["next_request_id"]
    ent._in_flight = {int(rid): {"start_time": Instant(int(t0)), "completed": bool(done), "hedges_sent": int(sent),
                                 "responses_received": int(got)} for rid, t0, done, sent, got in w["entries"]}


def _write_fallback(r: _Results, i: int, ent) -> None:
    w = r.engine.hedge(i)
    (ent._total_requests, ent._primary_successes, ent._primary_failures, ent._fallback_invocations, ent._fallback_successes,
     ent._fallback_failures) = (w["total_requests"], w["primary_successes"], w["primary_failures"], w["fallback_invocations"],
                                w["fallback_successes"], w["fallback_failures"])
    ent._next_request_id = w["next_request_id"]
    ent._in_flight = {int(rid): {"start_time": Instant(int(t0)), "state": "fallback" if st else "primary"} for rid, t0, st in w["entries"]}


def _write_pool(r: _Results, i: int, ent) -> None:
    w = r.engine.stock(i)
    ent._available, ent._active, ent._completed, ent._rejected = w["available"], w["active"], w["completed"], w["rejected"]
    ent._queue = [None] * w["queued"]                     # (the waiting Requests stay on the device: one placeholder each)


def _write_inventory(r: _Results, i: int, ent) -> None:
    w = r.engine.stock(i)
    ent._stock, ent._stockouts, ent._reorders, ent._items_consumed, ent._items_replenished = (
        w["stock"], w["stockouts"], w["reorders"], w["items_consumed"], w["items_replenished"])
    ent._order_pending = bool(w["order_pending"])


def _write_limiter(r: _Results, i: int, ent) -> None:
    st = r.stats["limiters"][i]
    ent._received, ent._forwarded, ent._queued, ent._dropped = (int(st[k]) for k in ("received", "forwarded", "queued", "dropped"))
    ent._queue_depth, ent._poll_scheduled = int(st["queue_depth"]), bool(st["poll_scheduled"])
    ent._events = (int(st["requests_handled"]), int(st["polls_handled"]))
    sel = r.rows(i)                                       # its records: (time, hs_limiter_outcome), in processing order
    tt, code = r.rec_t[sel], r.rec_cr[sel]
    ent.received_times = [Instant(int(t)) for t in tt[code != N.LIMITER_DRAINED]]
    ent.forwarded_times = [Instant(int(t)) for t in tt[(code == N.LIMITER_FORWARDED) | (code == N.LIMITER_DRAINED)]]
    ent.dropped_times = [Instant(int(t)) for t in tt[code == N.LIMITER_DROPPED]]
    pol, when = ent.policy, (Instant(int(st["time_ns"])) if st["has_time"] else None)
    if st["policy"] == N.LIMITER_TOKEN_BUCKET:
        pol._tokens, pol._last_refill_time = float(st["tokens"]), when
    elif st["policy"] == N.LIMITER_LEAKY_BUCKET:
        pol._last_leak_time = when
    elif st["policy"] == N.LIMITER_SLIDING_WINDOW:
        pol._request_log = [Instant(int(t)) for t in st["log"]]
    else:
        pol._current_window_start, pol._current_window_count = when, int(st["count"])


def _write_probe(r: _Results, i: int, ent) -> None:
    sel = r.rows(i)                                       # its samples: (time, sampled integer)
    ent.data_sink._set(r.rec_t[sel].copy(), r.rec_cr[sel].copy(), Probe.value_map(ent.metric, ent.target))


def _write_router(r: _Results, i: int, ent) -> None:
    ent.stats_routed = int(r.stats["routed"][i])
    tc: dict[str, int] = {}
    off = int(r.a.rt_off[i])
    for q, t in enumerate(ent.targets):               # target_counts[target.name] += 1 (random_router.py:37)
        c = int(r.stats["rt_taken"][off + q])
        if c:
            tc[t.name] = tc.get(t.name, 0) + c
    ent.target_counts = tc


def _write_sink(r: _Results, i: int, ent) -> None:
    sel = r.rows(i)
    ent._set_records(r.rec_t[sel].copy(), r.rec_cr[sel].copy())
    ent._device = r.device


# the first class a node is an instance of decides; what is none of them is a Sink, a Counter or a LatencyTracker (a Network is a
# registry: traffic_matrix() reads its links)
_WRITE_BACK = ((Source, _write_source), (Server, _write_server), (NetworkLink, _write_link), (Network, lambda r, i, ent: None),
               (LoadBalancer, _write_load_balancer), (CanaryDeployer, _write_canary_deployer), (RollingDeployer, _write_rolling_deployer),
               (AutoScaler, _write_auto_scaler), (HealthChecker, _write_health_checker), (Bulkhead, _write_bulkhead),
               ((BatchProcessor, ConveyorBelt, GateController), _write_flow), (Client, _write_client), (TimeoutWrapper, _write_timeout_wrapper),
               (Hedge, _write_hedge), (Fallback, _write_fallback), (PooledCycleResource, _write_pool), (InventoryBuffer, _write_inventory),
               (RateLimitedEntity, _write_limiter), (Probe, _write_probe), (RandomRouter, _write_router))


def write_back_general(g: GeneralGraph, stats: dict, rec_node: np.ndarray, rec_t: np.ndarray, rec_cr: np.ndarray, device: int = 0,
                       engine=None) -> None:
    """The run's per-node results onto the user's objects, under the attribute names the reference uses (lowering.write_back's
    counterpart).  `engine`: the GraphEngine or PartRun that ran the graph -- the readers of its families (health, wrapper, client,
    flow, queue_policy, scaler, deployer, canary) are asked per node of their kind; a graph of Sources, Servers, links, routers,
    limiters, Probes and Sinks alone needs none."""
    r = _Results(g, stats, rec_node, rec_t, rec_cr, device, engine)
    for i, ent in enumerate(g.nodes):
        if not r.dormant(i):
            next((f for cls, f in _WRITE_BACK if isinstance(ent, cls)), _write_sink)(r, i, ent)
