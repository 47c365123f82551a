"""General entity graphs: what the lowered entity classes can be wired into beyond the station shape of lowering.lower().

The station engines take `[Sources] -> Server -> {Sink | NetworkLink | RandomRouter}` with one sender per link, at most four
Sources per Server, four router targets ...; lowering.lower() refuses the rest by name.  `lower_general()` takes exactly those
graphs -- a NetworkLink with several senders (components/network/link.py:114-189), a RandomRouter with any number of targets,
Servers and routers among them, and with several upstreams (components/random_router.py:32-45), Server(downstream=<Server>)
next to links (components/server/server.py:64-122), any number of Sources per Server (load/source.py:93-180), any
FixedConcurrency (server/concurrency.py:67-141) -- and runs them on the device's single-heap loop (csrc/hs_graph.hip,
include/hs_engine.h "General entity graphs"): the reference's own (time, _sort_index) order event by event, ~2.4 us per event on
one lane.  Exact, not fast: Simulation only comes here with a graph lower() refused.

Entity streams (DESIGN.md section 3 -- the one definition that is the engine's own): the k-th Source of `sources=[...]` draws
ARRIVAL from stream base k; the s-th Server / l-th NetworkLink / r-th RandomRouter in node order (entities in `entities=[...]`
order, then whatever is only reachable downstream, in discovery order) draws SERVICE / LINK + LOSS / ROUTE from base s / l / r.
For a graph built station by station this is the numbering of the station engines.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .core.temporal import Duration, Instant
from .entities import (CanaryDeployer, CanaryState, METRIC_EVALUATORS, LatencyEvaluator, DeploymentState, RollingDeployer, AutoScaler, SCALING_POLICIES, ScalingEvent, StepScaling, TargetUtilization,
                       BackendInfo,
                       AdaptiveLIFO, CoDelQueue, FIFOQueue, QUEUE_POLICIES, BatchProcessor, ConveyorBelt, GateController,
                       BackendHealthState, Bulkhead, Client, ClientKeyEventProvider, ConsistentHash, ConstantLatency, ConstantRateProfile, Counter, Entity,
                       ExponentialLatency, HealthChecker, IPHash, LIMITER_POLICIES, LatencyTracker, LeastConnections, LinearRampProfile, LoadBalancer, Network, NetworkLink, Probe, Random,
                       RandomRouter, RateLimitedEntity, RoundRobin, Server, SimpleEventProvider, Sink, SlidingWindowPolicy, Source,
                       DecorrelatedJitter, ExponentialBackoff, FixedRetry, NoRetry,
                       TimeoutWrapper, TokenBucketPolicy, WeightedLeastConnections, WeightedRoundRobin)

_STRATEGY_CODE = ((ConsistentHash, N.LB_CONSISTENT_HASH), (RoundRobin, N.LB_ROUND_ROBIN), (Random, N.LB_RANDOM),
                  (WeightedRoundRobin, N.LB_WEIGHTED_ROUND_ROBIN), (IPHash, N.LB_IP_HASH), (LeastConnections, N.LB_LEAST_CONNECTIONS),
                  (WeightedLeastConnections, N.LB_WEIGHTED_LEAST_CONNECTIONS))

_SINKS = (Sink, Counter, LatencyTracker)
DEFAULT_MAX_EVENTS = 200_000_000          # ~ minutes on the one lane; Simulation(max_graph_events=) raises it


def _ptr(a):
    return None if a is None else a.__array_interface__["data"][0]      # (the address; `.ctypes.data_as` costs 3 us per array)


class GraphArrays:
    """Struct-of-arrays form of hs_graph_nodes (include/hs_engine.h)."""

    def __init__(self, n: int):
        self.n = n
        self.kind = np.zeros(n, np.uint8)
        self.target = np.full(n, -1, np.int32)
        self.stream_base = np.zeros(n, np.uint64)
        self.src_kind = np.full(n, N.SRC_POISSON, np.uint8)
        self.src_rate = np.ones(n, np.float64)
        self.src_stop_after_ns = np.full(n, -1, np.int64)
        self.concurrency = np.ones(n, np.int32)
        self.lat_kind = np.full(n, N.LAT_CONSTANT, np.uint8)
        self.lat_mean_s = np.zeros(n, np.float64)
        self.link_lat_min_s = np.zeros(n, np.float64)
        self.link_loss_rate = np.zeros(n, np.float64)
        self.queue_cap = np.full(n, -1, np.int64)
        self.rt_off = np.zeros(n, np.int32)
        self.rt_cnt = np.zeros(n, np.int32)
        self.rt_targets = np.zeros(0, np.int32)
        self.src_profile_kind = None         # [n] uint8 / [n, 4] float64: Sources with a time-varying profile
        self.src_profile_params = None
        self.probe_metric = None             # [n] uint8 / [n] float64: PROBE nodes
        self.probe_interval_s = None
        self.lb_strategy = None              # [n] uint8 / [n] int32: LB nodes; names (bytes) / name_off [n + 1] int32: their backends' names
        self.lb_vnodes = None
        self.names = None
        self.name_off = None
        self.src_n_clients = None            # [n] int64: Sources with a ClientKeyEventProvider
        self.lb_weights = None               # [n_rt] int32: strategy.get_weight(backend) per backend slot of the weighted strategies
        self.lim_policy = None               # [n] uint8 hs_limiter_policy / [n, 3] float64 / [n] int64: RATE_LIMITER nodes
        self.lim_params = None               #   (hs_limiter_policy_params: p0, p1, p2 and count), set through
        self.lim_count = None                #   hs_graph_set_limiter_policy once the handle exists
        self.hc_params = None                # [n, 5] float64: HEALTH_CHECKER nodes -- interval, timeout, the two thresholds, _is_running
                                             #   (their LoadBalancer: `target`), set through hs_graph_set_health_checker
        self.lb_healthy = None               # [n_rt] uint8: BackendInfo.is_healthy per backend slot when the run begins (None: all healthy
                                             #   and no checker -- the graph has no health state)

        self.wrap_params = None              # [n, 5] float64: BULKHEAD nodes -- max_concurrent, max_wait_queue, max_wait_time (-1: None);
                                             #   TIMEOUT_WRAPPER nodes -- column 3 = timeout, column 4 = the in-flight table's first capacity
                                             #   (0: the engine's default); set through hs_graph_set_wrapper

        self.cl_params = None                # [n, 2] float64: CLIENT nodes -- timeout (-1: None), the in-flight table's first capacity
                                             #   (0: the engine's default); set through hs_graph_set_client with ...
        self.cl_delay_off = None             # [n + 1] int64 and
        self.cl_delays_ns = None             # int64: Duration.from_seconds(policy.get_delay(a)) for a = 1 .. max_attempts - 1 of every
                                             #   Client, back to back

        self.flow_params = None              # [n, 4] int64: BATCH_PROCESSOR / CONVEYOR / GATE nodes -- hs_graph_set_flow's count, delay_ns,
                                             #   aux_ns and flag (entities.BatchProcessor / ConveyorBelt / GateController)

        self.qp_params = None                # [n, 5] float64: SERVER nodes with a LIFOQueue / AdaptiveLIFO / CoDelQueue -- hs_queue_policy
                                             #   (0: the FIFO), capacity (-1: unbounded), congestion_threshold, target_delay, interval;
                                             #   set through hs_graph_set_queue_policy
        self.as_params = None                # [n, 10] float64: AUTO_SCALER nodes -- hs_autoscaler_policy, p0, p1, min_instances, max_instances,
                                             #   evaluation_interval, scale_out_cooldown, scale_in_cooldown, the pool's size P, _is_running
        self.as_steps = None                 #   ... and per node its StepScaling steps as [(threshold, adjustment), ...] (a list per node);
                                             #   set through hs_graph_set_auto_scaler (their LoadBalancer: `target`)
        # (kept out of vars(): tests/test_autoscaler_host.py::test_existing_lowering_is_unchanged_without_a_scaler hashes every public
        #  attribute of these arrays but the `as_*` ones against the digest of the commit before the AutoScaler -- a new plain attribute,
        #  even one that is None, would change what that test hashes)
        self._rd_params = None               # `rd_params`

    @property
    def rd_params(self):
        """[n, 5] float64 (None: no deployer): ROLLING_DEPLOYER nodes -- batch_size, health_check_interval, healthy_threshold,
        max_failures, the pool's size P; set through hs_graph_set_rolling_deployer (their LoadBalancer: `target`)."""
        return self._rd_params

    @rd_params.setter
    def rd_params(self, value):
        self._rd_params = value

    @property
    def has_deployers(self) -> bool:
        return self._rd_params is not None

    @property
    def cn_params(self):
        """per node (None: no canary deployer; kept out of vars() like `rd_params`): None or (stages as [(traffic_percentage,
        evaluation_period), ...], hs_canary_evaluator, its limit, its threshold_multiplier, evaluation_interval) of a CANARY_DEPLOYER
        node; set through hs_graph_set_canary_deployer (its LoadBalancer: `target`)."""
        return getattr(self, "_cn_params", None)

    @cn_params.setter
    def cn_params(self, value):
        self._cn_params = value

    @property
    def has_canaries(self) -> bool:
        return self.cn_params is not None

    @property
    def has_scalers(self) -> bool:
        return self.as_params is not None

    @property
    def has_queue_policies(self) -> bool:
        return self.qp_params is not None

    @property
    def has_flows(self) -> bool:
        return self.flow_params is not None

    @property
    def has_clients(self) -> bool:
        return self.cl_params is not None

    @property
    def has_health(self) -> bool:
        return self.hc_params is not None or self.lb_healthy is not None

    @property
    def has_wrappers(self) -> bool:
        return self.wrap_params is not None

    def struct(self) -> N.GraphNodes:
        s = N.GraphNodes()
        s.n_nodes = self.n
        for name in ("kind", "target", "stream_base", "src_kind", "src_rate", "src_stop_after_ns", "concurrency", "lat_kind",
                     "lat_mean_s", "link_lat_min_s", "link_loss_rate", "queue_cap", "rt_off", "rt_cnt"):
            setattr(s, name, _ptr(getattr(self, name)))
        self.rt_targets = np.ascontiguousarray(self.rt_targets, np.int32)
        s.rt_targets = _ptr(self.rt_targets) if len(self.rt_targets) else None
        s.n_rt = len(self.rt_targets)
        for name in ("src_profile_kind", "src_profile_params", "probe_metric", "probe_interval_s", "lb_strategy", "lb_vnodes", "name_off",
                     "src_n_clients"):
            setattr(s, name, _ptr(getattr(self, name)))
        if self.names is not None:
            self._names_buf = C.create_string_buffer(self.names, max(len(self.names), 1))
            s.names = C.cast(self._names_buf, C.c_void_p)
        return s


class GraphEngine:
    """ctypes handle of one hs_graph.  No CPU fallback: without the library or a GPU the constructor raises."""

    def __init__(self, arrays: GraphArrays, *, seed: int = 42, start_ns: int = 0, device: int = 0, max_events: int = 0,
                 heap_capacity: int = 0, request_capacity: int = 0, record_capacity: int = 0, profile_budget: int = 0,
                 table_capacity: int = 0):
        self._lib = N.lib()
        self.arrays = arrays
        cfg = N.GraphConfig(struct_size=C.sizeof(N.GraphConfig), device=device, start_ns=start_ns, seed=seed,
                            heap_capacity=heap_capacity, request_capacity=request_capacity, record_capacity=record_capacity,
                            max_events=max_events, profile_budget=profile_budget)
        h = C.c_void_p()
        nodes = arrays.struct()
        rc = self._lib.hs_graph_create(C.byref(cfg), C.byref(nodes), C.byref(h))
        if rc != N.HS_OK:
            msg = (self._lib.hs_graph_last_error(None) or b"").decode()
            if rc == N.HS_E_NO_DEVICE:
                raise N.EngineUnavailable(msg)
            raise N.EngineError(rc, msg)
        self._h = h
        self._fault_tags: list = []          # per hs_graph_add_fault / hs_graph_add_link_fault call: the caller's tag of a link fault Event
        if arrays.lb_weights is not None and arrays.lb_strategy is not None:
            # WeightedRoundRobin / WeightedLeastConnections: strategy._weights, per LoadBalancer in slot order (the default is all ones)
            w = np.ascontiguousarray(arrays.lb_weights, np.int32)
            try:
                for i in np.nonzero((arrays.kind == N.NODE_LB) & ((arrays.lb_strategy == N.LB_WEIGHTED_ROUND_ROBIN) |
                                                                  (arrays.lb_strategy == N.LB_WEIGHTED_LEAST_CONNECTIONS)))[0]:
                    off, cnt = int(arrays.rt_off[i]), int(arrays.rt_cnt[i])
                    wi = np.ascontiguousarray(w[off:off + cnt])
                    if cnt and (wi != 1).any():
                        self._check(self._lib.hs_graph_set_lb_weights(self._h, int(i), _ptr(wi), cnt))
            except BaseException:
                self.close()
                raise

        if arrays.lim_policy is not None:
            try:
                for i in np.nonzero(arrays.kind == N.NODE_RATE_LIMITER)[0]:
                    q = N.LimiterPolicyParams(C.sizeof(N.LimiterPolicyParams), int(arrays.lim_policy[i]), *(float(v) for v in arrays.lim_params[i]),
                                              int(arrays.lim_count[i]))
                    self._check(self._lib.hs_graph_set_limiter_policy(self._h, int(i), C.byref(q)))
            except BaseException:
                self.close()
                raise

        if arrays.has_health:
            try:
                if arrays.lb_healthy is not None:
                    fl = np.ascontiguousarray(arrays.lb_healthy, np.uint8)
                    for i in np.nonzero(arrays.kind == N.NODE_LB)[0]:
                        off, cnt = int(arrays.rt_off[i]), int(arrays.rt_cnt[i])
                        fi = np.ascontiguousarray(fl[off:off + cnt])
                        self._check(self._lib.hs_graph_set_lb_health(self._h, int(i), _ptr(fi) if cnt else _ptr(np.zeros(1, np.uint8)), cnt))
                for i in np.nonzero(arrays.kind == N.NODE_HEALTH_CHECKER)[0]:
                    iv, to, ht, ut, running = arrays.hc_params[i]
                    self._check(self._lib.hs_graph_set_health_checker(self._h, int(i), int(arrays.target[i]), float(iv), float(to), int(ht), int(ut),
                                                                      int(running)))
            except BaseException:
                self.close()
                raise

        if arrays.has_scalers:
            try:
                for i in np.nonzero(arrays.kind == N.NODE_AUTO_SCALER)[0]:
                    pol, p0, p1, lo, hi, iv, cd_out, cd_in, pool, running = arrays.as_params[i]
                    steps = arrays.as_steps[i] or []
                    thr = np.array([t for t, _ in steps] or [0.0], np.float64)
                    adj = np.array([a for _, a in steps] or [0], np.int32)
                    self._check(self._lib.hs_graph_set_auto_scaler(self._h, int(i), int(arrays.target[i]), int(pol), float(p0), float(p1), len(steps),
                                                                   _ptr(thr), _ptr(adj), int(lo), int(hi), float(iv), float(cd_out), float(cd_in),
                                                                   int(pool), int(running)))
            except BaseException:
                self.close()
                raise

        if arrays.has_deployers:
            try:
                for i in np.nonzero(arrays.kind == N.NODE_ROLLING_DEPLOYER)[0]:
                    batch, iv, thr, fails, pool = arrays.rd_params[i]
                    self._check(self._lib.hs_graph_set_rolling_deployer(self._h, int(i), int(arrays.target[i]), int(batch), float(iv), int(thr),
                                                                        int(fails), int(pool)))
            except BaseException:
                self.close()
                raise

        if arrays.has_canaries:
            try:
                for i in np.nonzero(arrays.kind == N.NODE_CANARY_DEPLOYER)[0]:
                    stages, evaluator, limit, mult, iv = arrays.cn_params[i]
                    pct = np.array([s_[0] for s_ in stages], np.float64)
                    period = np.array([s_[1] for s_ in stages], np.float64)
                    self._check(self._lib.hs_graph_set_canary_deployer(self._h, int(i), int(arrays.target[i]), len(stages), _ptr(pct), _ptr(period),
                                                                       int(evaluator), float(limit), float(mult), float(iv)))
            except BaseException:
                self.close()
                raise

        if arrays.has_wrappers:
            try:
                for i in np.nonzero((arrays.kind == N.NODE_BULKHEAD) | (arrays.kind == N.NODE_TIMEOUT_WRAPPER))[0]:
                    mc, mq, mw, to, cap = arrays.wrap_params[i]
                    self._check(self._lib.hs_graph_set_wrapper(self._h, int(i), int(mc), int(mq), float(mw), float(to),
                                                               int(table_capacity) if table_capacity else int(cap)))
            except BaseException:
                self.close()
                raise

        if arrays.has_clients:
            try:
                for i in np.nonzero(arrays.kind == N.NODE_CLIENT)[0]:
                    timeout, cap = arrays.cl_params[i]
                    delays = np.ascontiguousarray(arrays.cl_delays_ns[arrays.cl_delay_off[i]:arrays.cl_delay_off[i + 1]], np.int64)
                    self._check(self._lib.hs_graph_set_client(self._h, int(i), float(timeout), _ptr(delays) if len(delays) else None, len(delays),
                                                              int(table_capacity) if table_capacity else int(cap)))
            except BaseException:
                self.close()
                raise

        if arrays.has_flows:
            try:
                for i in np.nonzero((arrays.kind >= N.NODE_BATCH_PROCESSOR) & (arrays.kind <= N.NODE_GATE))[0]:
                    count, delay_ns, aux_ns, flag = (int(v) for v in arrays.flow_params[i])
                    self._check(self._lib.hs_graph_set_flow(self._h, int(i), count, delay_ns, aux_ns, flag))
            except BaseException:
                self.close()
                raise

        if arrays.has_queue_policies:
            try:
                for i in np.nonzero((arrays.kind == N.NODE_SERVER) & (arrays.qp_params[:, 0] != N.QUEUE_FIFO))[0]:
                    pol, cap, thr, target, interval = arrays.qp_params[i]
                    self._check(self._lib.hs_graph_set_queue_policy(self._h, int(i), int(pol), int(cap), int(thr), float(target), float(interval)))
            except BaseException:
                self.close()
                raise

    _QUEUE_NAMES = ("policy", "len", "enqueued", "dequeued_fifo", "dequeued_lifo", "dropped", "capacity_rejected", "switches", "flag",
                    "count", "last_count", "has_first_above", "first_above_ns", "has_drop_next", "drop_next_ns")

    def queue_policy(self, node: int) -> dict:
        """hs_graph_get_queue_policy of a Server with a LIFOQueue, an AdaptiveLIFO or a CoDelQueue: its state by name (`dequeued_fifo`
        is a CoDelQueue's `dequeued`, `switches` its `drop_intervals` / an AdaptiveLIFO's `mode_switches`, `flag` `_dropping` /
        `_was_congested`)."""
        out = np.zeros(N.QUEUE_FIELDS, np.int64)
        self._check(self._lib.hs_graph_get_queue_policy(self._h, int(node), _ptr(out)))
        return {k: int(v) for k, v in zip(self._QUEUE_NAMES, out)}

    _FLOW_NAMES = {N.NODE_BATCH_PROCESSOR: ("batches_processed", "items_processed", "timeouts", "buffer_depth"),
                   N.NODE_CONVEYOR: ("items_transported", "items_rejected", "items_in_transit"),
                   N.NODE_GATE: ("passed_through", "queued_while_closed", "rejected", "open_cycles", "queue_depth", "is_open")}

    def flow(self, node: int) -> dict:
        """hs_graph_get_flow of a BatchProcessor, ConveyorBelt or GateController node: its counters by name."""
        c = np.zeros(N.FLOW_COUNTERS, np.int64)
        self._check(self._lib.hs_graph_get_flow(self._h, int(node), _ptr(c), None, None))
        return {k: int(v) for k, v in zip(self._FLOW_NAMES[int(self.arrays.kind[node])], c)}

    def flow_events(self) -> np.ndarray:
        """The graph's Events of the eight flow kinds (item / timeout / batch continuation, item / transit continuation, item / open /
        close) and, last, the cancelled `_BatchTimeout` Events it popped."""
        events, cancelled = np.zeros(N.FLOW_KINDS + 1, np.int64), C.c_int64(0)
        self._check(self._lib.hs_graph_get_flow(self._h, -1, None, _ptr(events), C.byref(cancelled)))
        events[N.FLOW_KINDS] = cancelled.value
        return events

    def client(self, node: int) -> dict:
        """hs_graph_get_client of a Client node: its counters by name and the keys in flight as sorted (request_id or 0, attempt) rows."""
        c = np.zeros(N.CLIENT_COUNTERS, np.int64)
        self._check(self._lib.hs_graph_get_client(self._h, int(node), _ptr(c), None, 0, None))
        live = int(c[5])
        keys = np.zeros((max(live, 1), 2), np.int64)
        self._check(self._lib.hs_graph_get_client(self._h, int(node), None, _ptr(keys), live, None))
        keys = keys[:live]
        out = {k: int(v) for k, v in zip(("requests_sent", "responses_received", "timeouts", "retries", "failures", "in_flight_count",
                                           "table_capacity"), c)}
        out["in_flight_keys"] = keys[np.lexsort((keys[:, 1], keys[:, 0]))]
        return out

    def client_events(self) -> np.ndarray:
        """The graph's Client request / response / timeout Events of the run."""
        events = np.zeros(3, np.int64)
        self._check(self._lib.hs_graph_get_client(self._h, -1, None, None, 0, _ptr(events)))
        return events

    def wrapper(self, node: int) -> dict:
        """hs_graph_get_wrapper of a Bulkhead or TimeoutWrapper node: its counters by name, the ids of its wait queue (head first) and
        the ids in flight (ascending)."""
        c = np.zeros(N.WRAPPER_COUNTERS, np.int64)
        self._check(self._lib.hs_graph_get_wrapper(self._h, int(node), _ptr(c), None, 0, None, 0, None))
        queue, live = np.zeros(max(int(c[8]), 1), np.int64), np.zeros(max(int(c[10]), 1), np.int64)
        self._check(self._lib.hs_graph_get_wrapper(self._h, int(node), None, _ptr(queue), int(c[8]), _ptr(live), int(c[10]), None))
        names = ("total", "accepted", "rejected", "timed_out", "queued", "peak_concurrent", "peak_queue_depth", "active_count", "queue_depth",
                 "next_request_id", "in_flight_count", "table_capacity")
        if self.arrays.kind[node] == N.NODE_TIMEOUT_WRAPPER:
            names = ("total", "successful", "timed_out") + ("",) * 6 + names[9:]
        out = {k: int(v) for k, v in zip(names, c) if k}
        out["queue_ids"] = queue[:int(c[8])]
        out["in_flight_ids"] = np.sort(live[:int(c[10])])
        return out

    def wrapper_events(self) -> np.ndarray:
        """The graph's Bulkhead request / response / timeout and TimeoutWrapper request / response / timeout Events of the run."""
        events = np.zeros(6, np.int64)
        self._check(self._lib.hs_graph_get_wrapper(self._h, -1, None, None, 0, None, 0, _ptr(events)))
        return events

    _SCALER_NAMES = ("evaluations", "scale_out_count", "scale_in_count", "instances_added", "instances_removed", "cooldown_blocks",
                     "next_instance_id", "last_action", "last_time_ns", "history_len", "members")

    def scaler(self, node: int) -> dict:
        """hs_graph_get_auto_scaler of an AutoScaler node: its state by name, `history` as rows (time ns, action, from_count, to_count,
        the instances the action counted) and `member`, the membership word of every target of its LoadBalancer."""
        a = self.arrays
        cnt = int(a.rt_cnt[int(a.target[node])])
        st, member = np.zeros(N.AUTOSCALER_FIELDS, np.int64), np.zeros(max(cnt, 1), np.uint8)
        self._check(self._lib.hs_graph_get_auto_scaler(self._h, int(node), _ptr(st), None, 0, _ptr(member), None))
        hist = np.zeros((max(int(st[9]), 1), 4), np.int64)
        self._check(self._lib.hs_graph_get_auto_scaler(self._h, int(node), None, _ptr(hist), int(st[9]), None, None))
        hist = hist[:int(st[9])]
        out = {k: int(v) for k, v in zip(self._SCALER_NAMES, st)}
        out["history"] = np.concatenate([hist[:, :1], hist[:, 1:2] & 3, hist[:, 2:], hist[:, 1:2] >> 2], axis=1)
        out["member"] = member[:cnt]
        return out

    def scaler_events(self) -> int:
        """The graph's `_autoscaler_evaluate` Events of the run (hs_graph_get_auto_scaler, node = -1)."""
        events = C.c_int64(0)
        self._check(self._lib.hs_graph_get_auto_scaler(self._h, -1, None, None, 0, None, C.byref(events)))
        return int(events.value)

    _DEPLOYER_NAMES = ("deployments_started", "deployments_completed", "deployments_rolled_back", "instances_replaced",
                       "health_checks_performed", "health_checks_passed", "health_checks_failed", "status", "total_instances", "replaced",
                       "failed", "current_batch", "next_instance_id", "health_fail_count", "n_old", "n_new", "n_batch_old", "n_batch_new",
                       "n_members")

    def deployer(self, node: int) -> dict:
        """hs_graph_get_rolling_deployer of a RollingDeployer node: its state by name, `old` / `new` / `batch_old` / `batch_new` and
        `members` (the LoadBalancer's, in order) as lists of slots, `pass_count` as {slot: count}, `readded`: the slots a rollback
        added again."""
        a = self.arrays
        cnt = max(int(a.rt_cnt[int(a.target[node])]), 1)
        st, lists = np.zeros(N.DEPLOYER_FIELDS, np.int64), np.full(4 * cnt, -1, np.int32)
        members, passes, readded = np.full(cnt, -1, np.int32), np.full(cnt, -1, np.int32), np.zeros(cnt, np.int32)
        self._check(self._lib.hs_graph_get_rolling_deployer(self._h, int(node), _ptr(st), _ptr(lists), _ptr(members), _ptr(passes), _ptr(readded),
                                                            None))
        out = {k: int(v) for k, v in zip(self._DEPLOYER_NAMES, st)}
        for j, (nm, ln) in enumerate((("old", "n_old"), ("new", "n_new"), ("batch_old", "n_batch_old"), ("batch_new", "n_batch_new"))):
            out[nm] = lists[j * cnt:j * cnt + out[ln]].tolist()
        out["members"] = members[:out["n_members"]].tolist()
        out["pass_count"] = {int(q): int(v) for q, v in enumerate(passes) if v >= 0}
        out["readded"] = np.nonzero(readded)[0].tolist()
        return out

    _CANARY_NAMES = ("deployments_started", "deployments_completed", "deployments_rolled_back", "stages_completed", "evaluations_performed",
                     "evaluations_passed", "evaluations_failed", "status", "current_stage", "total_stages", "has_canary", "stage_start_ns",
                     "n_baseline", "n_members")

    def canary(self, node: int) -> dict:
        """hs_graph_get_canary_deployer of a CanaryDeployer node: its state by name, `traffic_pct`, `baseline` and `members` (the
        LoadBalancer's, in order) as lists of slots, `weights` / `weight_set` / `service_sum` / `service_count` per slot."""
        a = self.arrays
        cnt = max(int(a.rt_cnt[int(a.target[node])]), 1)
        st, pct = np.zeros(N.CANARY_FIELDS, np.int64), C.c_double(0.0)
        base, members, weights, wset = (np.full(cnt, -1, np.int32) for _ in range(4))
        ssum, scnt = np.zeros(cnt, np.float64), np.zeros(cnt, np.int64)
        self._check(self._lib.hs_graph_get_canary_deployer(self._h, int(node), _ptr(st), C.byref(pct), _ptr(base), _ptr(members), _ptr(weights),
                                                           _ptr(wset), _ptr(ssum), _ptr(scnt), None))
        out = {k: int(v) for k, v in zip(self._CANARY_NAMES, st)}
        out.update(traffic_pct=float(pct.value), baseline=base[:out["n_baseline"]].tolist(), members=members[:out["n_members"]].tolist(),
                   weights=weights.tolist(), weight_set=np.nonzero(wset > 0)[0].tolist(), service_sum=ssum, service_count=scnt)
        return out

    def canary_events(self) -> np.ndarray:
        """The graph's canary deployer Events of the run by kind (hs_graph_get_canary_deployer, node = -1)."""
        events = np.zeros(N.CANARY_KINDS, np.int64)
        self._check(self._lib.hs_graph_get_canary_deployer(self._h, -1, None, None, None, None, None, None, None, None, _ptr(events)))
        return events

    def deployer_events(self) -> np.ndarray:
        """The graph's deployer Events of the run by kind (hs_graph_get_rolling_deployer, node = -1)."""
        return self._deployer_counts()[:N.DEPLOYER_KINDS]

    def deployer_compactions(self) -> tuple:
        """(by the lone lane, by all 64 lanes): the member lists this graph compacted behind a removal so far."""
        both = self._deployer_counts()[N.DEPLOYER_KINDS:]
        return int(both[0]), int(both[1])

    @staticmethod
    def compact_members(members, member_flags, wave: bool, device: int = 0) -> list:
        """hs_debug_compact_members: `members` (slots in insertion order) without the slots whose flag is 0, order kept -- compacted on
        the device by the lone lane or, `wave`, by all 64 lanes."""
        lst = np.ascontiguousarray(members, np.int32).copy()
        flags = np.ascontiguousarray(member_flags, np.uint8)
        out = C.c_int32(0)
        rc = N.lib().hs_debug_compact_members(int(device), len(flags), len(lst), _ptr(lst) if len(lst) else None, _ptr(flags) if len(flags) else None,
                                              int(bool(wave)), C.byref(out))
        if rc < 0:
            raise N.EngineError(rc, "hs_debug_compact_members")
        return lst[:out.value].tolist()

    def _deployer_counts(self) -> np.ndarray:
        events = np.zeros(N.DEPLOYER_KINDS + 2, np.int64)
        self._check(self._lib.hs_graph_get_rolling_deployer(self._h, -1, None, None, None, None, None, _ptr(events)))
        return events

    def health(self, node: int) -> dict:
        """hs_graph_get_health of a HealthChecker or LoadBalancer node: checker stats, per-backend states, the LoadBalancer's health
        flags and mark counts, the graph's three health event counts -- and the live WeightedRoundRobin current weights (None without
        health state)."""
        a = self.arrays
        lb = int(node) if a.kind[node] == N.NODE_LB else int(a.target[node])
        cnt = int(a.rt_cnt[lb])
        stats, states, flags = np.zeros(6, np.int64), np.zeros((max(cnt, 1), 6), np.int64), np.ones(max(cnt, 1), np.uint8)
        marks, events, cur = np.zeros(2, np.int64), np.zeros(3, np.int64), np.zeros(max(cnt, 1), np.int64)
        self._check(self._lib.hs_graph_get_health(self._h, int(node), _ptr(stats), _ptr(states), _ptr(flags), _ptr(marks), _ptr(events)))
        seen = np.zeros(max(cnt, 1), np.uint8)
        live = self._check(self._lib.hs_graph_get_lb_current_weights(self._h, lb, _ptr(cur), _ptr(seen), cnt))
        # current_weights: {backend slot: weight} of the slots the reference's dict has an entry for (None without health state)
        return dict(stats=stats, states=states[:cnt], healthy=flags[:cnt], marks=marks, events=events,
                    current_weights={q: int(cur[q]) for q in range(cnt) if seen[q]} if live else None)

    def health_events(self) -> np.ndarray:
        """The graph's cycle / response / timeout Events of the run (hs_graph_get_health, node = -1)."""
        events = np.zeros(3, np.int64)
        self._check(self._lib.hs_graph_get_health(self._h, -1, None, None, None, None, _ptr(events)))
        return events

    def limiter(self, node: int) -> dict:
        """hs_graph_get_limiter: counters, queue depth, the two event counts and the policy's state of limiter `node`."""
        st = N.LimiterState(struct_size=C.sizeof(N.LimiterState))
        sliding = self.arrays.lim_policy is not None and self.arrays.lim_policy[node] == N.LIMITER_SLIDING_WINDOW
        log = np.zeros(int(self.arrays.lim_count[node]) if sliding else 0, np.int64)      # (max_requests bounds the log)
        self._check(self._lib.hs_graph_get_limiter(self._h, int(node), C.byref(st), _ptr(log) if len(log) else None, len(log)))
        out = {name: getattr(st, name) for name, _ in N.LimiterState._fields_[1:]}
        out["log"] = log[:st.count] if sliding else log
        return out

    def set_debug_flags(self, flags: int) -> None:
        """hs_debug_graph_flags: N.GRAPH_DEBUG_LANE_SERIAL / N.GRAPH_DEBUG_COOPERATIVE force where least-loaded selections run."""
        self._check(self._lib.hs_debug_graph_flags(self._h, int(flags)))

    def coop_selects(self) -> int:
        """Least-loaded selections of the last run that all 64 lanes took (hs_graph_coop_selects)."""
        return int(self._check(self._lib.hs_graph_coop_selects(self._h)))

    def _check(self, rc: int):
        if rc < 0:
            raise N.EngineError(rc, (self._lib.hs_graph_last_error(self._h) or b"").decode())
        return rc

    def schedule(self, node: int, time_ns: int, request_id: int | None = None, gate_open: bool | None = None) -> None:
        """hs_graph_schedule; with a `request_id` (0: none) hs_graph_schedule_client: Client.send_request's Event; with `gate_open`
        hs_graph_schedule_gate: a GateController's `_GateOpen` / `_GateClose` Event."""
        if gate_open is not None:
            self._check(self._lib.hs_graph_schedule_gate(self._h, int(node), int(time_ns), int(bool(gate_open))))
        elif request_id is None:
            self._check(self._lib.hs_graph_schedule(self._h, int(node), int(time_ns)))
        else:
            self._check(self._lib.hs_graph_schedule_client(self._h, int(node), int(time_ns), int(request_id)))

    def add_fault(self, node: int, time_ns: int, on: bool, cancelled: bool = False) -> None:
        """hs_graph_add_fault: one fault Event (set / clear the crashed flag of `node`), numbered in call order."""
        self._check(self._lib.hs_graph_add_fault(self._h, int(node), int(time_ns), int(bool(on)), int(bool(cancelled))))
        self._fault_tags.append(None)

    def add_link_fault(self, node: int, time_ns: int, what: str, on: bool, value: float, cancelled: bool = False, tag=None) -> None:
        """hs_graph_add_link_fault: one Event of an InjectLatency (`what` = "latency") or an InjectPacketLoss ("loss") on link `node`,
        numbered in call order with add_fault's.  `tag` comes back from link_faults() while this Event's activation is in force."""
        if what not in ("latency", "loss"):
            raise ValueError(f"add_link_fault: what = {what!r} is neither 'latency' nor 'loss'")
        code = N.LINK_FAULT_LATENCY if what == "latency" else N.LINK_FAULT_LOSS
        self._check(self._lib.hs_graph_add_link_fault(self._h, int(node), int(time_ns), code, int(bool(on)), float(value), int(bool(cancelled))))
        self._fault_tags.append(tag)

    def add_faults(self, entries) -> None:
        """Simulation._general_faults' entries in their order: (node, ns, on, cancelled) of a node fault, (node, ns, on, cancelled,
        LinkFaultEvent) of a link fault."""
        for node, t, on, cancelled, *lf in entries:
            if lf:
                self.add_link_fault(node, t, lf[0].what, on, lf[0].value, cancelled, tag=lf[0])
            else:
                self.add_fault(node, t, on, cancelled)

    def link_faults(self) -> dict:
        """hs_graph_get_link_faults: {link node: (tag of the latency activation in force or None, tag of the loss activation in force
        or None, values read from the LOSS stream)}."""
        n = self.arrays.n
        lat, loss, draws = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        self._check(self._lib.hs_graph_get_link_faults(self._h, _ptr(lat), _ptr(loss), _ptr(draws)))
        tags = self._fault_tags
        return {int(i): (tags[lat[i]] if lat[i] >= 0 else None, tags[loss[i]] if loss[i] >= 0 else None, int(draws[i]))
                for i in np.nonzero(self.arrays.kind == N.NODE_LINK)[0]}

    def faults(self):
        """hs_graph_get_faults: (crashed flag per node, the four internal kinds' event counts -- limiter Requests, limiter polls,
        fault set, fault clear --, cancelled fault Events popped)."""
        crashed, internal = np.zeros(self.arrays.n, np.uint8), np.zeros(4, np.int64)
        cancelled = C.c_int64(0)
        self._check(self._lib.hs_graph_get_faults(self._h, _ptr(crashed), _ptr(internal), C.byref(cancelled)))
        return crashed, internal, int(cancelled.value)

    def run_until(self, end_ns: int) -> None:
        self._check(self._lib.hs_graph_run_until(self._h, int(end_ns)))

    @staticmethod
    def run_many(engines: list, end_ns: int) -> None:
        """hs_graph_run_many: independent graphs (replicas, sweep points) to `end_ns` side by side, one workgroup each."""
        if not engines:
            return
        hs_ = (C.c_void_p * len(engines))(*[e._h for e in engines])
        rc = engines[0]._lib.hs_graph_run_many(hs_, len(engines), int(end_ns))
        engines[0]._check(rc)

    def summary(self) -> N.Summary:
        s = N.Summary()
        self._check(self._lib.hs_graph_get_summary(self._h, C.byref(s)))
        return s

    def stats(self) -> dict:
        n, nrt = self.arrays.n, max(len(self.arrays.rt_targets), 1)
        out = {k: np.zeros(nrt if k == "rt_taken" else (n, 6) if k == "lb" else n, np.float64 if k == "total_service_s" else np.int64)
               for k in N.GRAPH_STATS}
        st = N.GraphStats()
        for k, a in out.items():
            setattr(st, k, _ptr(a))
        self._check(self._lib.hs_graph_get_stats(self._h, C.byref(st)))
        out["rt_taken"] = out["rt_taken"][:len(self.arrays.rt_targets)]
        out["limiters"] = {int(i): self.limiter(int(i)) for i in np.nonzero(self.arrays.kind == N.NODE_RATE_LIMITER)[0]}
        return out

    def records(self):
        """(Sink node, completion ns, created_at ns) of every Sink record, in processing order."""
        n = self._check(self._lib.hs_graph_read_records(self._h, None, None, None, 0))
        node, t, cr = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        if n:
            self._check(self._lib.hs_graph_read_records(self._h, _ptr(node), _ptr(t), _ptr(cr), n))
        return node, t, cr

    def close(self):
        if self._h:
            self._lib.hs_graph_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class GeneralGraph:
    """The node list of one Simulation: Sources in `sources=[...]` order, then the other entities."""

    def __init__(self, nodes: list, arrays: GraphArrays, node_of: dict):
        self.nodes = nodes              # entity objects by node id
        self.arrays = arrays
        self.node_of = node_of          # id(entity) -> node id
        self.scaled = {}                # LoadBalancer node -> (its AutoScaler's node, its initial backends, the pool's Servers)
        self.pool_of = {}               # pool Server node -> (its AutoScaler's node, its instance id k)
        self.n_own = len(nodes)         # the Simulation's own nodes; the scalers' pools stand behind them
        self.scaler_starts = 1          # the start() Events per scaler the pools were sized for
        self.deployed = {}              # LoadBalancer node -> (its RollingDeployer's node, its initial backends, the pool's Servers)
        self.dpool_of = {}              # pool Server node -> (its RollingDeployer's node, its instance id k)
        self.deploys = {}               # RollingDeployer node -> the deploy() Events its pool was sized for
        self.rr_base = {}               # scaled LoadBalancer node -> its RoundRobin's `_index` when the graph was lowered


def client_delay_table(policy, what: str) -> np.ndarray:
    """Duration.from_seconds(policy.get_delay(a)) in whole nanoseconds for a = 1 .. max_attempts - 1: what a Client's timeout handler
    adds to `now` for the retry of attempt a (client.py:393-410).  The device never evaluates a policy."""
    from .lowering import UnsupportedTopology

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


_FLOWS = (BatchProcessor, ConveyorBelt, GateController)
_FLOW_METRIC_OF = {"buffer_depth": BatchProcessor, "items_in_transit": ConveyorBelt, "queue_depth": GateController}


def _flow_target_refusal(what: str, end, tgt) -> str:
    via = " (through its NetworkLinks)" if end is not tgt else ""
    return (f"{what}: its target{via} is the {type(end).__name__} '{end.name}' -- a completion hook on an item that a BatchProcessor, "
            "ConveyorBelt or GateController holds is not lowered (a follow-up)")


def flow_delay_ns(seconds, what: str, name: str) -> int:
    """int(seconds * 1_000_000_000): what `Instant + seconds` adds to `now` (core/temporal.py:213-222) -- it does not depend on `now`,
    so the device gets whole nanoseconds."""
    from .lowering import UnsupportedTopology

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


def lower_general(sources: list, entities: list, probes=None, *, start_ns: int = 0, end_ns: int | None = None,
                  scaler_starts: int = 1, deploys: dict | None = None) -> GeneralGraph:
    """`sources` / `entities` of a Simulation -> the node arrays of the single-heap engine.  Refuses by name what that engine
    does not run either (lowering.UnsupportedTopology).  `start_ns` / `end_ns` (None: Infinity) / `scaler_starts` (the start() Events
    scheduled per scaler) size the instance pools of the AutoScalers."""
    from .lowering import UnsupportedTopology

    nodes: list = []
    node_of: dict[int, int] = {}

    def add(ent):
        if id(ent) not in node_of:
            node_of[id(ent)] = len(nodes)
            nodes.append(ent)
        return node_of[id(ent)]

    for src in sources or []:
        if not isinstance(src, Source):
            raise UnsupportedTopology(f"source {type(src).__name__} is not a lowered Source")
        if id(src) in node_of:
            raise UnsupportedTopology(f"source '{src.name}' is listed twice")
        add(src)
    n_src = len(nodes)
    for pr in probes or []:                                   # PROBE nodes behind the Sources, in `probes=[...]` order
        if not isinstance(pr, Probe):
            raise UnsupportedTopology(f"probe {type(pr).__name__} is not a lowered Probe")
        if id(pr) in node_of:
            raise UnsupportedTopology(f"probe '{pr.name}' is listed twice")
        add(pr)
    n_front = len(nodes)
    lowered = (Server, NetworkLink, RandomRouter, LoadBalancer, RateLimitedEntity, HealthChecker, Bulkhead, TimeoutWrapper, Client,
               BatchProcessor, ConveyorBelt, GateController, AutoScaler, RollingDeployer, CanaryDeployer) + _SINKS

    def check(ent, where):
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
        if isinstance(ent, HealthChecker) and where != "entities":
            raise UnsupportedTopology(f"{where}: the HealthChecker '{ent.name}' takes no Requests")
        if isinstance(ent, AutoScaler) and where != "entities":
            raise UnsupportedTopology(f"{where}: the AutoScaler '{ent.name}' takes no Requests")
        if isinstance(ent, (RollingDeployer, CanaryDeployer)) and where != "entities":
            raise UnsupportedTopology(f"{where}: the {type(ent).__name__} '{ent.name}' takes no Requests")
        if not isinstance(ent, lowered):
            raise UnsupportedTopology(f"{where}: {type(ent).__name__} '{getattr(ent, 'name', ent)}' is not lowered to the engine")

    for ent in entities or []:
        if isinstance(ent, Source):
            if id(ent) not in node_of:
                raise UnsupportedTopology(f"source '{ent.name}' is listed in entities but not in sources: it would never start")
            continue
        if not isinstance(ent, Entity):
            raise UnsupportedTopology(f"object {ent!r} is not an Entity")
        if isinstance(ent, Network):
            add(ent)                                          # its place in the entity order; nothing forwards to it (check())
            continue
        check(ent, "entities")
        add(ent)
    # whatever is only reachable downstream (the reference never needs it listed: events carry their target), in discovery order
    k = 0
    while k < len(nodes):
        ent = nodes[k]
        k += 1
        if isinstance(ent, (Probe, HealthChecker, AutoScaler, RollingDeployer, CanaryDeployer)):   # (a checker's / scaler's LoadBalancer has to be part of the Simulation by itself)
            continue
        for d in ent.downstream_entities():
            if d is None:
                continue
            check(d, f"'{ent.name}' forwards to it")
            if isinstance(d, Server) and id(d) not in node_of:
                # (the reference hands a clock to what `entities` lists: an unlisted Server would fail on its first event)
                raise UnsupportedTopology(f"'{ent.name}' forwards to server '{d.name}', which is not listed in `entities` of this "
                                          "Simulation (not part of this Simulation)")
            add(d)
    # the AutoScalers' instance pools: the factory's results for instances 1 .. P, dormant Server nodes behind all of the Simulation's
    # own nodes (node numbers keep their meaning), targets of their LoadBalancer behind its initial backends
    n_own = len(nodes)
    n_own_servers = sum(isinstance(x, Server) for x in nodes)
    scaled: dict[int, tuple] = {}                             # id(LoadBalancer) -> (scaler, its initial backends, the pool)
    pool_of: dict[int, tuple] = {}                            # pool node -> (scaler, k)
    for sc in [x for x in nodes if isinstance(x, AutoScaler)]:
        what = f"auto scaler '{sc.name}'"
        lb = sc.load_balancer
        if not isinstance(lb, LoadBalancer) or id(lb) not in node_of:
            raise UnsupportedTopology(f"{what}: its LoadBalancer is not an entity of this Simulation")
        if id(lb) in scaled:
            raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the scaler '{scaled[id(lb)][0].name}' already (one AutoScaler "
                                      "per LoadBalancer is lowered)")
        if isinstance(lb.strategy, (ConsistentHash, IPHash, Random)):
            raise UnsupportedTopology(f"{what}: strategy {type(lb.strategy).__name__} of '{lb.name}' is not lowered under an AutoScaler (its "
                                      "selection over a changing backend list is a follow-up: RoundRobin, WeightedRoundRobin, "
                                      "LeastConnections and WeightedLeastConnections are)")
        pol = sc.policy
        if type(pol) not in SCALING_POLICIES:
            raise UnsupportedTopology(f"{what}: policy {type(pol).__name__} is not lowered to the engine (lowered: TargetUtilization, "
                                      "StepScaling, QueueDepthScaling)")
        if isinstance(pol, StepScaling) and len(pol._steps) > AutoScaler.MAX_STEPS:
            raise UnsupportedTopology(f"{what}: StepScaling with {len(pol._steps)} steps is beyond the {AutoScaler.MAX_STEPS} the engine "
                                      "holds (AutoScaler.MAX_STEPS)")
        if lb.unhealthy_backends:
            raise UnsupportedTopology(f"{what}: backend '{lb.unhealthy_backends[0].name}' of '{lb.name}' is marked unhealthy -- health marks "
                                      "under an AutoScaler are not lowered (a follow-up)")
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
        if end_ns is None:
            raise UnsupportedTopology(f"{what}: end_time = Infinity leaves no horizon to size its instance pool by; pass end_time/duration")
        initial = lb.all_backends
        size = scaler_pool_size(sc, len(initial), start_ns, end_ns, scaler_starts)
        if size > AutoScaler.MAX_POOL:
            raise UnsupportedTopology(f"{what}: the run could create up to {size} instances, beyond the pool of {AutoScaler.MAX_POOL} "
                                      "per scaler (AutoScaler.MAX_POOL): a longer interval or cooldown, or a shorter run")
        pool = []
        for k in range(1, size + 1):
            inst = sc._instance(k)
            if not isinstance(inst, Server):
                raise UnsupportedTopology(f"{what}: server_factory returned a {type(inst).__name__} for instance {k}: only Servers may stand "
                                          "as a LoadBalancer's backends")
            if id(inst) in node_of:
                raise UnsupportedTopology(f"{what}: server_factory returned '{inst.name}' for instance {k}, which is an entity of this "
                                          "Simulation or another instance already (one new Server per call)")
            d = inst.downstream
            if d is not None and (id(d) not in node_of or node_of[id(d)] >= n_own):
                raise UnsupportedTopology(f"{what}: the downstream '{getattr(d, 'name', d)}' of instance {k} is not an entity of this "
                                          "Simulation")
            pool_of[add(inst)] = (sc, k)
            pool.append(inst)
        scaled[id(lb)] = (sc, initial, pool)
    # the RollingDeployers' pools likewise, behind the scalers'
    for dp in [x for x in nodes if isinstance(x, (RollingDeployer, CanaryDeployer))]:
        rolling = isinstance(dp, RollingDeployer)
        what = f"{'rolling' if rolling else 'canary'} deployer '{dp.name}'"
        lb = dp.load_balancer
        if not isinstance(lb, LoadBalancer) or id(lb) not in node_of:
            raise UnsupportedTopology(f"{what}: its LoadBalancer is not an entity of this Simulation")
        if id(lb) in scaled:
            other = scaled[id(lb)][0]
            raise UnsupportedTopology(f"{what}: LoadBalancer '{lb.name}' has the {type(other).__name__} '{other.name}' already (a deployer next "
                                      "to an AutoScaler or another deployer on one LoadBalancer is not lowered: a follow-up)")
        if not isinstance(lb.strategy, (RoundRobin, WeightedRoundRobin, LeastConnections, WeightedLeastConnections)):
            raise UnsupportedTopology(f"{what}: strategy {type(lb.strategy).__name__} of '{lb.name}' is not lowered under a deployer (its "
                                      "selection over a changing backend list is a follow-up: RoundRobin, WeightedRoundRobin, "
                                      "LeastConnections and WeightedLeastConnections are)")
        if lb.unhealthy_backends:
            raise UnsupportedTopology(f"{what}: backend '{lb.unhealthy_backends[0].name}' of '{lb.name}' is marked unhealthy -- health marks "
                                      "under a deployer are not lowered (a follow-up)")
        if not rolling:
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
            if (deploys or {}).get(id(dp), 1) > 1:
                raise UnsupportedTopology(f"{what}: {(deploys or {}).get(id(dp), 1)} deploy() Events are scheduled -- a second canary of the same name is never "
                                          "registered by the LoadBalancer (one deploy() per CanaryDeployer is lowered)")
        for v, nm, least in ((dp._batch_size, "batch_size", 1), (dp._healthy_threshold, "healthy_threshold", 1), (dp._max_failures, "max_failures", None)) if rolling else ():
            if type(v) is not int or not -(1 << 30) < v < (1 << 30) or (least is not None and v < least):
                raise UnsupportedTopology(f"{what}: {nm} must be an int{'' if least is None else f' of at least {least}'} below 2^30, got {v!r}")
        try:
            ok = not rolling or (bool(np.isfinite(dp._health_check_interval)) and dp._health_check_interval > 0 and dp._health_check_interval * 1e9 >= 1.0)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise UnsupportedTopology(f"{what}: health_check_interval = {dp._health_check_interval!r} must be a finite number of at least "
                                      "one nanosecond")
        initial = lb.all_backends
        n_deploys = (deploys or {}).get(id(dp), 1)
        size = deployer_pool_size(len(initial), n_deploys) if rolling else 1
        if size > RollingDeployer.MAX_POOL:
            raise UnsupportedTopology(f"{what}: {n_deploys} deploy() Events over {len(initial)} backends could create up to {size} instances, "
                                      f"beyond the pool of {RollingDeployer.MAX_POOL} per deployer (RollingDeployer.MAX_POOL)")
        pool = []
        for k in range(1, size + 1):
            inst = dp._instance(k)
            if not isinstance(inst, Server):
                raise UnsupportedTopology(f"{what}: server_factory returned a {type(inst).__name__} for instance {k}: only Servers may stand "
                                          "as a LoadBalancer's backends")
            if id(inst) in node_of:
                raise UnsupportedTopology(f"{what}: server_factory returned '{inst.name}' for instance {k}, which is an entity of this "
                                          "Simulation or another instance already (one new Server per call)")
            d = inst.downstream
            if d is not None and (id(d) not in node_of or node_of[id(d)] >= n_own):
                raise UnsupportedTopology(f"{what}: the downstream '{getattr(d, 'name', d)}' of instance {k} is not an entity of this "
                                          "Simulation")
            pool_of[add(inst)] = (dp, k)
            pool.append(inst)
        scaled[id(lb)] = (dp, initial, pool)
    n = len(nodes)
    a = GraphArrays(n)
    counters = {Server: 0, NetworkLink: 0, RandomRouter: 0}
    rt: list[int] = []
    weights: dict[int, list[int]] = {}                        # rt offset -> the weights of a weighted strategy's backends
    policies_seen: dict[int, str] = {}                        # id(policy) -> the limiter that holds it
    checked: dict[int, str] = {}                              # id(LoadBalancer) -> its HealthChecker
    unhealthy: dict[int, list[int]] = {}                      # rt offset -> is_healthy of a LoadBalancer's backends, one of them unhealthy
    client_delays: list = []                                  # per node: a Client's delay table in ns
    for i, ent in enumerate(nodes):
        if isinstance(ent, Source):
            ep, prov = ent._event_provider, ent._time_provider
            if not isinstance(ep, (SimpleEventProvider, ClientKeyEventProvider)):
                raise UnsupportedTopology(f"source '{ent.name}': event provider {type(ep).__name__} is not lowered on a general graph")
            tgt = ep._target
            n_clients = getattr(ep, "_n_clients", 0)
            if isinstance(tgt, LoadBalancer) and isinstance(tgt.strategy, Random):
                n_clients = len(tgt.all_backends)             # the Request's draw IS the choice: backends[int(u * len)] (entities.Random)
            if n_clients:
                if a.src_n_clients is None:
                    a.src_n_clients = np.zeros(n, np.int64)
                a.src_n_clients[i] = n_clients
            if not (ent.rate > 0):
                raise UnsupportedTopology(f"source '{ent.name}': rate must be > 0")
            if not isinstance(ep._target, Entity) or id(ep._target) not in node_of:
                raise UnsupportedTopology(f"source '{ent.name}' has no lowered target")
            a.kind[i] = N.NODE_SOURCE
            a.target[i] = node_of[id(ep._target)]
            a.stream_base[i] = i                              # (Sources are nodes 0 .. n_src - 1, in `sources` order)
            a.src_kind[i] = N.SRC_POISSON if prov.kind == "poisson" else N.SRC_CONSTANT
            a.src_rate[i] = float(prov.profile.peak_rate)
            a.src_stop_after_ns[i] = -1 if ep._stop_after is None else ep._stop_after.nanoseconds
            pr = prov.profile
            if not isinstance(pr, ConstantRateProfile):        # its ticks come from the tick-table kernel, like the station engines'
                if a.src_profile_kind is None:
                    a.src_profile_kind = np.zeros(n, np.uint8)
                    a.src_profile_params = np.zeros((n, 4), np.float64)
                if isinstance(pr, LinearRampProfile):
                    a.src_profile_kind[i] = N.PROF_LINEAR_RAMP
                    a.src_profile_params[i, :3] = (pr.duration_s, pr.start_rate, pr.end_rate)
                else:
                    a.src_profile_kind[i] = N.PROF_SPIKE
                    a.src_profile_params[i] = (pr.baseline_rate, pr.spike_rate, pr.warmup_s, pr.spike_duration_s)
        elif isinstance(ent, Probe):
            m = Probe.engine_metric(ent.metric)
            tgt = ent.target
            on_wrapper = isinstance(tgt, (Bulkhead, TimeoutWrapper)) and m in N.PROBE_WRAPPER_METRICS
            on_client = isinstance(tgt, Client) and m in N.PROBE_CLIENT_METRICS
            on_flow = isinstance(tgt, _FLOW_METRIC_OF.get(m, ()))
            if isinstance(tgt, AutoScaler) and m in N.PROBE_SCALER_METRICS:
                if a.probe_metric is None:
                    a.probe_metric = np.full(n, N.PROBE_NONE, np.uint8)
                    a.probe_interval_s = np.ones(n, np.float64)
                if id(tgt) not in node_of:
                    raise UnsupportedTopology(f"probe '{ent.name}': its target is not an entity of this Simulation")
                a.kind[i] = N.NODE_PROBE
                a.target[i] = node_of[id(tgt)]
                a.probe_metric[i] = N.PROBE_SCALER_METRICS[m]
                a.probe_interval_s[i] = ent.interval
                continue
            if on_flow:
                if a.probe_metric is None:
                    a.probe_metric = np.full(n, N.PROBE_NONE, np.uint8)
                    a.probe_interval_s = np.ones(n, np.float64)
                if id(tgt) not in node_of:
                    raise UnsupportedTopology(f"probe '{ent.name}': its target is not an entity of this Simulation")
                a.kind[i] = N.NODE_PROBE
                a.target[i] = node_of[id(tgt)]
                a.probe_metric[i] = N.PROBE_FLOW_METRICS[m]
                a.probe_interval_s[i] = ent.interval
                continue
            if m not in N.PROBE_METRICS and not on_wrapper and not on_client:
                raise UnsupportedTopology(f"probe '{ent.name}': metric '{ent.metric}' is not sampled on the engine")
            if id(tgt) not in node_of:
                raise UnsupportedTopology(f"probe '{ent.name}': its target is not an entity of this Simulation")
            want = Client if on_client else (TimeoutWrapper if m == "in_flight_count" else Bulkhead) if on_wrapper else Source if m == "generated_count" else _SINKS if m == "events_received" else RateLimitedEntity if m == "queue_depth" else Server
            if not isinstance(tgt, want):
                raise UnsupportedTopology(f"probe '{ent.name}': metric '{ent.metric}' is not an attribute of {type(tgt).__name__}")
            if a.probe_metric is None:
                a.probe_metric = np.full(n, N.PROBE_NONE, np.uint8)
                a.probe_interval_s = np.ones(n, np.float64)
            a.kind[i] = N.NODE_PROBE
            a.target[i] = node_of[id(tgt)]
            a.probe_metric[i] = N.PROBE_CLIENT_METRICS[m] if on_client else N.PROBE_WRAPPER_METRICS[m] if on_wrapper else N.PROBE_METRICS[m]
            a.probe_interval_s[i] = ent.interval
        elif isinstance(ent, Server):
            svc = ent.service_time
            if not isinstance(svc, (ExponentialLatency, ConstantLatency)):
                raise UnsupportedTopology(f"server '{ent.name}': service distribution {type(svc).__name__} is not lowered")
            a.kind[i] = N.NODE_SERVER
            if i in pool_of:
                a.stream_base[i] = n_own_servers + pool_of[i][1] - 1        # instance k: the Servers' numbering goes on
            else:
                a.stream_base[i] = counters[Server]
                counters[Server] += 1
            a.concurrency[i] = ent.concurrency
            a.lat_kind[i] = N.LAT_EXPONENTIAL if isinstance(svc, ExponentialLatency) else N.LAT_CONSTANT
            a.lat_mean_s[i] = svc.mean
            cap = ent._policy.capacity
            a.queue_cap[i] = -1 if cap == float("inf") else int(cap)
            pol = ent._policy
            if isinstance(pol, QUEUE_POLICIES):
                if a.qp_params is None:
                    a.qp_params = np.zeros((n, 5), np.float64)
                if len(pol):
                    raise UnsupportedTopology(f"server '{ent.name}': {len(pol)} items are still queued in its {type(pol).__name__} from an "
                                              "earlier run (not lowered)")
                if cap != float("inf") and not (type(cap) is int and 0 <= cap < (1 << 31)):
                    raise UnsupportedTopology(f"server '{ent.name}': the capacity {cap!r} of its {type(pol).__name__} is not an int below 2^31")
                if isinstance(pol, AdaptiveLIFO):
                    if type(pol.congestion_threshold) is not int:
                        raise UnsupportedTopology(f"server '{ent.name}': congestion_threshold must be an int, got {pol.congestion_threshold!r}")
                    a.qp_params[i] = (N.QUEUE_ADAPTIVE_LIFO, a.queue_cap[i], min(pol.congestion_threshold, 1 << 40), 0.0, 0.0)
                elif isinstance(pol, CoDelQueue):
                    target, interval = float(pol.target_delay), float(pol.interval)
                    if not (target < float("inf") and interval <= 4.0e9):
                        raise UnsupportedTopology(f"server '{ent.name}': CoDelQueue(target_delay={target!r}, interval={interval!r}) is beyond "
                                                  "4e9 s or not finite")
                    a.qp_params[i] = (N.QUEUE_CODEL, a.queue_cap[i], 0, target, interval)
                else:
                    a.qp_params[i] = (N.QUEUE_LIFO, a.queue_cap[i], 0, 0.0, 0.0)
            elif not isinstance(pol, FIFOQueue):
                raise UnsupportedTopology(f"server '{ent.name}': queue policy {type(pol).__name__} is not lowered")
            d = ent.downstream
            a.target[i] = -1 if d is None else node_of[id(d)]
        elif isinstance(ent, NetworkLink):
            if not isinstance(ent.latency, ConstantLatency) or not (ent.latency.mean >= 0):
                raise UnsupportedTopology(f"link '{ent.name}': the base latency must be a ConstantLatency >= 0")
            if ent.jitter is not None and not isinstance(ent.jitter, (ExponentialLatency, ConstantLatency)):
                raise UnsupportedTopology(f"link '{ent.name}': jitter {type(ent.jitter).__name__} is not lowered")
            a.kind[i] = N.NODE_LINK
            a.stream_base[i] = counters[NetworkLink]
            counters[NetworkLink] += 1
            a.link_lat_min_s[i] = ent.latency.mean
            if ent.jitter is not None:
                a.lat_kind[i] = N.LAT_EXPONENTIAL if isinstance(ent.jitter, ExponentialLatency) else N.LAT_CONSTANT
                a.lat_mean_s[i] = ent.jitter.mean
            a.link_loss_rate[i] = ent.packet_loss_rate
            a.target[i] = -1 if ent.egress is None else node_of[id(ent.egress)]
        elif isinstance(ent, LoadBalancer):
            backends = ent.all_backends
            if id(ent) in scaled:
                backends = scaled[id(ent)][1] + scaled[id(ent)][2]       # the candidate list: the initial backends, then the pool
            for b in backends:
                if not isinstance(b, Server):
                    raise UnsupportedTopology(f"backend '{b.name}' of '{ent.name}' is a {type(b).__name__}: only Server backends are lowered")
            if a.lb_strategy is None:
                a.lb_strategy = np.full(n, N.LB_ROUND_ROBIN, np.uint8)
                a.lb_vnodes = np.zeros(n, np.int32)
            st = ent.strategy
            a.kind[i] = N.NODE_LB
            code = next((c for cls, c in _STRATEGY_CODE if isinstance(st, cls)), None)
            if code is None:
                raise UnsupportedTopology(f"strategy {type(st).__name__} of '{ent.name}' is not lowered to the engine")
            a.lb_strategy[i] = code
            a.lb_vnodes[i] = getattr(st, "virtual_nodes", 0)
            a.rt_off[i] = len(rt)
            a.rt_cnt[i] = len(backends)
            if isinstance(st, (WeightedRoundRobin, WeightedLeastConnections)):
                n_init = len(ent.all_backends)                         # (an instance joins at weight 1: add_backend's default)
                ws = [int(st.get_weight(b)) if q < n_init else 1 for q, b in enumerate(backends)]
                if isinstance(st, WeightedRoundRobin) and sum(ws) > WeightedRoundRobin.MAX_TOTAL_WEIGHT:
                    raise UnsupportedTopology(f"'{ent.name}': WeightedRoundRobin with a total weight of {sum(ws)} needs a selection table "
                                              "beyond 2^24 entries (not lowered)")
                weights[len(rt)] = ws
            flags = [int(ent.get_backend_info(b).is_healthy) if ent.get_backend_info(b) is not None else 1 for b in backends]
            if not all(flags):
                if isinstance(st, (ConsistentHash, IPHash, Random)):
                    raise UnsupportedTopology(f"'{ent.name}': strategy {type(st).__name__} with an unhealthy backend ('"
                                              f"{ent.unhealthy_backends[0].name}') is not lowered (its selection over a changing backend list "
                                              "is a follow-up)")
                unhealthy[len(rt)] = flags
            rt.extend(node_of[id(b)] for b in backends)
        elif isinstance(ent, HealthChecker):
            lb = ent.load_balancer
            if not isinstance(lb, LoadBalancer) or id(lb) not in node_of:
                raise UnsupportedTopology(f"health checker '{ent.name}': its LoadBalancer is not an entity of this Simulation")
            if id(lb) in scaled:
                kind_ = type(scaled[id(lb)][0]).__name__
                raise UnsupportedTopology(f"health checker '{ent.name}': LoadBalancer '{lb.name}' has the {kind_} '{scaled[id(lb)][0].name}' "
                                          f"-- a HealthChecker and {'an' if kind_ == 'AutoScaler' else 'a'} {kind_} on one LoadBalancer are not lowered (a follow-up)")
            if id(lb) in checked:
                raise UnsupportedTopology(f"health checker '{ent.name}': LoadBalancer '{lb.name}' has the checker '{checked[id(lb)]}' already "
                                          "(one HealthChecker per LoadBalancer is lowered)")
            checked[id(lb)] = ent.name
            if isinstance(lb.strategy, (ConsistentHash, IPHash, Random)):
                raise UnsupportedTopology(f"health checker '{ent.name}': strategy {type(lb.strategy).__name__} of '{lb.name}' is not lowered "
                                          "under a HealthChecker (its selection over a changing backend list is a follow-up: RoundRobin, "
                                          "WeightedRoundRobin, LeastConnections and WeightedLeastConnections are)")
            if not (ent.interval * 1e9 >= 1.0):
                raise UnsupportedTopology(f"health checker '{ent.name}': an interval of {ent.interval} s is below one nanosecond")
            if a.hc_params is None:
                a.hc_params = np.zeros((n, 5), np.float64)
            a.kind[i] = N.NODE_HEALTH_CHECKER
            a.target[i] = node_of[id(lb)]
            a.hc_params[i] = (ent.interval, ent.timeout, ent.healthy_threshold, ent.unhealthy_threshold, 1.0 if ent.is_running else 0.0)
        elif isinstance(ent, AutoScaler):
            lb, pol = ent.load_balancer, ent.policy
            if id(lb) in checked:
                raise UnsupportedTopology(f"auto scaler '{ent.name}': LoadBalancer '{lb.name}' has the HealthChecker '{checked[id(lb)]}' -- a "
                                          "HealthChecker and an AutoScaler on one LoadBalancer are not lowered (a follow-up)")
            if a.as_params is None:
                a.as_params = np.zeros((n, 10), np.float64)
                a.as_steps = [None] * n
            a.kind[i] = N.NODE_AUTO_SCALER
            a.target[i] = node_of[id(lb)]
            if isinstance(pol, TargetUtilization):
                code, p0, p1 = N.AUTOSCALER_TARGET_UTILIZATION, pol._target, 0.0
            elif isinstance(pol, StepScaling):
                code, p0, p1 = N.AUTOSCALER_STEP, 0.0, 0.0
                try:
                    a.as_steps[i] = [(float(t), int(d)) for t, d in pol._steps]
                except (TypeError, ValueError):
                    raise UnsupportedTopology(f"auto scaler '{ent.name}': StepScaling steps must be (number, int) pairs") from None
            else:
                code, p0, p1 = N.AUTOSCALER_QUEUE_DEPTH, pol._scale_out_threshold, pol._scale_in_threshold
            a.as_params[i] = (code, p0, p1, ent._min_instances, ent._max_instances, ent._evaluation_interval, ent._scale_out_cooldown,
                              ent._scale_in_cooldown, len(scaled[id(lb)][2]), 1.0 if ent.is_running else 0.0)
        elif isinstance(ent, CanaryDeployer):
            lb, ev = ent.load_balancer, ent._metric_evaluator
            if id(lb) in checked:
                raise UnsupportedTopology(f"canary deployer '{ent.name}': LoadBalancer '{lb.name}' has the HealthChecker '{checked[id(lb)]}' -- a "
                                          "HealthChecker and a CanaryDeployer on one LoadBalancer are not lowered (a follow-up)")
            if a.cn_params is None:
                a.cn_params = [None] * n
            a.kind[i] = N.NODE_CANARY_DEPLOYER
            a.target[i] = node_of[id(lb)]
            latency = isinstance(ev, LatencyEvaluator)
            a.cn_params[i] = ([(float(s_.traffic_percentage), float(s_.evaluation_period)) for s_ in ent._stages],
                              N.CANARY_LATENCY if latency else N.CANARY_ERROR_RATE, float(ev._max_latency if latency else ev._max_error_rate),
                              float(ev._threshold_multiplier), float(ent._evaluation_interval))
        elif isinstance(ent, RollingDeployer):
            lb = ent.load_balancer
            if id(lb) in checked:
                raise UnsupportedTopology(f"rolling deployer '{ent.name}': LoadBalancer '{lb.name}' has the HealthChecker '{checked[id(lb)]}' -- a "
                                          "HealthChecker and a RollingDeployer on one LoadBalancer are not lowered (a follow-up)")
            if a.rd_params is None:
                a.rd_params = np.zeros((n, 5), np.float64)
            a.kind[i] = N.NODE_ROLLING_DEPLOYER
            a.target[i] = node_of[id(lb)]
            a.rd_params[i] = (ent._batch_size, ent._health_check_interval, ent._healthy_threshold, ent._max_failures, len(scaled[id(lb)][2]))
        elif isinstance(ent, (Bulkhead, TimeoutWrapper)):
            what = f"{type(ent).__name__} '{ent.name}'"
            tgt = ent.target
            if isinstance(tgt, (Source, Probe, HealthChecker)) or not isinstance(tgt, Entity) or id(tgt) not in node_of:
                raise UnsupportedTopology(f"{what}: its target {type(tgt).__name__} '{getattr(tgt, 'name', tgt)}' takes no Requests")
            end, hops = tgt, 0
            while isinstance(end, NetworkLink) and end.egress is not None and hops <= n:
                end, hops = end.egress, hops + 1
            if isinstance(end, _FLOWS):
                raise UnsupportedTopology(_flow_target_refusal(what, end, tgt))
            if isinstance(end, Client):
                via = " (through its NetworkLinks)" if end is not tgt else ""
                raise UnsupportedTopology(f"{what}: its target{via} is the Client '{end.name}' -- two completion hooks on one Event are not "
                                          "lowered (a follow-up)")
            if isinstance(end, (LoadBalancer, Bulkhead, TimeoutWrapper)):
                via = " (through its NetworkLinks)" if end is not tgt else ""
                raise UnsupportedTopology(f"{what}: its target{via} is the {type(end).__name__} '{end.name}' -- two completion hooks on one "
                                          "Event are not lowered (a follow-up)")
            if a.wrap_params is None:
                a.wrap_params = np.zeros((n, 5), np.float64)
            a.target[i] = node_of[id(tgt)]
            if isinstance(ent, Bulkhead):
                if ent.max_concurrent > Bulkhead.MAX_CONCURRENT:
                    raise UnsupportedTopology(f"{what}: max_concurrent = {ent.max_concurrent} is beyond the {Bulkhead.MAX_CONCURRENT} request "
                                              "ids the engine's in-flight table holds")
                if ent.max_wait_queue > (1 << 30):
                    raise UnsupportedTopology(f"{what}: max_wait_queue = {ent.max_wait_queue} is beyond 2^30")
                if ent.max_wait_time is not None and not np.isfinite(ent.max_wait_time):
                    raise UnsupportedTopology(f"{what}: max_wait_time must be finite or None")
                a.kind[i] = N.NODE_BULKHEAD
                a.wrap_params[i, :3] = (ent.max_concurrent, ent.max_wait_queue, -1.0 if ent.max_wait_time is None else ent.max_wait_time)
            else:
                if ent._on_timeout is not None:
                    raise UnsupportedTopology(f"{what}: on_timeout= is a host callable (not lowered)")
                if not np.isfinite(ent.timeout):
                    raise UnsupportedTopology(f"{what}: timeout must be finite")
                a.kind[i] = N.NODE_TIMEOUT_WRAPPER
                a.wrap_params[i, 3] = ent.timeout
        elif isinstance(ent, Client):
            what = f"Client '{ent.name}'"
            tgt = ent.target
            if isinstance(tgt, (Source, Probe, HealthChecker)) or not isinstance(tgt, Entity) or id(tgt) not in node_of:
                raise UnsupportedTopology(f"{what}: its target {type(tgt).__name__} '{getattr(tgt, 'name', tgt)}' takes no Requests")
            end, hops = tgt, 0
            while isinstance(end, NetworkLink) and end.egress is not None and hops <= n:
                end, hops = end.egress, hops + 1
            if isinstance(end, _FLOWS):
                raise UnsupportedTopology(_flow_target_refusal(what, end, tgt))
            if isinstance(end, (LoadBalancer, Bulkhead, TimeoutWrapper, Client)):
                via = " (through its NetworkLinks)" if end is not tgt else ""
                raise UnsupportedTopology(f"{what}: its target{via} is the {type(end).__name__} '{end.name}' -- two completion hooks on one "
                                          "Event are not lowered (a follow-up)")
            if ent._on_success is not None or ent._on_failure is not None:
                raise UnsupportedTopology(f"{what}: on_success= / on_failure= are host callables (not lowered)")
            if ent.timeout is not None and not np.isfinite(ent.timeout):
                raise UnsupportedTopology(f"{what}: timeout must be finite or None")
            delays = client_delay_table(ent.retry_policy, what)
            if a.cl_params is None:
                a.cl_params = np.zeros((n, 2), np.float64)
                client_delays = [np.zeros(0, np.int64) for _ in range(n)]
            a.kind[i] = N.NODE_CLIENT
            a.target[i] = node_of[id(tgt)]
            a.cl_params[i, 0] = -1.0 if ent.timeout is None else float(ent.timeout)
            client_delays[i] = delays
        elif isinstance(ent, _FLOWS):
            what = f"{type(ent).__name__} '{ent.name}'"
            d = ent.downstream
            if isinstance(d, (Source, Probe, HealthChecker)) or not isinstance(d, Entity) or id(d) not in node_of:
                raise UnsupportedTopology(f"{what}: its downstream {type(d).__name__} '{getattr(d, 'name', d)}' takes no Requests")
            if a.flow_params is None:
                a.flow_params = np.zeros((n, 4), np.int64)
            a.target[i] = node_of[id(d)]
            if isinstance(ent, BatchProcessor):
                if type(ent.batch_size) is not int:
                    raise UnsupportedTopology(f"{what}: batch_size must be an int, got {ent.batch_size!r}")
                if ent.batch_size > BatchProcessor.MAX_BATCH_SIZE:
                    raise UnsupportedTopology(f"{what}: batch_size = {ent.batch_size} is beyond the {BatchProcessor.MAX_BATCH_SIZE} items of "
                                              "one batch on the engine (BatchProcessor.MAX_BATCH_SIZE)")
                a.kind[i] = N.NODE_BATCH_PROCESSOR
                # the generator's `yield process_time` is float(process_time) added to an Instant, `now + timeout_s` the number itself
                a.flow_params[i] = (ent.batch_size, flow_delay_ns(float(ent.process_time), what, "process_time"),
                                    flow_delay_ns(ent.timeout_s, what, "timeout_s") if ent.timeout_s > 0 else 0, 0)
            elif isinstance(ent, ConveyorBelt):
                a.kind[i] = N.NODE_CONVEYOR
                cap = ent._capacity
                a.flow_params[i] = (0 if not cap > 0 else min(int(cap), (1 << 31) - 1), flow_delay_ns(float(ent.transit_time), what, "transit_time"), 0, 0)
            else:
                cap = ent._queue_capacity
                if cap > GateController.MAX_QUEUE_CAPACITY:
                    raise UnsupportedTopology(f"{what}: queue_capacity = {cap} is beyond the {GateController.MAX_QUEUE_CAPACITY} items of a "
                                              "bounded queue on the engine (GateController.MAX_QUEUE_CAPACITY; 0 is unbounded)")
                if ent._queue_depth:
                    raise UnsupportedTopology(f"{what}: {ent._queue_depth} items are still queued from an earlier run (not lowered)")
                a.kind[i] = N.NODE_GATE
                a.flow_params[i] = (max(int(cap), 0), 0, int(ent._open_cycles), 1 if ent._is_open else 0)
        elif isinstance(ent, RateLimitedEntity):
            pol = ent.policy
            if type(pol) not in LIMITER_POLICIES:
                raise UnsupportedTopology(f"limiter '{ent.name}': policy {type(pol).__name__} is not lowered to the engine (lowered: "
                                          "TokenBucketPolicy, LeakyBucketPolicy, SlidingWindowPolicy, FixedWindowPolicy)")
            if id(pol) in policies_seen:
                raise UnsupportedTopology(f"limiter '{ent.name}' shares its policy object with '{policies_seen[id(pol)]}': one policy per "
                                          "limiter is lowered")
            policies_seen[id(pol)] = ent.name
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
            if a.lim_policy is None:
                a.lim_policy = np.full(n, N.LIMITER_NONE, np.uint8)
                a.lim_params = np.zeros((n, 3), np.float64)
                a.lim_count = np.zeros(n, np.int64)
            a.kind[i] = N.NODE_RATE_LIMITER
            a.target[i] = node_of[id(ent.downstream)]
            a.queue_cap[i] = -1 if cap == float("inf") else int(cap)
            a.lim_policy[i], a.lim_params[i], a.lim_count[i] = kind, (p0, p1, p2), count
        elif isinstance(ent, RandomRouter):
            if not ent.targets:
                raise UnsupportedTopology(f"router '{ent.name}' has no targets")
            a.kind[i] = N.NODE_ROUTER
            a.stream_base[i] = counters[RandomRouter]
            counters[RandomRouter] += 1
            a.rt_off[i] = len(rt)
            a.rt_cnt[i] = len(ent.targets)
            rt.extend(node_of[id(t)] for t in ent.targets)
        else:
            a.kind[i] = N.NODE_SINK                           # (a Network too: a node that no Event reaches)
    a.rt_targets = np.array(rt, np.int32)
    if a.cl_params is not None:
        a.cl_delay_off = np.zeros(n + 1, np.int64)
        a.cl_delay_off[1:] = np.cumsum([len(d) for d in client_delays])
        a.cl_delays_ns = np.concatenate(client_delays).astype(np.int64)
    if weights:
        a.lb_weights = np.ones(len(rt), np.int32)
        for off, ws in weights.items():
            a.lb_weights[off:off + len(ws)] = ws
    if unhealthy or a.hc_params is not None or a.as_params is not None or a.rd_params is not None or a.cn_params is not None:     # (a scaled LoadBalancer's member list is the healthy list)
        a.lb_healthy = np.ones(len(rt), np.uint8)
        for off, flags in unhealthy.items():
            a.lb_healthy[off:off + len(flags)] = flags
    if a.lb_strategy is not None:
        _check_keys(nodes, node_of, a)
        blobs = [(x.name.encode() if isinstance(x, Server) else b"") for x in nodes]     # (only an LB's backends need their name)
        a.names = b"".join(blobs)
        a.name_off = np.zeros(n + 1, np.int32)
        a.name_off[1:] = np.cumsum([len(b) for b in blobs])
    assert all(a.kind[i] == N.NODE_SOURCE for i in range(n_src)) and all(a.kind[i] == N.NODE_PROBE for i in range(n_src, n_front))
    g = GeneralGraph(nodes, a, node_of)
    g.n_own, g.scaler_starts = n_own, scaler_starts
    g.scaled = {node_of[lb_id]: (node_of[id(sc)], initial, pool) for lb_id, (sc, initial, pool) in scaled.items() if isinstance(sc, AutoScaler)}
    g.pool_of = {i: (node_of[id(sc)], k) for i, (sc, k) in pool_of.items() if isinstance(sc, AutoScaler)}
    both = (RollingDeployer, CanaryDeployer)
    g.deployed = {node_of[lb_id]: (node_of[id(dp)], initial, pool) for lb_id, (dp, initial, pool) in scaled.items() if isinstance(dp, both)}
    g.dpool_of = {i: (node_of[id(dp)], k) for i, (dp, k) in pool_of.items() if isinstance(dp, both)}
    g.deploys = {node_of[id(dp)]: (deploys or {}).get(id(dp), 1) for dp, _i, _p in scaled.values() if isinstance(dp, both)}
    g.rr_base = {i: nodes[i].strategy._index for i in list(g.scaled) + list(g.deployed) if isinstance(nodes[i].strategy, RoundRobin)}
    return g


MAX_PARTS = 2048          # heaps one Simulation is spread over (hs_graph_run_parts): components beyond that share heaps


def split_parts(a: GraphArrays, max_parts: int = MAX_PARTS):
    """The graph's parts no Request can cross -- its connected components, packed into at most `max_parts` groups of neighbouring
    components -- as [(node ids ascending, rt positions, GraphArrays of the part)], or None when the graph is one component.
    Node order inside a part is the Simulation's (Sources first, then Probes: hs_graph_nodes' contract)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    n = a.n
    rt = np.asarray(a.rt_targets, np.int64)
    has_t = np.nonzero(a.target >= 0)[0]
    rt_owner = np.repeat(np.arange(n, dtype=np.int64), a.rt_cnt.astype(np.int64))
    if len(rt_owner) != len(rt):                       # (rt_off / rt_cnt do not tile rt_targets: leave it to the one heap)
        return None
    src = np.concatenate([has_t, rt_owner])
    dst = np.concatenate([a.target[has_t].astype(np.int64), rt])
    n_comp, label = connected_components(coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n)), directed=False)
    if n_comp < 2:
        return None
    # components in the order of their first node; neighbours share a heap when there are more components than heaps
    first = np.full(n_comp, n, np.int64)
    np.minimum.at(first, label, np.arange(n))
    rank = np.empty(n_comp, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(n_comp)
    k = min(n_comp, max_parts)
    part_of_node = rank[label] * k // n_comp
    order = np.argsort(part_of_node, kind="stable")                    # node ids grouped by part, ascending inside a part
    bounds = np.searchsorted(part_of_node[order], np.arange(k + 1))
    rt_off = np.asarray(a.rt_off, np.int64)
    new_index = np.empty(n, np.int64)
    per_node = [nm for nm in ("kind", "stream_base", "src_kind", "src_rate", "src_stop_after_ns", "concurrency", "lat_kind", "lat_mean_s",
                              "link_lat_min_s", "link_loss_rate", "queue_cap", "src_profile_kind", "src_profile_params", "probe_metric",
                              "probe_interval_s", "lb_strategy", "lb_vnodes", "src_n_clients", "lim_policy", "lim_params", "lim_count", "hc_params", "wrap_params", "cl_params",
                              "flow_params", "qp_params", "as_params", "rd_params")
                if getattr(a, nm) is not None]
    names = None if a.names is None else [a.names[a.name_off[i]:a.name_off[i + 1]] for i in range(n)]
    parts = []
    for p in range(k):
        ids = order[bounds[p]:bounds[p + 1]]
        m = len(ids)
        new_index[ids] = np.arange(m)
        b = GraphArrays(m)
        for nm in per_node:
            setattr(b, nm, np.ascontiguousarray(getattr(a, nm)[ids]))
        t = a.target[ids].astype(np.int64)
        b.target = np.where(t >= 0, new_index[np.maximum(t, 0)], -1).astype(np.int32)
        cnt = a.rt_cnt[ids].astype(np.int64)
        b.rt_cnt = cnt.astype(np.int32)
        b.rt_off = (np.cumsum(cnt) - cnt).astype(np.int32)
        total = int(cnt.sum())
        if total:
            pos = np.repeat(rt_off[ids] - (np.cumsum(cnt) - cnt), cnt) + np.arange(total)
            b.rt_targets = new_index[rt[pos]].astype(np.int32)
            if a.lb_weights is not None:
                b.lb_weights = np.ascontiguousarray(a.lb_weights[pos])
            if a.lb_healthy is not None:
                b.lb_healthy = np.ascontiguousarray(a.lb_healthy[pos])
        else:
            pos = np.zeros(0, np.int64)
            b.rt_targets = np.zeros(0, np.int32)
        if b.hc_params is not None and not (b.kind == N.NODE_HEALTH_CHECKER).any():
            b.hc_params = None                                             # (a part without a checker: no health state unless a flag says so)
        if b.rd_params is not None and not (b.kind == N.NODE_ROLLING_DEPLOYER).any():
            b.rd_params = None                                             # (a part without a deployer likewise)
        if a.cn_params is not None and (b.kind == N.NODE_CANARY_DEPLOYER).any():
            b.cn_params = [a.cn_params[i] for i in ids]
        if (b.lb_healthy is not None and b.hc_params is None and b.lb_healthy.all() and not (b.kind == N.NODE_AUTO_SCALER).any()
                and b.rd_params is None and b.cn_params is None):
            b.lb_healthy = None
        if b.wrap_params is not None and not ((b.kind == N.NODE_BULKHEAD) | (b.kind == N.NODE_TIMEOUT_WRAPPER)).any():
            b.wrap_params = None                                           # (a part without a wrapper runs the loop it would run alone)
        if b.flow_params is not None and not ((b.kind >= N.NODE_BATCH_PROCESSOR) & (b.kind <= N.NODE_GATE)).any():
            b.flow_params = None                                           # (a part without a flow entity likewise)
        if b.qp_params is not None and not (b.qp_params[:, 0] != N.QUEUE_FIFO).any():
            b.qp_params = None                                             # (a part without a policied Server likewise)
        if b.as_params is not None:
            if (b.kind == N.NODE_AUTO_SCALER).any():
                b.as_steps = [a.as_steps[i] for i in ids]
            else:
                b.as_params = None                                         # (a part without a scaler likewise)
        if b.cl_params is not None and not (b.kind == N.NODE_CLIENT).any():
            b.cl_params = None                                             # (a part without a Client likewise)
        if b.cl_params is not None:
            tables = [a.cl_delays_ns[a.cl_delay_off[i]:a.cl_delay_off[i + 1]] for i in ids]
            b.cl_delay_off = np.zeros(m + 1, np.int64)
            b.cl_delay_off[1:] = np.cumsum([len(x) for x in tables])
            b.cl_delays_ns = np.concatenate(tables).astype(np.int64)
        if names is not None:
            blobs = [names[i] for i in ids]
            b.names = b"".join(blobs)
            b.name_off = np.zeros(m + 1, np.int32)
            b.name_off[1:] = np.cumsum([len(x) for x in blobs])
        parts.append((ids, pos, b))
    return parts


class PartRun:
    """The engines of one Simulation's parts behind GraphEngine's reading interface (summary / stats / records), merged back into the
    Simulation's node numbering."""

    def __init__(self, arrays: GraphArrays, parts, engines):
        self.arrays, self.parts, self.engines = arrays, parts, engines

    def run(self, end_ns: int) -> bool:
        """hs_graph_run_parts: True when the parts' results are the Simulation's, False when the run is undecided (one heap decides)."""
        hs_ = (C.c_void_p * len(self.engines))(*[e._h for e in self.engines])
        rc = self.engines[0]._lib.hs_graph_run_parts(hs_, len(self.engines), int(end_ns))
        self.engines[0]._check(rc)
        return rc == 0

    def summary(self) -> N.Summary:
        subs = [e.summary() for e in self.engines]
        out = N.Summary()
        out.events_processed = sum(s.events_processed for s in subs)
        out.final_time_ns = max(s.final_time_ns for s in subs)           # (the one event beyond the end, or the last event of a drained run)
        for k in range(N.EV_KINDS):
            out.events_by_kind[k] = sum(s.events_by_kind[k] for s in subs)
        out.requests_completed = sum(s.requests_completed for s in subs)
        out.sink_records = sum(s.sink_records for s in subs)
        out.launches = sum(s.launches for s in subs)
        out.last_run_ms = max(s.last_run_ms for s in subs)
        out.kernel_ms = out.last_run_ms
        return out

    def stats(self) -> dict:
        n, nrt = self.arrays.n, len(self.arrays.rt_targets)
        out = {k: np.zeros(nrt if k == "rt_taken" else (n, 6) if k == "lb" else n, np.float64 if k == "total_service_s" else np.int64)
               for k in N.GRAPH_STATS}
        for (ids, pos, _b), e in zip(self.parts, self.engines):
            st = e.stats()
            for k, v in st.items():
                if k == "limiters":
                    out.setdefault(k, {}).update({int(ids[i]): x for i, x in v.items()})
                elif k == "rt_taken":
                    out[k][pos] = v
                else:
                    out[k][ids] = v
        return out

    def faults(self):
        crashed, internal, cancelled = np.zeros(self.arrays.n, np.uint8), np.zeros(4, np.int64), 0
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            c, p, k = e.faults()
            crashed[ids] = c
            internal += p
            cancelled += k
        return crashed, internal, cancelled

    def link_faults(self) -> dict:
        out = {}
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            out.update({int(ids[i]): v for i, v in e.link_faults().items()})
        return out

    def health_events(self) -> np.ndarray:
        return np.sum([e.health_events() for e in self.engines], axis=0).astype(np.int64)

    def wrapper_events(self) -> np.ndarray:
        return np.sum([e.wrapper_events() for e in self.engines], axis=0).astype(np.int64)

    def client_events(self) -> np.ndarray:
        return np.sum([e.client_events() for e in self.engines], axis=0).astype(np.int64)

    def flow_events(self) -> np.ndarray:
        return np.sum([e.flow_events() for e in self.engines], axis=0).astype(np.int64)

    def queue_policy(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.queue_policy(int(at))
        raise KeyError(node)

    def flow(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.flow(int(at))
        raise KeyError(node)

    def client(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.client(int(at))
        raise KeyError(node)

    def wrapper(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.wrapper(int(at))
        raise KeyError(node)

    def scaler_events(self) -> int:
        return int(sum(e.scaler_events() for e in self.engines))

    def deployer_events(self) -> np.ndarray:
        return np.sum([e.deployer_events() for e in self.engines], axis=0)

    def canary_events(self) -> np.ndarray:
        return np.sum([e.canary_events() for e in self.engines], axis=0)

    def canary(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.canary(int(at))
        raise KeyError(node)

    def deployer(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.deployer(int(at))
        raise KeyError(node)

    def scaler(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.scaler(int(at))
        raise KeyError(node)

    def health(self, node: int) -> dict:
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e.health(int(at))
        raise KeyError(node)

    def records(self):
        node, t, cr = [], [], []
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            nd, tt, cc = e.records()
            node.append(ids[nd].astype(np.int32))
            t.append(tt)
            cr.append(cc)
        return np.concatenate(node), np.concatenate(t), np.concatenate(cr)

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


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
    from .lowering import UnsupportedTopology

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


def keyless_hazard(g: "GeneralGraph", target) -> str | None:
    """Simulation.schedule(): a scheduled Request carries no client id -- the name of a Random LoadBalancer it could reach."""
    for j in _reaches(g.nodes, g.node_of, target):
        x = g.nodes[j]
        if isinstance(x, LoadBalancer) and isinstance(x.strategy, Random):
            return x.name
    return None


def write_back_general(g: GeneralGraph, stats: dict, rec_node: np.ndarray, rec_t: np.ndarray, rec_cr: np.ndarray, device: int = 0,
                       health=None, wrapper=None, client=None, flow=None, queue=None, scaler=None, deployer=None, canary=None) -> None:
    """The run's per-node results onto the user's objects, under the attribute names the reference uses (lowering.write_back's
    counterpart).  `health`: node -> GraphEngine.health(node) of a graph with health state; `wrapper`: node -> GraphEngine.wrapper(node)
    of a graph with a Bulkhead or a TimeoutWrapper; `client`: node -> GraphEngine.client(node) of a graph with a Client."""
    a = g.arrays
    order = np.argsort(rec_node, kind="stable")              # per Sink, still in processing order
    bounds = np.searchsorted(rec_node[order], np.arange(a.n + 1))
    scalers = {sn: scaler(sn) for sn, _initial, _pool in g.scaled.values()} if g.scaled else {}    # GraphEngine.scaler(node) per AutoScaler
    # GraphEngine.deployer(node) per RollingDeployer, GraphEngine.canary(node) per CanaryDeployer (its one instance: id 1 once it is set)
    deployers = {dn: (deployer(dn) if isinstance(g.nodes[dn], RollingDeployer) else canary(dn)) for dn, _initial, _pool in g.deployed.values()}
    for w in deployers.values():
        if "has_canary" in w:
            w.update(next_instance_id=w["has_canary"], readded=[])
    for i, ent in enumerate(g.nodes):
        if i in g.pool_of and g.pool_of[i][1] > scalers[g.pool_of[i][0]]["next_instance_id"]:
            continue                                               # (an instance the run never activated: left untouched)
        if i in g.dpool_of and g.dpool_of[i][1] > deployers[g.dpool_of[i][0]]["next_instance_id"]:
            continue
        if isinstance(ent, Source):
            ent._generated_count = int(stats["generated"][i])
            ent._event_provider._generated = int(stats["payloads"][i])
        elif isinstance(ent, Server):
            ent._queue.stats_accepted = int(stats["accepted"][i])
            ent._queue.stats_dropped = int(stats["dropped"][i])
            ent._queue.depth = int(stats["queue_depth"][i])
            ent._requests_completed = int(stats["completed"][i])
            ent._requests_rejected = int(stats["rejected"][i])
            ent._total_service_time = float(stats["total_service_s"][i])
            ent._active = int(stats["active"][i])
            pol = ent._policy
            if isinstance(pol, QUEUE_POLICIES):
                w = queue(i)                  # GraphEngine.queue_policy(node) of a graph with such a Server
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
        elif isinstance(ent, NetworkLink):
            ent.packets_sent = int(stats["packets_sent"][i])
            ent.packets_dropped = int(stats["packets_dropped"][i])
            ent._entered = int(stats["entered"][i])
            # (a graph with link faults: Simulation._general_finish puts the count of the engine's own word here)
            ent._loss_draws = ent._entered if ent.packet_loss_rate > 0 else 0
        elif isinstance(ent, Network):
            pass                                                   # (a registry: traffic_matrix() reads its links)
        elif isinstance(ent, LoadBalancer):
            (ent._requests_received, ent._requests_forwarded, ent._requests_failed, ent._no_backend_available,
             ent._in_flight_count, selections) = (int(v) for v in stats["lb"][i])
            if isinstance(ent.strategy, RoundRobin):
                ent.strategy._index += selections                  # one select per forwarded Request (strategies.py:66-67)
            elif isinstance(ent.strategy, (ConsistentHash, IPHash)):
                ent.strategy._fallback._index += selections        # ... per KEY-LESS Request (strategies.py:309,362,420-421)
            off = int(a.rt_off[i])
            if i in g.scaled:
                # a scaled LoadBalancer: `_backends` is the initial backends, then the live managed instances in id order; a removed
                # instance has no entry any more, the strategy keeps what it learned of it (its weight, its current weight)
                sn, initial, pool = g.scaled[i]
                w, h = scalers[sn], health(i)
                slots = [q for q in range(len(initial) + len(pool)) if w["member"][q]]
                cand = initial + pool
                old = ent._backends
                ent._backends = {}
                for q in slots:
                    b = cand[q]
                    info = old.get(b.name) if q < len(initial) else None
                    ent._backends[b.name] = info if info is not None and info.backend is b else BackendInfo(backend=b, weight=1)
                    ent._backends[b.name].total_requests = int(stats["rt_taken"][off + q])
                if i in g.rr_base:
                    ent.strategy._index = g.rr_base[i] + selections    # (bound behind every window: absolute, not added once more)
                if hasattr(ent.strategy, "set_weight"):
                    for b in pool[:w["next_instance_id"]]:
                        ent.strategy._weights[b.name] = 1            # add_backend's set_weight(backend, 1)
                if isinstance(ent.strategy, WeightedRoundRobin) and h["current_weights"] is not None:
                    ent.strategy._selections = selections
                    ent.strategy._current_weights = {cand[q].name: v for q, v in sorted(h["current_weights"].items())}
                continue
            if i in g.deployed:
                # a deployed LoadBalancer: `_backends` in insertion order, as the device's member list holds it.  A backend that left
                # has no entry; one that came back has a new BackendInfo (the device counts its total_requests from 0 again); the
                # strategy keeps what it learned of every name (its weight, its current weight)
                dn, initial, pool = g.deployed[i]
                w, h = deployers[dn], health(i)
                cand = initial + pool
                old = ent._backends
                ent._backends = {}
                for q in w["members"]:
                    b = cand[q]
                    info = old.get(b.name)
                    if info is None or info.backend is not b or (q in w["readded"] and info.weight != 1):
                        info = BackendInfo(backend=b, weight=1)
                    ent._backends[b.name] = info
                    info.total_requests = int(stats["rt_taken"][off + q])
                if i in g.rr_base:
                    ent.strategy._index = g.rr_base[i] + selections    # (bound behind every window: absolute, not added once more)
                if hasattr(ent.strategy, "set_weight") and "weight_set" in w:
                    for q in w["weight_set"]:                        # a canary deployer's set_weight calls: the device's weights
                        ent.strategy._weights[cand[q].name] = int(w["weights"][q])
                elif hasattr(ent.strategy, "set_weight"):
                    for b in pool[:w["next_instance_id"]] + [cand[q] for q in w["readded"]]:
                        ent.strategy._weights[b.name] = 1            # add_backend's set_weight(backend, 1)
                if isinstance(ent.strategy, WeightedRoundRobin) and h["current_weights"] is not None:
                    ent.strategy._selections = selections
                    ent.strategy._current_weights = {cand[q].name: v for q, v in sorted(h["current_weights"].items())}
                continue
            for q, b in enumerate(ent.all_backends):
                ent._backends[b.name].total_requests = int(stats["rt_taken"][off + q])
            if health is not None:
                h = health(i)
                for q, b in enumerate(ent.all_backends):
                    ent._backends[b.name].is_healthy = bool(h["healthy"][q])
                ent._backends_marked_unhealthy += int(h["marks"][0])
                ent._backends_marked_healthy += int(h["marks"][1])
                if isinstance(ent.strategy, WeightedRoundRobin) and h["current_weights"] is not None:
                    # the live algorithm ran (csrc/hs_graph.hip): what it left, for every backend a select() ever saw (strategies.py:117-119)
                    ent.strategy._selections = selections
                    ent.strategy._current_weights = {b.name: h["current_weights"][q] for q, b in enumerate(ent.all_backends)
                                                     if q in h["current_weights"]}
                    continue
            if isinstance(ent.strategy, WeightedRoundRobin) and ent.all_backends:
                # what select() leaves in `_current_weights` after t selections of which n_i went to backend i: w_i * t - W * n_i
                # (strategies.py:125-132; a run starts from a fresh strategy, as every engine run starts from time zero)
                st = ent.strategy
                ws = [int(st.get_weight(b)) for b in ent.all_backends]
                st._selections = selections
                st._current_weights = ({b.name: w * selections - sum(ws) * int(stats["rt_taken"][off + q])
                                        for q, (b, w) in enumerate(zip(ent.all_backends, ws))} if selections else {})
        elif isinstance(ent, CanaryDeployer):
            w = deployers[i]
            (ent._deployments_started, ent._deployments_completed, ent._deployments_rolled_back, ent._stages_completed,
             ent._evaluations_performed, ent._evaluations_passed, ent._evaluations_failed) = (w[k] for k in GraphEngine._CANARY_NAMES[:7])
            ent.state = CanaryState(status=N.CANARY_STATUS[w["status"]], current_stage=w["current_stage"], total_stages=w["total_stages"],
                                    canary_traffic_pct=w["traffic_pct"])
            _dn, initial, pool = g.deployed[int(a.target[i])]
            cand = initial + pool
            ent._canary = pool[0] if w["has_canary"] else None
            ent._baseline_backends = [cand[q] for q in w["baseline"]]
            ent._stage_start_time = Instant(w["stage_start_ns"]) if w["stage_start_ns"] >= 0 else None
        elif isinstance(ent, RollingDeployer):
            w = deployers[i]
            (ent._deployments_started, ent._deployments_completed, ent._deployments_rolled_back, ent._instances_replaced,
             ent._health_checks_performed, ent._health_checks_passed, ent._health_checks_failed) = (w[k] for k in GraphEngine._DEPLOYER_NAMES[:7])
            ent.state = DeploymentState(status=N.DEPLOYMENT_STATUS[w["status"]], total_instances=w["total_instances"], replaced=w["replaced"],
                                        failed=w["failed"], current_batch=w["current_batch"])
            ent._next_instance_id, ent._health_fail_count = w["next_instance_id"], w["health_fail_count"]
            _dn, initial, pool = g.deployed[int(a.target[i])]
            cand = initial + pool
            ent._old_backends, ent._new_backends = [cand[q] for q in w["old"]], [cand[q] for q in w["new"]]
            ent._current_batch_old, ent._current_batch_new = [cand[q] for q in w["batch_old"]], [cand[q] for q in w["batch_new"]]
            ent._health_pass_count = {cand[q].name: v for q, v in sorted(w["pass_count"].items())}
        elif isinstance(ent, AutoScaler):
            w = scalers[i]
            (ent._evaluations, ent._scale_out_count, ent._scale_in_count, ent._instances_added, ent._instances_removed,
             ent._cooldown_blocks, ent._next_instance_id) = (w[k] for k in GraphEngine._SCALER_NAMES[:7])
            ent._last_scale_action = (None, "scale_out", "scale_in")[w["last_action"]]
            ent._last_scale_time = Instant(w["last_time_ns"]) if w["last_action"] else None
            ent.scaling_history = [ScalingEvent(Instant(int(t)), "scale_out" if act == 1 else "scale_in", int(c0), int(c1),
                                                f"{'Added' if act == 1 else 'Removed'} {int(cnt)} instances")
                                   for t, act, c0, c1, cnt in w["history"].tolist()]
            _sn, initial, pool = g.scaled[int(a.target[i])]
            ent._managed_servers = [pool[q - len(initial)] for q in range(len(initial), len(initial) + len(pool)) if w["member"][q]]
        elif isinstance(ent, HealthChecker):
            h = health(i)
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
        elif isinstance(ent, Bulkhead):
            w = wrapper(i)
            (ent._total_requests, ent._accepted_requests, ent._rejected_requests, ent._timed_out_requests, ent._queued_requests,
             ent._peak_concurrent, ent._peak_queue_depth, ent._active_count) = (w[k] for k in (
                 "total", "accepted", "rejected", "timed_out", "queued", "peak_concurrent", "peak_queue_depth", "active_count"))
            ent._next_request_id = w["next_request_id"]
            ent._wait_queue = [int(x) for x in w["queue_ids"]]
            ent._in_flight = {int(x): {} for x in w["in_flight_ids"]}
        elif isinstance(ent, _FLOWS):
            w = flow(i)                       # GraphEngine.flow(node) of a graph with one of the three
            if isinstance(ent, BatchProcessor):
                ent._batches_processed, ent._items_processed, ent._timeouts, ent._buffer_depth = (
                    w["batches_processed"], w["items_processed"], w["timeouts"], w["buffer_depth"])
            elif isinstance(ent, ConveyorBelt):
                ent._items_transported, ent._items_rejected, ent._items_in_transit = w["items_transported"], w["items_rejected"], w["items_in_transit"]
            else:
                ent._passed_through, ent._queued_while_closed, ent._rejected, ent._open_cycles, ent._queue_depth = (
                    w["passed_through"], w["queued_while_closed"], w["rejected"], w["open_cycles"], w["queue_depth"])
                ent._is_open = bool(w["is_open"])
        elif isinstance(ent, Client):
            w = client(i)
            (ent._requests_sent, ent._responses_received, ent._timeouts, ent._retries, ent._failures) = (w[k] for k in (
                "requests_sent", "responses_received", "timeouts", "retries", "failures"))
            ent._in_flight = {(int(rid) or None, int(att)): {} for rid, att in w["in_flight_keys"]}
            # _response_times: (now - start_time).to_seconds() of every response, in order -- the rows hold both in nanoseconds
            rows = order[bounds[i]:bounds[i + 1]]
            ent._response_times = [Duration(int(ns)).to_seconds() for ns in rec_t[rows]]
        elif isinstance(ent, TimeoutWrapper):
            w = wrapper(i)
            ent._total_requests, ent._successful_requests, ent._timed_out_requests = w["total"], w["successful"], w["timed_out"]
            ent._next_request_id = w["next_request_id"]
            ent._in_flight = {int(x): {} for x in w["in_flight_ids"]}
        elif isinstance(ent, RateLimitedEntity):
            st = stats["limiters"][i]
            ent._received, ent._forwarded, ent._queued, ent._dropped = (int(st[k]) for k in ("received", "forwarded", "queued", "dropped"))
            ent._queue_depth, ent._poll_scheduled = int(st["queue_depth"]), bool(st["poll_scheduled"])
            ent._events = (int(st["requests_handled"]), int(st["polls_handled"]))
            sel = order[bounds[i]:bounds[i + 1]]                 # its records: (time, hs_limiter_outcome), in processing order
            tt, code = rec_t[sel], rec_cr[sel]
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
        elif isinstance(ent, Probe):
            sel = order[bounds[i]:bounds[i + 1]]                 # its samples: (time, sampled integer)
            ent.data_sink._set(rec_t[sel].copy(), rec_cr[sel].copy(), Probe.value_map(ent.metric, ent.target))
        elif isinstance(ent, RandomRouter):
            ent.stats_routed = int(stats["routed"][i])
            tc: dict[str, int] = {}
            off = int(a.rt_off[i])
            for q, t in enumerate(ent.targets):               # target_counts[target.name] += 1 (random_router.py:37)
                c = int(stats["rt_taken"][off + q])
                if c:
                    tc[t.name] = tc.get(t.name, 0) + c
            ent.target_counts = tc
        else:
            sel = order[bounds[i]:bounds[i + 1]]
            ent._set_records(rec_t[sel].copy(), rec_cr[sel].copy())
            ent._device = device
