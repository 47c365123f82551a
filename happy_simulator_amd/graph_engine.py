"""General entity graphs: what the lowered entity classes can be wired into beyond the station shape of lowering.lower().

The station engines take `[Sources] -> Server -> {Sink | NetworkLink | RandomRouter}` with one sender per link, at most four
Sources per Server, four router targets ...; lowering.lower() refuses the rest by name.  `lower_general()` takes exactly those
graphs -- a NetworkLink with several senders (components/network/link.py:114-189), a RandomRouter with any number of targets,
Servers and routers among them, and with several upstreams (components/random_router.py:32-45), Server(downstream=<Server>)
next to links (components/server/server.py:64-122), any number of Sources per Server (load/source.py:93-180), any
FixedConcurrency (server/concurrency.py:67-141) -- and runs them on the device's single-heap loop (csrc/hs_graph.hip,
include/hs_engine.h "General entity graphs"): the reference's own (time, _sort_index) order event by event, ~2.4 us per event on
one lane.  Exact, not fast: Simulation only comes here with a graph lower() refused.

The path's Python side: graph_arrays.py (the node arrays, their parts), graph_lowering.py (entities -> arrays, every refusal), this
module (the engine's handle, one Simulation's parts behind the same readers) and graph_write_back.py (results -> entities); per
entity family one `_lower_*` function, one `_apply_*` method with its readers here, one `_write_*` function.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .graph_arrays import MAX_PARTS, GraphArrays, _ptr, split_parts  # noqa: F401

DEFAULT_MAX_EVENTS = 200_000_000          # ~ minutes on the one lane; Simulation(max_graph_events=) raises it


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
        self._table_capacity = int(table_capacity)       # (not 0: the first capacity of every wrapper's and Client's in-flight table)
        try:
            for flag, apply in self._APPLY:
                if flag is None or getattr(arrays, flag):
                    apply(self, arrays)
        except BaseException:
            self.close()
            raise

    # one _apply_* per family: its nodes' parameters onto the new handle (hs_graph_set_*)
    def _apply_lb_weights(self, a: GraphArrays) -> None:
        """WeightedRoundRobin / WeightedLeastConnections: strategy._weights, per LoadBalancer in slot order (the default is all ones)."""
        if a.lb_weights is None or a.lb_strategy is None:
            return
        w = np.ascontiguousarray(a.lb_weights, np.int32)
        for i in np.nonzero((a.kind == N.NODE_LB) & ((a.lb_strategy == N.LB_WEIGHTED_ROUND_ROBIN) |
                                                     (a.lb_strategy == N.LB_WEIGHTED_LEAST_CONNECTIONS)))[0]:
            off, cnt = int(a.rt_off[i]), int(a.rt_cnt[i])
            wi = np.ascontiguousarray(w[off:off + cnt])
            if cnt and (wi != 1).any():
                self._check(self._lib.hs_graph_set_lb_weights(self._h, int(i), _ptr(wi), cnt))

    def _apply_limiters(self, a: GraphArrays) -> None:
        if a.lim_policy is None:
            return
        for i in np.nonzero(a.kind == N.NODE_RATE_LIMITER)[0]:
            q = N.LimiterPolicyParams(C.sizeof(N.LimiterPolicyParams), int(a.lim_policy[i]), *(float(v) for v in a.lim_params[i]),
                                      int(a.lim_count[i]))
            self._check(self._lib.hs_graph_set_limiter_policy(self._h, int(i), C.byref(q)))

    def _apply_health(self, a: GraphArrays) -> None:
        if a.lb_healthy is not None:
            fl = np.ascontiguousarray(a.lb_healthy, np.uint8)
            for i in np.nonzero(a.kind == N.NODE_LB)[0]:
                off, cnt = int(a.rt_off[i]), int(a.rt_cnt[i])
                fi = np.ascontiguousarray(fl[off:off + cnt])
                self._check(self._lib.hs_graph_set_lb_health(self._h, int(i), _ptr(fi) if cnt else _ptr(np.zeros(1, np.uint8)), cnt))
        for i in np.nonzero(a.kind == N.NODE_HEALTH_CHECKER)[0]:
            iv, to, ht, ut, running = a.hc_params[i]
            self._check(self._lib.hs_graph_set_health_checker(self._h, int(i), int(a.target[i]), float(iv), float(to), int(ht), int(ut),
                                                              int(running)))

    def _apply_scalers(self, a: GraphArrays) -> None:
        for i in np.nonzero(a.kind == N.NODE_AUTO_SCALER)[0]:
            pol, p0, p1, lo, hi, iv, cd_out, cd_in, pool, running = a.as_params[i]
            steps = a.as_steps[i] or []
            thr = np.array([t for t, _ in steps] or [0.0], np.float64)
            adj = np.array([d for _, d in steps] or [0], np.int32)
            self._check(self._lib.hs_graph_set_auto_scaler(self._h, int(i), int(a.target[i]), int(pol), float(p0), float(p1), len(steps),
                                                           _ptr(thr), _ptr(adj), int(lo), int(hi), float(iv), float(cd_out), float(cd_in),
                                                           int(pool), int(running)))

    def _apply_rolling_deployers(self, a: GraphArrays) -> None:
        for i in np.nonzero(a.kind == N.NODE_ROLLING_DEPLOYER)[0]:
            batch, iv, thr, fails, pool = a.rd_params[i]
            self._check(self._lib.hs_graph_set_rolling_deployer(self._h, int(i), int(a.target[i]), int(batch), float(iv), int(thr),
                                                                int(fails), int(pool)))

    def _apply_canary_deployers(self, a: GraphArrays) -> None:
        for i in np.nonzero(a.kind == N.NODE_CANARY_DEPLOYER)[0]:
            stages, evaluator, limit, mult, iv = a.cn_params[i]
            pct = np.array([s_[0] for s_ in stages], np.float64)
            period = np.array([s_[1] for s_ in stages], np.float64)
            self._check(self._lib.hs_graph_set_canary_deployer(self._h, int(i), int(a.target[i]), len(stages), _ptr(pct), _ptr(period),
                                                               int(evaluator), float(limit), float(mult), float(iv)))

    def _apply_wrappers(self, a: GraphArrays) -> None:
        for i in np.nonzero((a.kind == N.NODE_BULKHEAD) | (a.kind == N.NODE_TIMEOUT_WRAPPER))[0]:
            mc, mq, mw, to, cap = a.wrap_params[i]
            self._check(self._lib.hs_graph_set_wrapper(self._h, int(i), int(mc), int(mq), float(mw), float(to),
                                                       self._table_capacity or int(cap)))

    def _apply_hedges(self, a: GraphArrays) -> None:
        for i in np.nonzero((a.kind == N.NODE_HEDGE) | (a.kind == N.NODE_FALLBACK))[0]:
            delay_ns, max_hedges, fallback, cap = (int(v) for v in a.hg_params[i])
            if a.kind[i] == N.NODE_HEDGE:
                self._check(self._lib.hs_graph_set_hedge(self._h, int(i), delay_ns, max_hedges, self._table_capacity or cap))
            else:
                self._check(self._lib.hs_graph_set_fallback(self._h, int(i), fallback, delay_ns, self._table_capacity or cap))

    def _apply_stock(self, a: GraphArrays) -> None:
        for i in np.nonzero((a.kind == N.NODE_POOLED_CYCLE) | (a.kind == N.NODE_INVENTORY))[0]:
            row = a.st_params[i]
            if a.kind[i] == N.NODE_POOLED_CYCLE:
                self._check(self._lib.hs_graph_set_pool(self._h, int(i), int(row[0]), int(row[1]), int(row[2])))
            else:
                self._check(self._lib.hs_graph_set_inventory(self._h, int(i), int(row[0]), int(row[1]), int(row[2]),
                                                             float(row[3:4].view(np.float64)[0]), int(row[4])))

    def _apply_clients(self, a: GraphArrays) -> None:
        for i in np.nonzero(a.kind == N.NODE_CLIENT)[0]:
            timeout, cap = a.cl_params[i]
            delays = np.ascontiguousarray(a.cl_delays_ns[a.cl_delay_off[i]:a.cl_delay_off[i + 1]], np.int64)
            self._check(self._lib.hs_graph_set_client(self._h, int(i), float(timeout), _ptr(delays) if len(delays) else None, len(delays),
                                                      self._table_capacity or int(cap)))

    def _apply_flows(self, a: GraphArrays) -> None:
        for i in np.nonzero((a.kind >= N.NODE_BATCH_PROCESSOR) & (a.kind <= N.NODE_GATE))[0]:
            count, delay_ns, aux_ns, flag = (int(v) for v in a.flow_params[i])
            self._check(self._lib.hs_graph_set_flow(self._h, int(i), count, delay_ns, aux_ns, flag))

    def _apply_queue_policies(self, a: GraphArrays) -> None:
        for i in np.nonzero((a.kind == N.NODE_SERVER) & (a.qp_params[:, 0] != N.QUEUE_FIFO))[0]:
            pol, cap, thr, target, interval = a.qp_params[i]
            self._check(self._lib.hs_graph_set_queue_policy(self._h, int(i), int(pol), int(cap), int(thr), float(target), float(interval)))

    # (GraphArrays' flag of a family, None: the method looks for itself), in the order the device takes them: a LoadBalancer's health
    # before its scaler ...
    _APPLY = ((None, _apply_lb_weights), (None, _apply_limiters), ("has_health", _apply_health), ("has_scalers", _apply_scalers),
              ("has_deployers", _apply_rolling_deployers), ("has_canaries", _apply_canary_deployers), ("has_wrappers", _apply_wrappers),
              ("has_hedges", _apply_hedges), ("has_stock", _apply_stock), ("has_clients", _apply_clients), ("has_flows", _apply_flows), ("has_queue_policies", _apply_queue_policies))

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

    _HEDGE_NAMES = ("total_requests", "primary_wins", "hedge_wins", "hedges_sent", "hedges_cancelled", "next_request_id", "in_flight_count",
                    "table_capacity")
    _FALLBACK_NAMES = ("total_requests", "primary_successes", "primary_failures", "fallback_invocations", "fallback_successes",
                       "fallback_failures", "next_request_id", "in_flight_count", "table_capacity")

    def hedge(self, node: int) -> dict:
        """hs_graph_get_hedge / hs_graph_get_fallback of a Hedge or Fallback node: its counters by name and `entries`, the requests in
        flight by ascending id -- rows (id, start_time ns, completed, hedges_sent, responses_received) of a Hedge, (id, start_time ns,
        state: 0 "primary" / 1 "fallback") of a Fallback."""
        hedge = self.arrays.kind[node] == N.NODE_HEDGE
        get, names, width = ((self._lib.hs_graph_get_hedge, self._HEDGE_NAMES, 5) if hedge else
                             (self._lib.hs_graph_get_fallback, self._FALLBACK_NAMES, 3))
        c = np.zeros(len(names), np.int64)
        self._check(get(self._h, int(node), _ptr(c), None, 0, None))
        out = {k: int(v) for k, v in zip(names, c)}
        live = out["in_flight_count"]
        rows = np.zeros((max(live, 1), width), np.int64)
        self._check(get(self._h, int(node), None, _ptr(rows), live, None))
        rows = rows[:live]
        out["entries"] = rows[np.argsort(rows[:, 0], kind="stable")]
        return out

    def hedge_events(self) -> np.ndarray:
        """The graph's Hedge request / response / send-hedge and Fallback request / primary-response / timeout / fallback-response
        Events of the run."""
        events = np.zeros(N.HEDGE_KINDS, np.int64)
        self._check(self._lib.hs_graph_get_hedge(self._h, -1, None, None, 0, _ptr(events)))
        return events

    _POOL_NAMES = ("available", "active", "queued", "completed", "rejected")
    _INVENTORY_NAMES = ("stock", "stockouts", "reorders", "items_consumed", "items_replenished", "order_pending")

    def stock(self, node: int) -> dict:
        """hs_graph_get_pool / hs_graph_get_inventory of a PooledCycleResource or InventoryBuffer node: its counters by name."""
        pool = self.arrays.kind[node] == N.NODE_POOLED_CYCLE
        get, names = (self._lib.hs_graph_get_pool, self._POOL_NAMES) if pool else (self._lib.hs_graph_get_inventory, self._INVENTORY_NAMES)
        c = np.zeros(len(names), np.int64)
        self._check(get(self._h, int(node), _ptr(c), None))
        return {k: int(v) for k, v in zip(names, c)}

    def stock_events(self) -> np.ndarray:
        """The graph's pool Request / cycle end / consume Request / replenish Events of the run."""
        events = np.zeros(N.STOCK_KINDS, np.int64)
        self._check(self._lib.hs_graph_get_pool(self._h, -1, None, _ptr(events)))
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

    def _locate(self, node: int):
        """(the engine of the part that holds `node`, its number there)."""
        for (ids, _pos, _b), e in zip(self.parts, self.engines):
            at = np.searchsorted(ids, node)
            if at < len(ids) and ids[at] == node:
                return e, int(at)
        raise KeyError(node)

    def _of_node(reader: str):
        """GraphEngine's `reader` of one node, by the Simulation's node number."""
        def read(self, node: int) -> dict:
            e, at = self._locate(node)
            return getattr(e, reader)(at)
        return read

    def _summed(reader: str, as_type=None):
        """GraphEngine's `reader` of a whole graph -- a count, or counts by kind --, summed over the parts."""
        def read(self):
            total = np.sum([getattr(e, reader)() for e in self.engines], axis=0)
            return total if as_type is None else as_type(total)
        return read

    def _int64(v):
        return v.astype(np.int64)

    queue_policy, flow, client, wrapper = _of_node("queue_policy"), _of_node("flow"), _of_node("client"), _of_node("wrapper")
    hedge, hedge_events = _of_node("hedge"), _summed("hedge_events", _int64)
    stock, stock_events = _of_node("stock"), _summed("stock_events", _int64)
    canary, deployer, scaler, health = _of_node("canary"), _of_node("deployer"), _of_node("scaler"), _of_node("health")
    health_events, wrapper_events = _summed("health_events", _int64), _summed("wrapper_events", _int64)
    client_events, flow_events = _summed("client_events", _int64), _summed("flow_events", _int64)
    deployer_events, canary_events, scaler_events = _summed("deployer_events"), _summed("canary_events"), _summed("scaler_events", int)

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


# (behind the classes: both modules import GeneralGraph / GraphEngine from here)
from .graph_lowering import (client_delay_table, deployer_pool_size, flow_delay_ns, keyless_hazard, lower_general,  # noqa: E402,F401
                             scaler_pool_size)
from .graph_write_back import write_back_general  # noqa: E402,F401


