"""The node arrays of the single-heap engine (include/hs_engine.h, hs_graph_nodes) and how one Simulation's arrays fall into the
parts no Request can cross."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

MAX_PARTS = 2048          # heaps one Simulation is spread over (hs_graph_run_parts): components beyond that share heaps


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
    def cn_params(self):
        """per node (None: no canary deployer; kept out of vars() like `rd_params`): None or (stages as [(traffic_percentage,
        evaluation_period), ...], hs_canary_evaluator, its limit, its threshold_multiplier, evaluation_interval) of a CANARY_DEPLOYER
        node; set through hs_graph_set_canary_deployer (its LoadBalancer: `target`)."""
        return getattr(self, "_cn_params", None)

    @cn_params.setter
    def cn_params(self, value):
        self._cn_params = value

    @property
    def hg_params(self):
        """[n, 4] int64 (None: neither a Hedge nor a Fallback; kept out of vars() like `rd_params`): HEDGE nodes -- hedge_delay in ns,
        max_hedges, -1, the in-flight table's first capacity (0: the engine's default); FALLBACK nodes -- timeout in ns (-1: None), 0,
        the node of the fallback entity (the node's second outgoing edge; the primary: `target`), the table's first capacity; set
        through hs_graph_set_hedge / hs_graph_set_fallback."""
        return getattr(self, "_hg_params", None)

    @hg_params.setter
    def hg_params(self, value):
        self._hg_params = value

    @property
    def st_params(self):
        """[n, 5] int64 (None: neither a pool nor a buffer; kept out of vars() like `rd_params`): POOLED_CYCLE nodes -- pool_size,
        cycle_time in ns, queue_capacity (0: unbounded), 0, -1; INVENTORY nodes -- initial_stock, reorder_point, order_quantity, the
        bits of lead_time (binary64 seconds), the node of the stockout_target (-1: none -- the node's second outgoing edge; the
        downstream: `target`); set through hs_graph_set_pool / hs_graph_set_inventory."""
        return getattr(self, "_st_params", None)

    @st_params.setter
    def st_params(self, value):
        self._st_params = value

    # the families a graph has nodes of: what GraphEngine applies and reads, what the run's results hold
    has_deployers = property(lambda self: self._rd_params is not None)
    has_canaries = property(lambda self: self.cn_params is not None)
    has_scalers = property(lambda self: self.as_params is not None)
    has_queue_policies = property(lambda self: self.qp_params is not None)
    has_flows = property(lambda self: self.flow_params is not None)
    has_clients = property(lambda self: self.cl_params is not None)
    has_health = property(lambda self: self.hc_params is not None or self.lb_healthy is not None)
    has_wrappers = property(lambda self: self.wrap_params is not None)
    has_hedges = property(lambda self: self.hg_params is not None)
    has_stock = property(lambda self: self.st_params is not None)

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


# the arrays one node in one part carries along: hs_graph_nodes' own and every family's per-node parameters
_PER_NODE = ("kind", "stream_base", "src_kind", "src_rate", "src_stop_after_ns", "concurrency", "lat_kind", "lat_mean_s", "link_lat_min_s",
             "link_loss_rate", "queue_cap", "src_profile_kind", "src_profile_params", "probe_metric", "probe_interval_s", "lb_strategy",
             "lb_vnodes", "src_n_clients", "lim_policy", "lim_params", "lim_count", "hc_params", "wrap_params", "cl_params", "flow_params",
             "qp_params", "as_params", "rd_params", "hg_params", "st_params")

# (a family's array, which of a part's nodes are of that family): a part without one drops the array and runs the loop it would run
# alone (without a checker: no health state unless a flag says so, below)
_FAMILY_OF = (("hc_params", lambda b: b.kind == N.NODE_HEALTH_CHECKER),
              ("rd_params", lambda b: b.kind == N.NODE_ROLLING_DEPLOYER),
              ("wrap_params", lambda b: (b.kind == N.NODE_BULKHEAD) | (b.kind == N.NODE_TIMEOUT_WRAPPER)),
              ("flow_params", lambda b: (b.kind >= N.NODE_BATCH_PROCESSOR) & (b.kind <= N.NODE_GATE)),
              ("qp_params", lambda b: b.qp_params[:, 0] != N.QUEUE_FIFO),
              ("as_params", lambda b: b.kind == N.NODE_AUTO_SCALER),
              ("cl_params", lambda b: b.kind == N.NODE_CLIENT),
              ("hg_params", lambda b: (b.kind == N.NODE_HEDGE) | (b.kind == N.NODE_FALLBACK)),
              ("st_params", lambda b: (b.kind == N.NODE_POOLED_CYCLE) | (b.kind == N.NODE_INVENTORY)))


def _offsets(blobs, dtype) -> np.ndarray:
    """Where each of `blobs` begins, and the last ends, once they stand back to back."""
    off = np.zeros(len(blobs) + 1, dtype)
    off[1:] = np.cumsum([len(x) for x in blobs])
    return off


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
    if a.hg_params is not None:                        # a Fallback's second edge: its fallback entity
        fb = np.nonzero(a.kind == N.NODE_FALLBACK)[0]
        src, dst = np.concatenate([src, fb]), np.concatenate([dst, a.hg_params[fb, 2]])
    if a.st_params is not None:                        # an InventoryBuffer's second edge: its stockout_target
        ib = np.nonzero((a.kind == N.NODE_INVENTORY) & (a.st_params[:, 4] >= 0))[0]
        src, dst = np.concatenate([src, ib]), np.concatenate([dst, a.st_params[ib, 4]])
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
    per_node = [nm for nm in _PER_NODE if getattr(a, nm) is not None]
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
        if b.hg_params is not None:
            fb = b.kind == N.NODE_FALLBACK
            b.hg_params[fb, 2] = new_index[b.hg_params[fb, 2]]
        if b.st_params is not None:
            ib = (b.kind == N.NODE_INVENTORY) & (b.st_params[:, 4] >= 0)
            b.st_params[ib, 4] = new_index[b.st_params[ib, 4]]
        for nm, of_family in _FAMILY_OF:
            if getattr(b, nm) is not None and not of_family(b).any():
                setattr(b, nm, None)
        if a.cn_params is not None and (b.kind == N.NODE_CANARY_DEPLOYER).any():
            b.cn_params = [a.cn_params[i] for i in ids]
        if b.as_params is not None:
            b.as_steps = [a.as_steps[i] for i in ids]
        if (b.lb_healthy is not None and b.hc_params is None and b.lb_healthy.all() and not (b.kind == N.NODE_AUTO_SCALER).any()
                and b.rd_params is None and b.cn_params is None):
            b.lb_healthy = None
        if b.cl_params is not None:
            tables = [a.cl_delays_ns[a.cl_delay_off[i]:a.cl_delay_off[i + 1]] for i in ids]
            b.cl_delay_off = _offsets(tables, np.int64)
            b.cl_delays_ns = np.concatenate(tables).astype(np.int64)
        if names is not None:
            blobs = [names[i] for i in ids]
            b.names = b"".join(blobs)
            b.name_off = _offsets(blobs, np.int32)
        parts.append((ids, pos, b))
    return parts
