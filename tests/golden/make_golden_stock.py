#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for PooledCycleResource and InventoryBuffer -- the yardstick of
tests/test_stock_host.py and tests/test_gpu_stock.py.  Run by hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_stock.py          # writes tests/golden/live_stock/part_*.npz

Recorded (tests/stock_specs.py STOCK reads them back): every spec of stock_specs.recorded_specs() through
record_family.run_case(spec, "stock").  The family is registered on record_family's and graph_family's objects here, at run time, as
tests/golden/make_golden_hedge.py registers the hedges': graph_family.wire is stock_specs' (pools and buffers among the entities), the
four Events of the two entities are kinds 60 .. 63 at the entity's node.  The reference's handlers run unchanged; two counts are taken
next to them for the coverage checks of tests/test_stock_host.py -- `requeued`: the Requests a pool re-sent to itself that found no
unit free when they were popped (an arrival of their nanosecond had taken it) and queued again, `lost`: the re-sent Requests that a
crashed or paused pool dropped.  The recorder first asserts that the product's host-side lowering takes every spec; after the run it
asserts what the named fixtures are there to show and the coverage that the host test asserts again on the files.  Run twice, it
writes the same bytes (the archive members carry a fixed date).
"""
from __future__ import annotations

import zipfile

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import canary_specs as CN  # noqa: E402
import deployer_specs as DS  # noqa: E402
import hedge_specs as HG  # noqa: E402
import stock_specs as ST  # noqa: E402
from happysimulator.components.industrial.inventory import InventoryBuffer  # noqa: E402
from happysimulator.components.industrial.pooled_cycle import PooledCycleResource  # noqa: E402
from happysimulator.core.event import ProcessContinuation  # noqa: E402

EV = RF.EV
EV["as_eval"] = len(EV)
for _name in DS.RD_EVENTS + CN.CN_EVENTS + HG.HG_EVENTS + ST.ST_EVENTS:
    EV[_name] = len(EV)
assert EV["pc_item"] == ST.EV_ST_FIRST and len(EV) == ST.N_KINDS == 64
RF.REF_NS.PooledCycleResource, RF.REF_NS.InventoryBuffer = PooledCycleResource, InventoryBuffer
RF.REF_METRIC.update(available="available", active="active", queued="queued", stock="stock")
_cur = {}          # of the case that is running
_classify, _run_sim_windows = RF.classify, RF.MG.run_sim_windows


def wire(spec, F, ns):
    out = ST.wire(spec, F, ns)
    if ns is RF.REF_NS:
        _cur.clear()
        _cur.update(spec=spec, pools=out[0], resent=set(), requeued=0, lost=0, window_states=[])
    return out


def classify(e, node_of, by_name):
    t = e.target
    if isinstance(t, PooledCycleResource):
        if isinstance(e, ProcessContinuation):
            if t._queue:                                     # the head of the line is re-sent with its own context
                _cur["resent"].add(id(t._queue[0].context))
            return EV["pc_cont"], node_of[id(t)]
        if id(e.context) in _cur["resent"]:
            _cur["resent"].discard(id(e.context))
            if getattr(t, "_crashed", False):
                _cur["lost"] += 1
            elif t._available == 0:
                _cur["requeued"] += 1
        return EV["pc_item"], node_of[id(t)]
    if isinstance(t, InventoryBuffer):
        return (EV["ib_replenish"] if e.event_type == "_InventoryReplenish" else EV["ib_item"]), node_of[id(t)]
    return _classify(e, node_of, by_name)


def run_sim_windows(sim, spec):
    if not spec.get("windows"):
        return _run_sim_windows(sim, spec)
    for t in list(spec["windows"]) + [spec["end_s"]]:
        sim._run_window(RF.MG._at(spec, t))
        _cur["window_states"].append(ST.stock_state(_cur["pools"]))
    sim._is_running = False
    return sim._build_summary()


def _section(c):
    out = ST.stock_results(c.spec, c.pools)
    out.update(requeued=int(_cur["requeued"]), lost=int(_cur["lost"]))
    if c.spec.get("windows"):
        out.update(ST.window_states(_cur["window_states"]))
    return out


GF.wire, RF.classify, RF.MG.run_sim_windows = wire, classify, run_sim_windows
RF._SECTION["stock"] = _section
RF.SECTIONS["stock"] = RF.SECTIONS["mixed"] + ("stock",)
RF.N_KINDS["stock"] = len(EV)


def rounded_replenishes(spec, res):
    """How many `_InventoryReplenish` Events of a traced one-buffer case were popped on a nanosecond that no consume's nanosecond plus
    int(lead_time * 1e9) gives: there the binary64 sum of seconds and its truncation decided, not an integer addition."""
    trace, lead_ns = res["trace"], int(spec["buffers"][0]["lt"] * 1_000_000_000)
    consumes = set(trace[trace[:, 1] == EV["ib_item"]][:, 0].tolist())
    return sum(1 for t in trace[trace[:, 1] == EV["ib_replenish"]][:, 0].tolist() if t - lead_ns not in consumes)


def coverage(results):
    """The counts tests/test_stock_host.py asserts on the recordings: cases per Event kind and per situation."""
    kinds = np.sum([r["by_kind"][ST.EV_ST_FIRST:] > 0 for r in results], axis=0)
    return dict(kinds=kinds.tolist(), requeued=sum(1 for r in results if r["requeued"] > 0), lost=sum(1 for r in results if r["lost"] > 0),
                rejected=sum(1 for r in results if (r["pc_state"][:, 4] > 0).any()), stockouts=sum(1 for r in results if (r["ib_state"][:, 1] > 0).any()),
                pending_at_the_end=sum(1 for r in results if ((r["ib_state"][:, 5] == 1) & (r["ib_state"][:, 6] == 0)).any()))


class _FixedDate(zipfile.ZipInfo):
    """An archive member dated 1980-01-01 whatever the clock says: the parts are the same bytes on every run.  numpy's savez makes its
    members through the module's name `zipfile.ZipInfo`, looked up when a member is opened; should a later numpy or zipfile do
    otherwise, main() fails at the check behind the write instead of leaving parts that change from run to run."""

    def __init__(self, filename="NoName", date_time=(1980, 1, 1, 0, 0, 0)):
        super().__init__(filename, (1980, 1, 1, 0, 0, 0))


def main():
    cases, results = {}, []
    for spec in ST.recorded_specs():
        sim, _pools = ST.build(spec)
        g = sim.lowered()                                  # the product takes this graph (host-side lowering; raises otherwise)
        sim._general_prepare(g, bool(spec.get("auto")))    # ... every scheduled Event of it
        assert g.arrays.has_stock, spec["name"]
        res = cases[ST.STOCK.key("case", spec)] = RF.run_case(spec, "stock", want_trace=spec["name"] in ST.TRACED)
        results.append(res)
        assert res["total_events"] <= 60_000 and (spec["end_s"] <= 5.0 or res["total_events"] <= 1_000), (spec["name"], res["total_events"])
        assert len(res["by_kind"]) == ST.N_KINDS and not res["by_kind"][39:ST.EV_ST_FIRST].any()
        print(spec["name"], res["total_events"], res["by_kind"][ST.EV_ST_FIRST:].tolist(), res["pc_state"].tolist(), res["ib_state"].tolist(),
              res["requeued"], res["lost"], flush=True)
    get = lambda name: cases[ST.STOCK.key("case", ST.FIXTURES[name])]  # noqa: E731
    # ---- what the fixtures are there to show
    r = get("pool_accepts_queues_and_rejects_within_three_arrivals")
    assert r["pc_state"][0, 4] > 0 and r["pc_state"][0, 3] > 0 and r["trace"][r["trace"][:, 1] == EV["pc_item"]][:3, 0].tolist() == [10 ** 8, 2 * 10 ** 8, 3 * 10 ** 8]
    for name in ("resent_request_loses_the_unit_to_an_arrival_of_its_nanosecond", "resent_request_into_a_bounded_line"):
        assert get(name)["requeued"] > 3, (name, get(name)["requeued"])
    assert get("resent_request_meets_arrivals_with_two_units")["pc_state"][0, 2] > 10       # (there the re-sent Request wins: the line only grows)
    r = get("pool_with_a_cycle_time_of_zero")
    assert r["pc_state"][0, 3] > 10 and r["by_kind"][EV["pc_cont"]] == r["pc_state"][0, 3]
    r = get("pool_without_a_downstream")
    assert r["pc_state"][0, 3] > 10 and r["received"][0] == 0
    assert (get("pool_feeding_a_pool")["pc_state"][:, 3] > 10).all() and get("pool_feeding_a_pool")["pc_state"][1, 4] > 0
    r = get("crashed_pool_restarts_with_a_line")
    assert r["lost"] >= 1 and r["pc_state"][0, 2] > 0 and r["pc_state"][0, 3] > 2, (r["lost"], r["pc_state"])
    assert get("paused_pool_across_a_cycle_end")["lost"] >= 1
    r = get("buffer_with_no_initial_stock")
    assert r["ib_state"][0, 1] > 0 and r["ib_state"][0, 2] > 1 and r["received"][1] == r["ib_state"][0, 1]
    r = get("reorder_point_at_the_initial_stock_reorders_at_the_first_consume")
    tr = r["trace"]
    first = tr[tr[:, 1] == EV["ib_item"]][0, 0]
    assert tr[tr[:, 1] == EV["ib_replenish"]][0, 0] == first + 400_000_000
    assert get("reorder_point_zero")["ib_state"][0, 2] > 1 and get("lead_time_zero")["ib_state"][0, 2] > 5
    rounded = {name: rounded_replenishes(ST.FIXTURES[name], get(name)) for name in ST.ROUNDED}
    assert min(rounded.values()) >= 3, rounded
    r = get("stock_out_with_a_target")
    assert r["ib_state"][0, 1] > 3 and r["received"][1] == r["ib_state"][0, 1]
    r = get("stock_out_without_a_target")
    assert r["ib_state"][0, 1] > 3 and r["received"][1] == 0
    r = get("both_targets_are_one_sink")
    assert r["received"][0] == r["ib_state"][0, 1] + r["ib_state"][0, 3] and r["ib_state"][0, 1] > 3
    r = get("crash_over_a_replenish_leaves_the_order_pending")
    assert r["ib_state"][0, 5] == 1 and r["ib_state"][0, 6] == 0 and r["ib_state"][0, 2] == 1 and r["ib_state"][0, 1] > 3, r["ib_state"]
    assert get("large_order_quantity")["ib_state"][0, 0] > (1 << 60)              # (beyond what a binary64 holds exactly)
    r = get("buffer_pool_server_sink")
    assert r["completed"][0] > 10 and r["pc_state"][0, 3] > 10 and r["ib_state"][0, 2] > 1
    r = get("pool_in_front_of_a_load_balancer")                  # (lb_stats: received, forwarded, failed, no backend, in flight)
    assert r["lb_stats"][0, 1] > 20 and r["pc_state"][0, 3] - r["lb_stats"][0, 0] in (0, 1) and (r["completed"] > 5).all()       # (the last forward may lie beyond the end)
    r = get("stock_outs_go_to_a_load_balancer")
    assert r["lb_stats"][0, 0] == r["ib_state"][0, 1] > 10 and r["received"][1] > 10
    assert len(get("probes_on_all_four_metrics")["probe_v"]) > 100 and len(set(get("probes_on_all_four_metrics")["probe_v"].tolist())) > 4
    r = get("auto_terminating_run_of_scheduled_requests")
    assert r["pending_events"] == 0 and r["ib_state"][0, 2] >= 1
    for name in ST.FIXTURES:
        if name.endswith("_in_windows"):
            a, b = get(name[:-len("_in_windows")]), get(name)
            for k in a:
                if k != "trace" and isinstance(a[k], np.ndarray):
                    assert a[k].tobytes() == b[k].tobytes(), (name, k)
    sizes = sorted(ST.group_sizes(ST.groups_spec()))
    assert 48 in sizes and 49 in sizes and len(sizes) == 6, sizes
    assert cases[ST.STOCK.key("case", ST.growth_spec())]["pc_state"][0, 2] > 300
    cov = coverage(results)
    print(cov, rounded)
    assert min(cov["kinds"]) >= 40 and min(cov[k] for k in ("requeued", "lost", "rejected", "stockouts", "pending_at_the_end")) >= 5, cov
    assert len(ST.FIXTURES) >= 45 and len(ST.TRACED) >= 20 and ST.N_RANDOM >= 100
    zipfile.ZipInfo, keep = _FixedDate, zipfile.ZipInfo
    try:
        ST.STOCK.write(cases)
    finally:
        zipfile.ZipInfo = keep
    import glob

    for path in sorted(glob.glob(ST.STOCK.rec_dir + "/*.npz")):
        with zipfile.ZipFile(path) as z:
            dated = {info.date_time for info in z.infolist()}
        assert dated == {(1980, 1, 1, 0, 0, 0)}, (path, dated)       # every member carries the fixed date: a second run writes these bytes again


if __name__ == "__main__":
    main()
