#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for Hedge and Fallback -- the yardstick of tests/test_hedge_host.py and
tests/test_gpu_hedge.py.  Run by hand where the reference is installed (refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_hedge.py          # writes tests/golden/live_hedge/part_*.npz

Recorded (tests/hedge_specs.py HEDGE reads them back): every spec of hedge_specs.recorded_specs() through
record_family.run_case(spec, "hedge").  The family is registered on record_family's and graph_family's objects here, at run time, as
tests/golden/make_golden_canary.py registers the canary deployer's: graph_family.wire / make_schedule are hedge_specs' (Hedges and
Fallbacks among the entities, the link faults of tests/link_fault_specs.py), the wrappers' seven Events are kinds 53 .. 59 at the
wrapper's node, a link fault's Events count as fault_on / fault_off at the link's node.  The reference's handlers run unchanged; two
counts are taken next to them for the coverage checks of tests/test_hedge_host.py -- `same_ns_pairs`: the `_hg_send_hedge` / `_hg_response`
pairs of one Hedge that were popped on one nanosecond, `late_primary`: the `_fb_primary_response` Events of a request whose
`_fb_timeout` had sent it to the fallback entity before.  The recorder first asserts that the product's host-side lowering takes every spec; after the run it asserts what the
named fixtures are there to show and the coverage that the host test asserts again on the files.
"""
from __future__ import annotations

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import canary_specs as CN  # noqa: E402
import deployer_specs as DS  # noqa: E402
import hedge_specs as HG  # noqa: E402
import link_fault_specs as LF  # noqa: E402
from happysimulator.components.network.network import Network  # noqa: E402
from happysimulator.components.resilience.fallback import Fallback  # noqa: E402
from happysimulator.components.resilience.hedge import Hedge  # noqa: E402
from happysimulator.faults.network_faults import InjectLatency, InjectPacketLoss  # noqa: E402

EV = RF.EV
EV["as_eval"] = len(EV)
for _name in DS.RD_EVENTS + CN.CN_EVENTS + HG.HG_EVENTS:
    EV[_name] = len(EV)
assert EV["hg_req"] == HG.EV_HG_FIRST and len(EV) == HG.N_KINDS
RF.REF_NS.Hedge, RF.REF_NS.Fallback, RF.REF_NS.Network, RF.REF_NS.InjectLatency, RF.REF_NS.InjectPacketLoss = (
    Hedge, Fallback, Network, InjectLatency, InjectPacketLoss)
RF._OWN_KINDS[Hedge] = {"_hg_response": EV["hg_resp"], "_hg_send_hedge": EV["hg_send"], None: EV["hg_req"]}
RF._OWN_KINDS[Fallback] = {"_fb_primary_response": EV["fb_prim_resp"], "_fb_timeout": EV["fb_timeout"], "_fb_fallback_response": EV["fb_fb_resp"],
                           None: EV["fb_req"]}
_cur = {}          # of the case that is running
_classify, _run_sim_windows = RF.classify, RF.MG.run_sim_windows


def wire(spec, F, ns):
    out = HG.wire(spec, F, ns)
    if ns is RF.REF_NS:
        _cur.clear()
        _cur.update(spec=spec, pools=out[0], events=None, last={}, same_ns_pairs=0, late_primary=0, window_states=[])
    return out


def make_schedule(ns, spec, pools):
    fs, handles = LF.make_schedule(ns, spec, pools)
    if ns is RF.REF_NS:
        _cur["handles"] = handles
    return fs, handles


def classify(e, node_of, by_name):
    et, t = e.event_type, e.target
    if et.startswith(("fault.latency.", "fault.loss.")):
        if _cur["events"] is None:                           # (the Events exist since Simulation.__init__)
            spec, pools = _cur["spec"], _cur["pools"]
            _cur["events"] = {id(ev): LF.fault_link(spec, ft, pools) for ft, h in zip(spec["faults"], _cur["handles"]) if LF.is_link_fault(ft)
                              for ev in h._events}
        return (EV["fault_on"] if ".activate:" in et else EV["fault_off"]), node_of[id(_cur["events"][id(e)])]
    live = not getattr(t, "_crashed", False)
    if isinstance(t, Hedge) and et in ("_hg_response", "_hg_send_hedge") and live:
        mine, other = (0, 1) if et == "_hg_response" else (1, 0)
        seen = _cur["last"].setdefault(id(t), [None, None])
        seen[mine] = e.time.nanoseconds
        _cur["same_ns_pairs"] += int(seen[other] == seen[mine])
        if seen[other] == seen[mine]:
            seen[0] = seen[1] = None
    if isinstance(t, Fallback) and et in ("_fb_primary_response", "_fb_timeout") and live:
        rid = e.context.get("metadata", {}).get("request_id")
        timed_out = _cur["last"].setdefault(id(t), set())
        if et == "_fb_timeout" and t._in_flight.get(rid, {}).get("state") == "primary":
            timed_out.add(rid)
        elif et == "_fb_primary_response":
            _cur["late_primary"] += int(rid in timed_out)
    return _classify(e, node_of, by_name)


def run_sim_windows(sim, spec):
    if not spec.get("windows"):
        return _run_sim_windows(sim, spec)
    for t in list(spec["windows"]) + [spec["end_s"]]:
        sim._run_window(RF.MG._at(spec, t))
        _cur["window_states"].append(HG.hedge_state(_cur["pools"]))
    sim._is_running = False
    return sim._build_summary()


def _section(c):
    out = HG.hedge_results(c.spec, c.pools)
    out.update(same_ns_pairs=int(_cur["same_ns_pairs"]), late_primary=int(_cur["late_primary"]))
    if c.spec.get("windows"):
        out.update(HG.window_states(_cur["window_states"]))
    return out


GF.wire, GF.make_schedule, RF.classify, RF.MG.run_sim_windows = wire, make_schedule, classify, run_sim_windows
RF._SECTION["hedge"] = _section
RF.SECTIONS["hedge"] = RF.SECTIONS["mixed"] + ("hedge",)
RF.N_KINDS["hedge"] = len(EV)


def coverage(results):
    """The counts tests/test_hedge_host.py asserts on the recordings: cases per Event kind and per situation."""
    kinds = np.sum([r["by_kind"][HG.EV_HG_FIRST:] > 0 for r in results], axis=0)
    return dict(kinds=kinds.tolist(), hedges_cancelled=sum(1 for r in results if (r["hg_stats"][:, 4] > 0).any()),
                hedge_wins=sum(1 for r in results if (r["hg_stats"][:, 2] > 0).any()),
                leaked=sum(1 for r in results if HG.leaked(r)), same_ns_pairs=sum(1 for r in results if r["same_ns_pairs"] > 0),
                late_primary=sum(1 for r in results if r["late_primary"] > 0))


def main():
    cases, results = {}, []
    for spec in HG.recorded_specs():
        sim, _pools = HG.build(spec)
        g = sim.lowered()                                  # the product takes this graph (host-side lowering; raises otherwise)
        sim._general_prepare(g, bool(spec.get("auto")))    # ... every scheduled Event of it
        assert g.arrays.has_hedges and len(sim._general_faults(g)) == sum(2 for _ in spec["faults"]) - sum(
            1 for ft in spec["faults"] if ft["kind"] == "crash" and ft.get("restart") is None), spec["name"]
        res = cases[HG.HEDGE.key("case", spec)] = RF.run_case(spec, "hedge", want_trace=spec["name"] in HG.TRACED)
        results.append(res)
        assert res["total_events"] <= 60_000 and spec["end_s"] <= 5.0, (spec["name"], res["total_events"])
        assert len(res["by_kind"]) == HG.N_KINDS and not res["by_kind"][39:HG.EV_HG_FIRST].any()
        print(spec["name"], res["total_events"], res["by_kind"][HG.EV_HG_FIRST:].tolist(), res["hg_stats"].tolist(), res["fb_stats"].tolist(),
              res["same_ns_pairs"], res["late_primary"], flush=True)
    get = lambda name: cases[HG.HEDGE.key("case", HG.FIXTURES[name])]  # noqa: E731
    # ---- what the fixtures are there to show
    for n in (1, 2, 3):
        r = get(f"hedge_{n}_delay_at_the_link_latency")
        assert r["same_ns_pairs"] > 0 and r["hg_stats"][0, 3] > 0, (n, r["hg_stats"])
        r = get(f"hedge_{n}_delay_above_the_link_latency")           # the primary's two responses delete the entry before any hedge
        assert r["hg_stats"][0, 3] == 0 and r["hg_stats"][0, 4] == 0 and r["hg_stats"][0, 1] == r["by_kind"][EV["hg_resp"]] // 2, r["hg_stats"]
        r = get(f"hedge_{n}_delay_below_the_link_latency")
        assert r["hg_stats"][0, 3] >= r["hg_stats"][0, 0] - 2 and r["hg_stats"][0, 2] == 0, r["hg_stats"]
    for name in ("hedge_in_front_of_a_server", "hedge_in_front_of_a_sink", "hedge_in_front_of_a_router", "hedge_in_front_of_a_limiter"):
        r = get(name)                                      # the primary wins on the nanosecond it was sent; no hedge ever goes out
        assert r["hg_stats"][0, 1] == r["hg_stats"][0, 0] > 10 and r["hg_stats"][0, 3] == 0 and r["hg_stats"][0, 6] == 0, (name, r["hg_stats"])
    r = get("crashed_hedge_target_restarts")
    leaked = r["hg_in_flight"]
    assert ((leaked[:, 3] == 3) & (leaked[:, 2] == 0) & (leaked[:, 4] == 0)).sum() > 3 and r["hg_stats"][0, 1] > 0, leaked       # all three hedges went out
    assert get("crashed_hedge_target_for_good")["hg_stats"][0, 6] > 5
    r = get("crashed_hedge_restarts")
    assert 0 < r["hg_stats"][0, 6] and r["hg_stats"][0, 0] < r["generated"][0], r["hg_stats"]
    assert get("hedge_over_a_jittered_lossy_link")["hg_stats"][0, 2] > 0 and get("hedge_over_a_jittered_lossy_link")["packets_dropped"][0] > 0
    r = get("hedge_over_a_lossy_link_every_packet_lost")   # a lost packet fires the hook at once: one response each
    assert r["packets_sent"][0] == 0 and r["hg_stats"][0, 1] == r["hg_stats"][0, 0] and r["hg_stats"][0, 6] == 0, r["hg_stats"]
    assert len(get("two_hedges_in_one_graph")["hg_stats"]) == 2 and get("two_hedges_in_one_graph")["hg_stats"][:, 0].min() > 5
    assert len(get("probe_on_a_hedge_in_flight_count")["probe_v"]) > 20 and get("probe_on_a_hedge_in_flight_count")["probe_v"].max() > 1
    r = get("fallback_timeout_below_the_primary_latency")
    assert r["fb_stats"][0, 1] == 0 and r["fb_stats"][0, 2] == r["fb_stats"][0, 3] > 10 and r["late_primary"] > 0 and r["fb_stats"][0, 5] == 0, r["fb_stats"]
    r = get("fallback_timeout_above_the_primary_latency")
    assert r["fb_stats"][0, 2] == 0 and r["fb_stats"][0, 1] > 10 and r["by_kind"][EV["fb_timeout"]] > 10, r["fb_stats"]
    r = get("fallback_timeout_none_the_primary_latency")
    assert r["by_kind"][EV["fb_timeout"]] == 0 and r["fb_stats"][0, 3] == 0 and r["fb_stats"][0, 1] > 10
    assert get("late_primary_response_after_the_timeout")["late_primary"] > 5
    r = get("fallback_entity_is_a_link_in_front_of_a_server")        # the fallback entity's hook fires twice
    assert r["by_kind"][EV["fb_fb_resp"]] >= 2 * r["fb_stats"][0, 4] - 2 > 10, (r["by_kind"][EV["fb_fb_resp"]], r["fb_stats"])
    r = get("crashed_fallback_entity")
    assert (r["fb_in_flight"][:, 2] == 1).sum() > 3 and HG.leaked(r), r["fb_stats"]
    r = get("crashed_primary")
    assert r["fb_stats"][0, 2] > 5 and r["fb_stats"][0, 1] > 5, r["fb_stats"]
    assert get("crashed_primary_without_a_timeout")["fb_stats"][0, 7] > 5
    r = get("inject_latency_on_the_primary_link")
    assert r["fb_stats"][0, 1] > 10 and r["fb_stats"][0, 2] > 5 and r["by_kind"][17:19].tolist() == [1, 1], r["fb_stats"]
    r = get("primary_and_fallback_share_one_sink")
    assert r["received"][0] > r["fb_stats"][0, 0] and r["fb_stats"][0, 3] > 3, (r["received"], r["fb_stats"])
    for name in HG.FIXTURES:
        if name.endswith("_in_windows"):
            a, b = get(name[:-len("_in_windows")]), get(name)
            for k in a:
                if k != "trace" and isinstance(a[k], np.ndarray):
                    assert a[k].tobytes() == b[k].tobytes(), (name, k)
    sizes = sorted(HG.group_sizes(HG.groups_spec()))
    assert 48 in sizes and 49 in sizes and len(sizes) == 16, sizes
    cov = coverage(results)
    print(cov)
    assert min(cov["kinds"]) >= 20 and min(cov[k] for k in ("hedges_cancelled", "hedge_wins", "leaked", "same_ns_pairs", "late_primary")) >= 5, cov
    assert len(HG.FIXTURES) >= 50 and len(HG.TRACED) >= 20 and HG.N_RANDOM >= 150
    HG.HEDGE.write(cases)


if __name__ == "__main__":
    main()
