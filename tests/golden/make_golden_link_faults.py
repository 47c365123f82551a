#!/usr/bin/env python3
"""Record what the LIVE upstream reference computes for InjectLatency and InjectPacketLoss on links registered in a Network -- the
yardstick of tests/test_link_faults_host.py and tests/test_gpu_link_faults.py.  Run by hand where the reference is installed
(refshim.py: HS_REFERENCE_ROOT):

    python tests/golden/make_golden_link_faults.py          # writes tests/golden/live_link_faults/part_*.npz

Recorded (tests/link_fault_specs.py LINK_FAULTS reads them back): every spec of link_fault_specs.recorded_specs() through
record_family.run_case(spec, "link_faults").  The family is registered on record_family's and graph_family's objects here, at run
time: graph_family.wire puts the spec's Networks among the entities, graph_family.make_schedule builds the two link faults,
record_family.classify counts a link fault's activation as kind fault_on and its deactivation as fault_off at the LINK's node (the
Events themselves are aimed at a callback entity) and follows which fault is in force on every link; the section records
link_fault_specs.link_results -- packet_loss_rate, the latency object, the fault in force, the values read from the LOSS stream,
every Network's traffic_matrix() and counters -- and `link_jitter_draws`.  `_Reference` is subclassed so that a link's two Philox
streams count their reads.  The reference's handlers run unchanged.  The recorder first asserts that the product's host-side
lowering takes every spec; after the run it asserts what each named fixture is there to show.  Running it again rewrites the parts
byte for byte.
"""
from __future__ import annotations

import numpy as np

import record_family as RF  # (puts tests/ and the repository root on sys.path; installs the reference's import path)
import graph_family as GF  # noqa: E402
import link_fault_specs as LS  # noqa: E402
from happysimulator.components.network.network import Network  # noqa: E402
from happysimulator.faults.network_faults import InjectLatency, InjectPacketLoss  # noqa: E402

EV = RF.EV
RF.REF_NS.Network, RF.REF_NS.InjectLatency, RF.REF_NS.InjectPacketLoss = Network, InjectLatency, InjectPacketLoss
_cur = {}          # of the case that is running: spec, pools, handles, the link and fault of every link-fault Event, the fault in force


class _Counted:
    """A Philox stream that counts its reads."""

    def __init__(self, stream):
        self._stream, self.reads = stream, 0

    def next_uniform(self):
        self.reads += 1
        return self._stream.next_uniform()


class _LinkFaultReference(RF._Reference):
    def link(self, l, lk):
        link = super().link(l, lk)
        link._loss_stream = _Counted(link._loss_stream)
        if hasattr(link.jitter, "_stream"):
            link.jitter._stream = _Counted(link.jitter._stream)
        return link


_wire, _classify, _run_sim_windows = GF.wire, RF.classify, RF.MG.run_sim_windows


def run_sim_windows(sim, spec):
    """make_golden.run_sim_windows, with the links' object state read behind every window of a windowed spec."""
    if not spec.get("windows"):
        return _run_sim_windows(sim, spec)
    _cur["window_states"] = []
    for t in list(spec["windows"]) + [spec["end_s"]]:
        sim._run_window(RF.MG._at(spec, t))
        _cur["window_states"].append(LS.link_state(_cur["pools"]))
    sim._is_running = False
    return sim._build_summary()


def wire(spec, F, ns):
    pools, sources, probes, entities = _wire(spec, F, ns)
    entities = LS.with_networks(spec, pools, entities, ns)
    if ns is RF.REF_NS:
        _cur.clear()
        _cur.update(spec=spec, pools=pools, events=None, active=[[-1, -1] for _ in pools["link"]])
    return pools, sources, probes, entities


def make_schedule(ns, spec, pools):
    fs, handles = LS.make_schedule(ns, spec, pools)
    if ns is RF.REF_NS:
        _cur["handles"] = handles
    return fs, handles


def classify(e, node_of, by_name):
    et = e.event_type
    if not et.startswith(("fault.latency.", "fault.loss.")):
        return _classify(e, node_of, by_name)
    if _cur["events"] is None:                               # (the Events exist since Simulation.__init__)
        spec, pools = _cur["spec"], _cur["pools"]
        _cur["events"] = {id(ev): (i, LS.fault_link(spec, ft, pools)) for i, (ft, h) in enumerate(zip(spec["faults"], _cur["handles"]))
                          if LS.is_link_fault(ft) for ev in h._events}
    index, link = _cur["events"][id(e)]
    on = ".activate:" in et
    l = next(i for i, x in enumerate(_cur["pools"]["link"]) if x is link)
    _cur["active"][l][0 if et.startswith("fault.latency.") else 1] = index if on else -1
    return (EV["fault_on"] if on else EV["fault_off"]), node_of[id(link)]


def _section(c):
    links = c.pools["link"]
    out = LS.link_results(c.spec, c.pools, _cur["active"], [lk._loss_stream.reads for lk in links])
    out["link_jitter_draws"] = np.array([lk.jitter._stream.reads if hasattr(lk.jitter, "_stream") else 0 for lk in links], np.int64)
    if c.spec.get("windows"):
        out.update(LS.window_states(_cur["window_states"]))
    return out


GF.wire, GF.make_schedule, RF.classify, RF.MG.run_sim_windows = wire, make_schedule, classify, run_sim_windows
RF._Reference = _LinkFaultReference
RF._SECTION["link_faults"] = _section
RF.SECTIONS["link_faults"] = RF.SECTIONS["mixed"] + ("link_faults",)
RF.N_KINDS["link_faults"] = len(RF.EV)


def run_case(spec, want_trace=False):
    return RF.run_case(spec, "link_faults", want_trace=want_trace)


def _same(a, b, but=()):
    assert set(a) == set(b)
    for k in a:
        if k in but:
            continue
        x, y = a[k], b[k]
        ok = (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y
        assert ok, k


def _created(r):
    """(created_at, latency) in seconds of every Sink record."""
    return r["sink_t_ns"] / 1e9 - r["sink_latency_s"], r["sink_latency_s"]


def main():
    cases = {}
    for spec in LS.recorded_specs():
        sim, _pools = LS.build(spec)
        g = sim.lowered()                                  # the product takes this graph (host-side lowering; raises otherwise)
        sim._general_prepare(g, bool(spec.get("auto")))    # ... every scheduled Event of it
        n_lf = sum(2 for ft in spec["faults"] if LS.is_link_fault(ft))
        assert sum(1 for f in sim._general_faults(g) if len(f) == 5) == n_lf > 0, spec["name"]       # ... and every link fault
        res = cases[LS.LINK_FAULTS.key("case", spec)] = run_case(spec, want_trace=spec["name"] in LS.TRACED)
        assert res["total_events"] <= 40_000, (spec["name"], res["total_events"])
        assert spec.get("auto") or spec["end_s"] <= 20.0
        assert len(res["by_kind"]) == 39                   # no new Event kinds
        print(spec["name"], res["total_events"], res["by_kind"][17:19].tolist(), res["link_loss_rate"].tolist(), res["link_active_fault"].tolist(),
              res["link_loss_draws"].tolist(), res["packets_dropped"].tolist(), res["events_cancelled"], flush=True)
    get = lambda name: cases[LS.LINK_FAULTS.key("case", LS.FIXTURES[name])]  # noqa: E731
    bare = lambda name, **kw: run_case(dict(LS.without_link_faults(LS.FIXTURES[name]), **kw))  # noqa: E731
    # ---- what each fixture is there to show
    r = get("latency_window")                              # Sink latencies step up inside the window and return afterwards
    cr, lt = _created(r)
    inside = (cr > 1.0 - 1e-7) & (cr < 2.0 - 1e-7)
    assert inside.sum() == 8 and (~inside).sum() >= 15 and np.allclose(lt[inside], 0.08) and np.allclose(lt[~inside], 0.03), (cr, lt)
    assert cr[~inside].max() > 2.0 and r["link_active_fault"].tolist() == [[-1, -1]] and r["link_latency"][0, 0] == 0.0
    r = get("latency_spike_behind_a_client")               # timeouts and retries, every timeout issued inside the window
    spec = LS.FIXTURES["latency_spike_behind_a_client"]
    assert r["cl_stats"][0, 2] > 0 and r["cl_stats"][0, 3] > 0, r["cl_stats"]
    assert bare("latency_spike_behind_a_client")["cl_stats"][0, 2] == 0
    # (a run processes the one Event beyond its end: the Request of 1.0 s would still be sent and its timeout handled)
    assert run_case(dict(spec, name="until_the_window", end_s=0.99))["cl_stats"][0, 2] == 0
    assert run_case(dict(spec, name="past_the_window", end_s=1.6))["cl_stats"][0, 2] == r["cl_stats"][0, 2]
    r = get("exponential_jitter_plus_extra_latency")       # no extra random draw
    b = bare("exponential_jitter_plus_extra_latency")
    assert r["link_jitter_draws"][0] == b["link_jitter_draws"][0] > 50 and r["sink_latency_s"].tobytes() != b["sink_latency_s"].tobytes()
    r = get("loss_window_on_a_lossless_link")              # drops only inside the window; the first draw comes after Requests went through
    assert r["packets_dropped"][0] > 0 and 0 < r["link_loss_draws"][0] < r["packets_sent"][0] + r["packets_dropped"][0]
    assert run_case(dict(LS.FIXTURES["loss_window_on_a_lossless_link"], name="until_the_window", end_s=1.0))["packets_sent"][0] > 10
    for name, end, dropped in (("until_the_window", 1.0, 0), ("past_the_window", 2.0, r["packets_dropped"][0])):
        assert run_case(dict(LS.FIXTURES["loss_window_on_a_lossless_link"], name=name, end_s=end))["packets_dropped"][0] == dropped
    r = get("loss_on_a_lossy_link_whose_sum_exceeds_one")  # min(1.0, 0.3 + 0.9): everything inside the window is dropped
    cr, _lt = _created(r)
    assert not ((cr > 1.0) & (cr < 2.0)).any() and (cr < 1.0).any() and (cr > 2.0).any() and r["packets_dropped"][0] > 30
    r = get("loss_rate_zero_on_a_lossless_link")           # no draw, and the results of the run without the fault
    assert r["link_loss_draws"][0] == 0
    _same(r, bare("loss_rate_zero_on_a_lossless_link"), but=("by_kind", "total_events", "fault_stats", "fault_events", "pending_events"))
    r = get("two_overlapping_latency_faults_on_one_link")  # the last activation wins, the first deactivation restores the original
    cr, lt = _created(r)
    for lo, hi, want in ((0.0, 1.0, 0.03), (1.0, 1.5, 0.08), (1.5, 2.0, 0.11), (2.0, 3.0, 0.03)):
        sel = (cr > lo - 1e-7) & (cr < hi - 1e-7)
        assert sel.sum() >= 5 and np.allclose(lt[sel], want), (lo, hi, lt[sel])
    r = get("latency_end_before_start")                    # left on for good
    assert r["link_active_fault"].tolist() == [[0, -1]] and r["link_latency"][0].tolist() == [1.0, 0.02, 0.04, 0.02 + 0.04]
    r = get("loss_end_before_start")
    assert r["link_active_fault"].tolist() == [[-1, 0]] and r["link_loss_rate"].tolist() == [0.4]
    for name in ("windows_that_outlast_the_run", "windows_that_outlast_the_run_in_windows"):
        r = get(name)
        assert r["link_active_fault"].tolist() == [[0, 1]] and r["link_loss_rate"].tolist() == [0.2]
        assert r["link_latency"][0].tolist() == [1.0, 0.02, 0.03, 0.02 + 0.03] and r["link_latency_ns"][0] == 50_000_000
    _same({k: v for k, v in get("windows_that_outlast_the_run").items() if k != "trace"},
          {k: v for k, v in get("windows_that_outlast_the_run_in_windows").items() if k not in LS.WINDOW_KEYS})
    r = get("windows_that_outlast_the_run_in_windows")     # windows end at 0.5, 1.0, 1.5, 2.25 and 3.0 s: each processes the one Event beyond it
    assert r["window_link_latency"][:, 0, 0].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0] and r["window_link_loss_rate"][:, 0].tolist() == [0.0, 0.0, 0.2, 0.2, 0.2]
    assert r["window_link_latency_ns"][:, 0].tolist() == [20_000_000] + [50_000_000] * 4
    r = get("handles_cancelled_before_and_after_the_simulation_exists")
    assert r["events_cancelled"] == 2 and r["fault_stats"].tolist() == [3, 0, 0, 2] and r["by_kind"][17:19].tolist() == [2, 2]
    assert r["packets_dropped"][0] == 0 and r["link_loss_draws"][0] == 0       # (the loss fault never fired; the first latency fault did)
    r = get("crashed_link_while_its_fault_events_fire")    # aimed at a callback: the crashed link does not drop them
    assert r["by_kind"][17:19].tolist() == [3, 3] and r["link_active_fault"].tolist() == [[-1, -1]] and r["packets_dropped"][0] > 0
    cr, lt = _created(r)
    assert not ((cr > 0.8) & (cr < 2.2)).any() and np.allclose(lt[(cr > 2.2) & (cr < 2.4)].min(), 0.08, atol=0.011)
    r = get("activation_on_the_nanosecond_a_request_reaches_the_link")
    cr, lt = _created(r)
    at = lambda t: lt[np.abs(cr - t) < 1e-7]  # noqa: E731
    assert np.allclose(at(1.0), 0.08) and np.allclose(at(0.875), 0.03) and np.allclose(at(2.0), 0.03) and len(at(1.5)) == 1 and r["packets_dropped"][0] == 0
    tr = r["trace"]
    rows = tr[tr[:, 0] == 10 ** 9]
    assert rows[0, 1] == EV["fault_on"] and len(rows) >= 3, rows
    r = get("network_name_none_with_two_networks")
    assert r["link_active_fault"].tolist() == [[-1, -1], [-1, -1]] and r["packets_dropped"].tolist()[0] == 0 < r["packets_dropped"].tolist()[1]
    assert [x[0] for x in r["traffic_routes"]] == ["edge", "core"]
    r = get("get_link_through_the_default_link")
    assert r["packets_dropped"][0] > 0 and len(r["traffic_routes"]) == 0 and r["by_kind"][17:19].tolist() == [2, 2]
    r = get("lost_packet_under_a_bulkhead_hook")
    # the hook fires once for a lost packet (the generator ends before its first yield) and twice for a delivered one (at the end of
    # transit and at the egress): every permit is back, every response Event accounted for
    sent, lost, w = int(r["packets_sent"][0]), int(r["packets_dropped"][0]), r["wrap_stats"][0]
    assert lost > 5 and r["by_kind"][EV["bh_resp"]] == 2 * sent + lost and w[1] == sent + lost, (sent, lost, r["by_kind"][EV["bh_resp"]], w)
    assert w[7] == 0 and w[11] == 0 and w[9] == 2 and r["pending_events"] <= 4, w      # active_count, len(_in_flight), available_permits
    r = get("lost_packet_under_a_timeout_wrapper_hook")
    assert r["packets_dropped"][0] > 5 and r["by_kind"][EV["tw_resp"]] > 0 and r["wrap_stats"][0, 2] > 0
    r = get("link_with_several_senders")
    assert r["packets_dropped"][0] > 0 and r["generated"].min() > 10
    r = get("auto_terminating_run")                        # the fault Events of 6 s, 7 s and 8 s do not keep the run alive
    assert r["final_ns"] < 6 * 10 ** 9 and r["pending_events"] == 3 and r["by_kind"][17:19].tolist() == [2, 1], (r["final_ns"], r["pending_events"], r["by_kind"][17:19])
    assert r["link_active_fault"].tolist() == [[-1, 1]] and r["packets_dropped"][0] == 1
    r = get("schedule_that_mixes_crash_pause_and_both_link_faults")
    assert r["by_kind"][17:19].tolist() == [6, 6] and r["packets_dropped"][1] > 0 and r["cl_stats"][0, 2] > 0
    r = get("bidirectional_link_whose_reverse_copy_takes_no_traffic")
    assert r["traffic_routes"] == [["net0", "link0", "srv0"], ["net0", "srv0", "link0"]] and r["traffic_matrix"][1].tolist() == [0, 0, 0] < r["traffic_matrix"][0].tolist()
    r = get("extra_latency_of_zero")                       # Duration.from_seconds over the sum moves the base by a nanosecond
    assert r["sink_latency_s"].tobytes() != bare("extra_latency_of_zero")["sink_latency_s"].tobytes()
    for c in cases.values():
        assert (c["network_counters"] == 0).all()
    assert len(LS.FIXTURES) >= 24 and len(LS.TRACED) >= 6 and LS.N_RANDOM >= 100
    LS.LINK_FAULTS.write(cases)


if __name__ == "__main__":
    main()
