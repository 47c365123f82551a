"""A CPU model of a Simulation run as parts (csrc/hs_graph.hip hs_graph_run_parts, graph_engine.split_parts / PartRun): the oracle on
the whole Simulation, and the oracle on every connected component alone, the way the device runs one heap per part.

A part graph keeps every node's parameters and stream base, the relative list order of its Sources and Probes, and its own
`schedule()` calls in call order -- so the oracle on a part alone computes what a correct device heap for that part computes
(every draw is keyed by (seed, stream base, draw count): equal traces mean equal results).  With hso_params.part_check the oracle
also applies the device's rule: it stops in front of the first event beyond the end, steps over it only in the part that holds
the earliest such event, and flags the first pop that meets a pair of one nanosecond whose sort indices come from different
counters.  The composition then elects across parts exactly as hs_graph_run_parts does (a tie between parts: undecided).

`run_model` says whether the device would take the parts' answer ("decided") and whether that answer is the whole Simulation's
(`sensitive`: some part orders its own events differently inside the union).  tests/test_graph_parts_host.py holds the device's
rule to the second; tests/test_gpu_graph_parts.py holds the device to the first.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import helpers as H
from oracle import hs_oracle as O

RULE = 1               # hso_params.part_check: the device's rule, origins carried through the queue (hs_graph.hip)
RULE_NO_WORK_ORIGIN = 2   # ... with every WORK event counted as the run's own (the device before it carried the origin)
TRACE_CAP = 1 << 21

_STATS = ("generated", "accepted", "dropped", "completed", "rejected", "total_service_s", "received", "depth", "active",
          "packets_sent", "routed")
_PER_NODE = [f.name for f in dataclasses.fields(O.Graph) if f.name not in ("rt_targets",)]

# Pinned part_order_spec seeds per class (tests/test_graph_parts_host.py asserts they keep their class; tests/test_gpu_graph_parts.py
# runs them).  The class-(A) seeds are the ones whose WORK origin decides: without it the rule would take the parts' answer, and that
# answer differs from the one heap in a Sink record or a drop count.
PINNED = {
    "A": [1805, 655, 440, 205, 1570],
    "B": [676, 236, 501],
    "C": [1422, 1377, 1752],
    "D": [1818, 383, 518],
    "E": [1339, 525, 1650],
}


def components(g: O.Graph) -> list:
    """Connected components of the oracle graph (a Request can cross target / router / load-balancer edges; a Probe hangs on its
    target), as ascending node-id arrays ordered by their first node -- graph_engine.split_parts' order."""
    n = len(g)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)

    for i in range(n):
        if g.target[i] >= 0:
            union(i, g.target[i])
        if g.kind[i] in (O.ROUTER, O.LB):
            for t in g.rt_targets[g.rt_off[i]:g.rt_off[i] + g.rt_cnt[i]]:
                union(i, t)
    groups: dict = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    return [np.asarray(v, np.int64) for _, v in sorted(groups.items(), key=lambda kv: kv[1][0])]


def sub_graph(g: O.Graph, ids) -> O.Graph:
    """The part of `g` on nodes `ids` (ascending): parameters, stream bases and names kept, edges renumbered."""
    local = {int(i): j for j, i in enumerate(ids)}
    b = O.Graph()
    for nm in _PER_NODE:
        col = getattr(g, nm)
        setattr(b, nm, [col[i] for i in ids])
    b.target = [local[t] if t >= 0 else -1 for t in b.target]
    b.rt_off = []
    for i in ids:
        b.rt_off.append(len(b.rt_targets))
        b.rt_targets.extend(local[t] for t in g.rt_targets[g.rt_off[i]:g.rt_off[i] + g.rt_cnt[i]])
    return b


@dataclasses.dataclass
class Model:
    decided: bool              # the device's rule takes the parts' answer
    sensitive: bool            # some part orders its own events differently inside the whole Simulation
    visible: bool              # ... and the parts' answer differs in a Sink record, a Probe sample or a drop count
    results_equal: bool        # the parts' composed results == the whole Simulation's (every statistic, record, total)
    n_parts: int
    flag: dict | None          # a part's first flagged pop, dict(part, pop, ns, kinds, pre) (hs_oracle.run part_check): the one of the
                               # first class below among the parts' first flags
    tie: bool                  # the earliest first events beyond the end of two parts share a nanosecond
    cls: str                   # "A" WORK of a schedule()d Request | "B" a first tick | "C" a schedule()d Event | "D" tie | "E" decided
    bad_parts: list            # parts whose trace differs from the whole Simulation's


def _classify(flag, tie) -> str:
    if flag is None:
        return "D" if tie else "E"
    pairs = list(zip(flag["kinds"], flag["pre"]))
    if any(k == 5 and p for k, p in pairs):                  # HSO_EV_WORK with a pre-run index
        return "A"
    if any(k in (0, 13) and p for k, p in pairs):            # HSO_EV_SOURCE / HSO_EV_PROBE_TICK: a first tick
        return "B"
    return "C"


def run_model(g: O.Graph, schedule, end_ns: int, seed: int, rule: int = RULE, union=None) -> Model:
    """The whole Simulation (`union`: a finished hs_oracle.run with trace, or None to run it) against its parts under `rule`."""
    if union is None:
        union = O.run(g, end_ns, seed=seed, schedule=schedule, trace_cap=TRACE_CAP)
    assert len(union.trace[0]) < TRACE_CAP
    comps = components(g)
    n = len(g)
    part_of = np.empty(n, np.int64)
    local = np.empty(n, np.int64)
    for p, ids in enumerate(comps):
        part_of[ids] = p
        local[ids] = np.arange(len(ids))
    subs, scheds, runs = [], [], []
    for p, ids in enumerate(comps):
        subs.append(sub_graph(g, ids))
        scheds.append([(int(local[nd]), t) for nd, t in schedule if part_of[nd] == p])
        runs.append(O.run(subs[p], end_ns, seed=seed, schedule=scheds[p], trace_cap=TRACE_CAP, part_check=rule))
    # hs_graph_run_parts: the earliest first event beyond the end is processed, in its own part, and nothing else
    best, tie = -1, False
    for p, r in enumerate(runs):
        if r.next_ns is None:
            continue
        if best < 0 or r.next_ns < runs[best].next_ns:
            best, tie = p, False
        elif r.next_ns == runs[best].next_ns:
            tie = True
    if best >= 0 and not tie:
        runs[best] = O.run(subs[best], end_ns, seed=seed, schedule=scheds[best], trace_cap=TRACE_CAP, part_check=rule, step=True)
    flags = [dict(part=p, **r.part_check) for p, r in enumerate(runs) if r.part_check is not None]
    flag = min(flags, key=lambda f: "ABC".index(_classify(f, False))) if flags else None
    # sensitivity: the union's trace restricted to a part (local ids) against the part's own
    ut, uk, un = union.trace[0], union.trace[1], union.trace[2]
    upart = part_of[un]
    bad = []
    for p, r in enumerate(runs):
        m = upart == p
        a = (ut[m], uk[m], local[un[m]])
        b = r.trace[:3]
        if len(a[0]) != len(b[0]) or any(not np.array_equal(x, y) for x, y in zip(a, b)):
            bad.append(p)
    # the parts' answer, composed as PartRun does it
    eq, vis = True, False
    for nm in _STATS:
        got = np.zeros(n, np.float64 if nm == "total_service_s" else np.int64)
        for ids, r in zip(comps, runs):
            got[ids] = getattr(r, nm)
        if not np.array_equal(got, getattr(union, nm)):
            eq = False
            vis |= nm == "dropped"
    for nd, (t, cr) in union.sinks.items():
        pt, pcr = runs[part_of[nd]].sinks[int(local[nd])]
        if not (np.array_equal(t, pt) and np.array_equal(cr, pcr)):
            eq, vis = False, True
    eq &= sum(r.events_processed for r in runs) == union.events_processed
    eq &= max(r.final_time_ns for r in runs) == union.final_time_ns
    eq &= np.array_equal(np.sum([r.events_by_kind for r in runs], axis=0), union.events_by_kind)
    return Model(decided=flag is None and not tie, sensitive=bool(bad), visible=vis, results_equal=bool(eq), n_parts=len(comps),
                 flag=flag, tie=tie, cls=_classify(flag, tie), bad_parts=bad)


def spec_model(spec, rules=(RULE,)) -> list:
    """run_model on a graph spec (random_specs / graph_specs format, `schedule` and `probes` included), once per rule."""
    g, nodes = H.oracle_graph(spec)
    sched, end_ns = H.oracle_graph_schedule(spec, nodes), H.ns_from_seconds(spec["end_s"])
    union = O.run(g, end_ns, seed=spec["seed"], schedule=sched, trace_cap=TRACE_CAP)
    return [run_model(g, sched, end_ns, spec["seed"], rule=rule, union=union) for rule in rules]
