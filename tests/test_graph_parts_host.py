"""CPU: the exactness argument of part runs (csrc/hs_graph.hip hs_graph_run_parts), on the oracle alone (tests/part_model.py).

A Simulation whose graph falls into disconnected parts runs one heap per part; the device hands the run back to one heap when a
part meets a timestamp group whose order depends on the whole Simulation (a pre-run and a run-time sort index on one nanosecond), or
when two parts' first events beyond the end tie.  Whenever that rule says "decided", every part must order its own events exactly as
the whole Simulation does, and the parts' composed results must be the whole Simulation's.  random_specs.part_order_spec builds the
groups where the argument can break, on purpose; random unions of graph_spec / lb_graph_spec graphs are the background."""
import functools

import numpy as np
import pytest

import part_model as PM
from random_specs import graph_spec, lb_graph_spec, part_order_spec, union_spec

N_PART_ORDER, N_UNIONS = 2000, 500


@functools.lru_cache(maxsize=None)
def _part_order_models():
    out = []
    for k in range(N_PART_ORDER):
        spec = part_order_spec(k)
        out.append((k, spec["part_class"], PM.spec_model(spec)[0]))
    return out


def _random_union(k):
    rng = np.random.default_rng(95_000 + k)
    members = [(lb_graph_spec if rng.random() < 0.5 else graph_spec)(int(rng.integers(0, 5000))) for _ in range(int(rng.integers(2, 6)))]
    spec = union_spec(members, name=f"union_{k}")
    for sc in spec["sources"]:
        sc["rate"] = min(sc["rate"], 4.0)                     # (a short union: the trace of every event stays small)
    spec["end_s"] = min(spec["end_s"], 3.0)
    if k % 2 == 0:                                            # half of them Poisson only, nothing schedule()d: mostly decidable
        spec["schedule"] = []
        for sc in spec["sources"]:
            sc["kind"] = "poisson"
    return spec


def _unsound(rows):
    """(seed, the class part_order_spec built, parts that ordered differently, results equal) of every case decided wrongly"""
    return [(k, want, m.bad_parts, m.results_equal) for k, want, m in rows if m.decided and (m.sensitive or not m.results_equal)]


def test_parts_the_rule_decides_order_their_events_as_the_whole_simulation():
    """part_order_spec: wherever the device's rule takes the parts' answer, every part's trace == the whole Simulation's restricted to
    it (time, kind, node; the one event beyond the end in the part that holds it), and the composed results == the one heap's."""
    bad = _unsound(_part_order_models())
    assert not bad, f"{len(bad)} part_order_spec seeds decided but ordered differently (seed, built class, parts, results equal): {bad[:8]}"


def test_random_unions_the_rule_decides_equal_the_whole_simulation():
    rows = [(k, None, PM.spec_model(_random_union(k))[0]) for k in range(N_UNIONS)]
    bad = _unsound(rows)
    assert not bad, f"{len(bad)} random unions decided but ordered differently (seed, built class, parts, results equal): {bad[:8]}"
    assert sum(m.decided for _, _, m in rows) >= N_UNIONS // 4       # (the background is mostly decidable: the rule is no blanket refusal)


def test_every_hazard_class_occurs():
    """Each class of hazard occurs in numbers: (A) a queued schedule()d Request's WORK on a run-time event's nanosecond, (B) a first
    tick, (C) a schedule()d Event, (D) a tie of parts beyond the end, (E) decided controls -- and the sensitive ones are many."""
    rows = _part_order_models()
    count = {c: sum(m.cls == c for _, _, m in rows) for c in "ABCDE"}
    assert count["A"] >= 120 and count["B"] >= 250 and count["C"] >= 250 and count["D"] >= 250 and count["E"] >= 350, count
    assert sum(m.sensitive for _, _, m in rows) >= 1000
    for cls in "ABCDE":                                        # the generator's intent shows: its k % 5 class lands there
        mine = [m for _, want, m in rows if want == cls]
        assert sum(m.cls == cls for m in mine) >= len(mine) * 2 // 5, cls


def test_without_the_work_origin_the_rule_takes_wrong_answers():
    """The rule as the device had it -- every WORK event counted as the run's own -- accepts sensitive class-(A) cases as decided, some
    with different Sink records or drop counts (what the GPU test sees without a trace).  The origin the Request carries closes it."""
    rows = _part_order_models()
    wrong = []
    for k, _, m in rows:
        if m.cls != "A":
            continue
        old = PM.spec_model(part_order_spec(k), rules=(PM.RULE_NO_WORK_ORIGIN,))[0]
        if old.decided and old.sensitive:
            wrong.append((k, old.visible))
    assert len(wrong) >= 40, wrong
    assert sum(v for _, v in wrong) >= 30, wrong


@pytest.mark.parametrize("cls", "ABCDE")
def test_pinned_seeds_keep_their_class(cls):
    """The seeds tests/test_gpu_graph_parts.py runs: each keeps its class; the class-(A) ones stay visible mistakes of the old rule."""
    for k in PM.PINNED[cls]:
        spec = part_order_spec(k)
        new, old = PM.spec_model(spec, rules=(PM.RULE, PM.RULE_NO_WORK_ORIGIN))
        assert new.cls == cls, (k, new)
        assert new.decided == (cls == "E"), (k, new)
        assert not new.decided or (not new.sensitive and new.results_equal), (k, new)
        if cls == "A":
            assert old.decided and old.sensitive and old.visible, (k, old)
        assert len(spec["sources"]) <= 300                    # (small enough for one GPU test each)
