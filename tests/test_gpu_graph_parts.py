"""GPU: the device's part-run rule (csrc/hs_graph.hip hs_graph_run_parts) held to the CPU model of it (tests/part_model.py), in both
directions, on the pinned random_specs.part_order_spec seeds: a Simulation the model calls undecided runs on ONE heap, one it calls
decided runs as parts -- and either way every statistic, Sink record, Probe sample, the total and the final time == the oracle's one
heap.  The class-(A) seeds are Requests schedule()d on a busy Server whose WORK shares a nanosecond with a tick or a completion: the
device decides them only by the origin the Request carries through the queue."""
import numpy as np
import pytest

import graph_specs as GS
import helpers as H
import part_model as PM
from happy_simulator_amd.graph_engine import GeneralGraph, GraphEngine, PartRun, split_parts
from oracle import hs_oracle as O
from random_specs import part_order_spec
from test_gpu_graph import _compare_with_oracle

pytestmark = pytest.mark.gpu


def _oracle(spec):
    g_o, nodes = H.oracle_graph(spec)
    return O.run(g_o, H.ns_from_seconds(spec["end_s"]), seed=spec["seed"], schedule=H.oracle_graph_schedule(spec, nodes)), nodes


@pytest.mark.parametrize("cls,k", [(cls, k) for cls in "ABCDE" for k in PM.PINNED[cls]])
def test_pinned_part_order_cases_match_the_model_and_the_oracle(cls, k):
    spec = part_order_spec(k)
    model = PM.spec_model(spec)[0]
    sim, ents = GS.build(spec)
    assert isinstance(sim.lowered(), GeneralGraph)
    r, nodes = _oracle(spec)
    sim.run()
    _compare_with_oracle(spec, sim, ents, r, nodes)
    for (pr, data), nd in zip(ents["probes"], nodes["probe"]):
        t, v = r.sinks[nd]
        np.testing.assert_array_equal(data._t_ns, t, err_msg=pr.name)
        np.testing.assert_array_equal(data._v, v, err_msg=pr.name)
    if model.decided:
        assert sim._graph_parts == model.n_parts >= 2, (sim._graph_parts, model)
    else:
        assert sim._graph_parts == 1, (sim._graph_parts, model)


def test_a_part_run_hands_a_queued_scheduled_request_back_to_one_heap():
    """PartRun.run directly on a class-(A) seed: the WORK of a queued schedule()d Request meets an event of the run on its nanosecond,
    so hs_graph_run_parts reports the run undecided (False) instead of answering."""
    spec = part_order_spec(PM.PINNED["A"][0])
    sim, _ = GS.build(spec)
    g = sim.lowered()
    assert isinstance(g, GeneralGraph)
    end_ns, start_ns, sched, _cancelled = sim._general_prepare(g, False)
    parts = split_parts(g.arrays)
    assert parts is not None and len(parts) >= 2
    part_of = np.empty(g.arrays.n, np.int64)
    local = np.empty(g.arrays.n, np.int64)
    for p, (ids, _pos, _b) in enumerate(parts):
        part_of[ids] = p
        local[ids] = np.arange(len(ids))
    engines = [GraphEngine(b, seed=spec["seed"], start_ns=start_ns, record_capacity=4096) for _ids, _pos, b in parts]
    with PartRun(g.arrays, parts, engines) as run:
        for node, t in sched:
            engines[int(part_of[node])].schedule(int(local[node]), t)
        assert run.run(end_ns) is False
