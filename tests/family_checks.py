"""What the GPU tests of the recorded families (test_gpu_{lb_strategies,rate_limiter,faults,health,resilience,client}.py) share: the
comparison of the product's results with a recording, of two runs of the product with each other, a GraphEngine of a spec driven by
hand, and the rows of a recorded trace that left something in the engine's record log.  Nothing here needs a GPU to import;
tests/test_family_checks_host.py shows on the recordings themselves that `compare` sees every kind of difference."""
import numpy as np

import graph_family as GF
import happy_simulator_amd as hs
from happy_simulator_amd import _native as N
from happy_simulator_amd.graph_engine import GraphEngine

FAULT_ON, FAULT_OFF = N.EV_KINDS + 2, N.EV_KINDS + 3          # trace kinds 17 / 18: a crash or pause, a restart or resume


def compare(name, got, ref, not_compared, by_kind_slices):
    """`got` (the product's results of case `name`) against the recording `ref`, exactly: every recorded key outside `not_compared`
    -- float64 arrays in dtype, shape and bytes (so -0.0 is not 0.0), other arrays element for element, scalars by == -- and a
    recorded key that `got` does not hold is an error.  `by_kind_slices` = [(key of got, or a function of got, end)]: the parts
    that tile the recording's by_kind from 0 to its length, each slice starting where the last one ended (the engine reports the
    public kinds in by_kind and the internal ones per graph).  Together they count every processed event: total_events is their sum."""
    for key, want in ref.items():
        if key in not_compared:
            continue
        assert key in got, (name, key, "recorded, but not among the product's results")
        have = got[key]
        if isinstance(want, np.ndarray):
            have = np.asarray(have)
            if want.dtype == np.float64:
                assert have.dtype == np.float64 and have.shape == want.shape and have.tobytes() == want.tobytes(), (
                    name, key, have.tolist()[:16], want.tolist()[:16])
            else:
                assert np.array_equal(have, want), (name, key, have.tolist()[:16], want.tolist()[:16])
        else:
            assert have == want, (name, key, have, want)
    first, total = 0, 0
    for part, end in by_kind_slices:
        have = np.asarray(got[part] if isinstance(part, str) else part(got))
        np.testing.assert_array_equal(have, ref["by_kind"][first:end], err_msg=f"{name}: by_kind[{first}:{end}]")
        first, total = end, total + int(have.sum())
    assert first == len(ref["by_kind"]), (name, first, len(ref["by_kind"]))
    # the event identity: the internal kinds count in events_processed, not in events_by_kind
    assert got["total_events"] == total, (name, got["total_events"], total)


def same(got, one, where=""):
    """Two results of the product: the same keys, every value equal."""
    assert set(got) == set(one)
    for key in one:
        assert np.array_equal(np.asarray(got[key]), np.asarray(one[key])), (where, key)


def engine(spec, **caps):
    """The spec on a GraphEngine of its own (not yet run), with its faults and its scheduled Events, as Simulation.run() sets it up."""
    sim, pools = GF.build(spec)
    g = sim.lowered()
    end_ns, start_ns, sched, cancelled = sim._general_prepare(g, bool(spec.get("auto")))
    eng = GraphEngine(g.arrays, seed=spec["seed"], start_ns=start_ns, **caps)
    for node, t, on, c in sim._general_faults(g):
        eng.add_fault(node, t, on, c)
    for entry in sched:
        eng.schedule(*entry)
    return sim, pools, g, eng, end_ns, start_ns, cancelled


def engine_run(spec, ends_s, flags=0, read=None, **caps):
    """engine(spec), run to every end of `ends_s` in turn; the results bound like Simulation.run() binds them.  `read(eng, g)` is
    called before the engine is closed; (sim, pools, what it returned)."""
    sim, pools, g, eng, end_ns, start_ns, cancelled = engine(spec, **caps)
    with eng:
        if flags:
            eng.set_debug_flags(flags)
        for t in ends_s:
            eng.run_until(start_ns + hs.Instant.from_seconds(t).nanoseconds)
        extra = read(eng, g) if read else None
        sim._general_finish(g, eng, end_ns, cancelled, 0.0)
    return sim, pools, extra


def live_rows(trace, kinds=(N.EV_NAMES.index("sink"),)):
    """The rows of a recorded trace (time ns, kind, node, sort index) of `kinds` whose node was not crashed or paused when they were
    popped -- the fault flag replayed along the trace: an Event the reference popped at a crashed target produced nothing."""
    crashed, keep = set(), []
    for row in trace:
        if row[1] == FAULT_ON:
            crashed.add(int(row[2]))
        elif row[1] == FAULT_OFF:
            crashed.discard(int(row[2]))
        keep.append(row[1] in kinds and int(row[2]) not in crashed)
    return trace[np.array(keep, bool)]
