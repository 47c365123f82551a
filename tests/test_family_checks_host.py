"""family_checks.compare on the recordings themselves (no GPU): one small recorded case per family serves as `ref` and, put into the
form the product reports it in, as `got`.  The unmodified copy passes; every kind of difference that compare is there for makes it
raise; a difference in a key the family does not compare does not.  The families' _NOT_COMPARED sets and by_kind slices are the ones
their GPU tests use, and the sets are pinned here as literals."""
import copy

import numpy as np
import pytest

import client_specs as CS
import family_checks as FC
import fault_specs as FS
import health_specs as HS
import mixed_specs as MX
import rate_limiter_specs as RS
import recorded
import resilience_specs as XS
import strategy_specs as SS
import test_gpu_client
import test_gpu_faults
import test_gpu_health
import test_gpu_lb_strategies
import test_gpu_mixed
import test_gpu_rate_limiter
import test_gpu_resilience
from happy_simulator_amd import _native as N

# family -> (its GPU tests, its recordings, a small case with a 0.0 in a float64 array, what the product reports by_kind[15:] in, the
# set its GPU tests leave out of the key-by-key comparison)
FAMILIES = {
    "strategies": (test_gpu_lb_strategies, recorded.STRATEGIES, SS.FIXTURES["lc_lockstep_constant"], {}, {"trace"}),
    "rate_limiter": (test_gpu_rate_limiter, recorded.RATE_LIMITER, RS.FIXTURES["auto_terminate"], {},
                     {"trace", "by_kind", "pending_events", "lim_guard_hits", "entity_summaries"}),
    "faults": (test_gpu_faults, recorded.FAULTS, FS.FIXTURES["lockstep_tick_grid"], {"internal_by_kind": (15, 19)},
               {"trace", "by_kind", "pending_events", "time_travel"}),
    "health": (test_gpu_health, recorded.HEALTH, HS.FIXTURES["every_backend_marked_unhealthy_without_a_checker"],
               {"internal_by_kind": (15, 19), "health_by_kind": (19, 22)},
               {"trace", "by_kind", "pending_events", "time_travel", "health_events", "probe_drops"}),
    "resilience": (test_gpu_resilience, recorded.RESILIENCE, XS.FIXTURES["bulkhead_limiter_target_leaky"],
                   {"internal_by_kind": (15, 19), "health_by_kind": (19, 22), "resilience_by_kind": (22, 28)},
                   {"trace", "by_kind", "pending_events", "time_travel"}),
    "client": (test_gpu_client, recorded.CLIENT, CS.FIXTURES["retry_lands_after_the_restart"],
               {"internal_by_kind": (15, 19), "health_by_kind": (19, 22), "resilience_by_kind": (22, 28), "client_by_kind": (28, 31)},
               {"trace", "by_kind", "pending_events", "time_travel"}),
    "mixed": (test_gpu_mixed, MX.MIXED, MX.FIXTURES["checked_backends_into_a_processor_a_client_and_a_bulkhead"],
              {"internal_by_kind": (15, 19), "health_by_kind": (19, 22), "resilience_by_kind": (22, 28), "client_by_kind": (28, 31), "flow_by_kind": (31, 39)},
              {"trace", "by_kind", "pending_events", "time_travel", "probe_drops"}),
}


def _case(family):
    """(name, got, ref, not_compared, slices): the recording as `ref`; as `got` a deep copy with by_kind split like the product's."""
    module, store, spec, parts, _literal = FAMILIES[family]
    ref = store.get("case", spec)
    got = copy.deepcopy(ref)
    got["by_kind"] = ref["by_kind"][:N.EV_KINDS].copy()
    for key, (lo, hi) in parts.items():
        got[key] = ref["by_kind"][lo:hi].copy()
    return spec["name"], got, ref, module._NOT_COMPARED, module._BY_KIND_SLICES


def _arrays(ref, not_compared, floating):
    return [k for k, v in ref.items() if k not in not_compared and isinstance(v, np.ndarray) and v.size and (v.dtype == np.float64) == floating]


@pytest.mark.parametrize("family", FAMILIES)
def test_an_unmodified_copy_passes_and_the_set_is_the_literal(family):
    name, got, ref, not_compared, slices = _case(family)
    assert N.EV_KINDS == 15 and not_compared == FAMILIES[family][4]
    assert slices[-1][1] == len(ref["by_kind"]) == {"strategies": 15, "rate_limiter": 17, "faults": 19, "health": 22, "resilience": 28, "client": 31,
                                                        "mixed": 39}[family]
    FC.compare(name, got, ref, not_compared, slices)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_integer_element_changed_raises(family):
    name, got, ref, not_compared, slices = _case(family)
    keys = _arrays(ref, not_compared | {"by_kind"}, floating=False)
    assert len(keys) >= 5
    for key in keys:
        altered = dict(got, **{key: got[key].copy()})
        altered[key].flat[-1] += 1
        with pytest.raises(AssertionError, match=key):
            FC.compare(name, altered, ref, not_compared, slices)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_zero_that_became_a_negative_zero_raises(family):
    """What np.array_equal lets pass: -0.0 == 0.0."""
    name, got, ref, not_compared, slices = _case(family)
    hit = 0
    for key in _arrays(ref, not_compared, floating=True):
        zeros = np.flatnonzero((ref[key] == 0.0) & ~np.signbit(ref[key]))
        if len(zeros):
            altered = dict(got, **{key: got[key].copy()})
            altered[key].flat[zeros[0]] = -0.0
            assert np.array_equal(altered[key], ref[key])
            with pytest.raises(AssertionError, match=key):
                FC.compare(name, altered, ref, not_compared, slices)
            hit += 1
        for other in (got[key].astype(np.float32), got[key].reshape(-1, 1)):           # the dtype and the shape count too
            with pytest.raises(AssertionError, match=key):
                FC.compare(name, dict(got, **{key: other}), ref, not_compared, slices)
    assert hit >= 1


@pytest.mark.parametrize("family", FAMILIES)
def test_one_scalar_changed_raises(family):
    name, got, ref, not_compared, slices = _case(family)
    scalars = [k for k, v in ref.items() if k not in not_compared and not isinstance(v, np.ndarray)]
    assert "final_ns" in scalars and "total_events" in scalars
    for key in scalars:
        with pytest.raises(AssertionError, match=key):
            FC.compare(name, dict(got, **{key: got[key] + 1}), ref, not_compared, slices)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_count_changed_in_each_by_kind_slice_raises(family):
    name, got, ref, not_compared, slices = _case(family)
    first = 0
    for part, end in slices:
        # (the rate limiters' second slice is the column sums of lim_events, the strategies' only one the recorded by_kind as it
        #  is: compared keys of their own, which are found to differ first)
        key = part if isinstance(part, str) else "lim_events"
        altered = dict(got, **{key: got[key].copy()})
        altered[key].flat[0] += 1
        with pytest.raises(AssertionError, match=rf"by_kind\[{first}:{end}\]" if key in not_compared or key not in ref else key):
            FC.compare(name, altered, ref, not_compared, slices)
        first = end
    # a slice left out, and one that ends somewhere else: the slices no longer tile by_kind
    with pytest.raises(AssertionError):
        FC.compare(name, got, ref, not_compared, slices[:-1])
    with pytest.raises(AssertionError):
        FC.compare(name, got, ref, not_compared, slices[:-1] + [(slices[-1][0], slices[-1][1] + 1)])
    # ... and the event identity alone: a count moved between two public kinds leaves every slice's sum, not its content; one event
    # more in total_events and in no kind is caught by the identity
    with pytest.raises(AssertionError):
        FC.compare(name, dict(got, total_events=got["total_events"] + 1), dict(ref, total_events=ref["total_events"] + 1), not_compared, slices)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_recorded_key_removed_from_got_raises(family):
    name, got, ref, not_compared, slices = _case(family)
    compared = [k for k in ref if k not in not_compared]
    assert len(compared) >= 20
    for key in compared:
        without = {k: v for k, v in got.items() if k != key}
        with pytest.raises(AssertionError, match=key):
            FC.compare(name, without, ref, not_compared, slices)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_key_the_family_does_not_compare_may_differ(family):
    name, got, ref, not_compared, slices = _case(family)
    for key in not_compared - {"by_kind"}:            # (by_kind is compared in its own form: the slices)
        assert key in ref or key == "trace", (family, key)
        FC.compare(name, dict(got, **{key: "something else"}), ref, not_compared, slices)
        FC.compare(name, {k: v for k, v in got.items() if k != key}, ref, not_compared, slices)
