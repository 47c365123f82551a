"""CPU: the table of tests/uniform_cases.py is what it says it is.  Every condition a load is in the table for is computed from the
oracle's own result of that case, not from constants: a changed seed, span or size that empties a condition fails here, on a
machine without a GPU, instead of leaving tests/test_gpu_uniform_kernels_oracle.py green and vacuous."""
import numpy as np
import pytest

import uniform_cases as U


def _load(rate, mean, span_s, then=False):
    (ld,) = [x for x in U.LOADS if (x.rate, x.mean, x.span_ns) == (rate, mean, int(span_s * 1e9)) and (x.then_ns is not None) == then]
    return ld


def _first(n, start, ld):
    return U.expected(n, start, ld, (start + ld.span_ns,))


def test_table_is_the_one_the_kernels_need():
    assert U.SIZES == (1, 17, 63, 64, 65, 513, 1025) and U.STARTS == (0, 17, 1_500_000_000)
    assert len(U.LOADS) == 10
    assert [len(U.loads_for(n)) for n in U.SIZES] == [8, 10, 8, 8, 10, 8, 8]
    # every value is one of the wave sweep's own (tests/test_gpu_wide.py)
    for ld in U.LOADS:
        assert ld.rate in (0.002, 0.05, 0.7, 3.0, 8.0, 20.0, 60.0) and ld.mean in (0.001, 0.02, 0.1, 0.3, 0.8)
        assert ld.span_ns in (20_000_000, 300_000_000, 2_000_000_000, 7_000_000_000, 40_000_000_000)
        for start in U.STARTS:
            shapes = ld.shapes(start)
            assert shapes[0][1] == (start + ld.span_ns,)
            seconds = [ends[1] for _, ends in shapes[1:]]
            if ld.then_ns is None:
                assert seconds == [start + ld.span_ns * 13 // 10, start + 2 * ld.span_ns]
            else:
                assert seconds == [start + 2_000_000_000]
            assert all(ends[-1] < (1 << 39) for _, ends in shapes)           # (the wave kernel's horizon gate)
    assert [(nm, hex(f)) for nm, f in U.variants()] == [
        ("one lane per LP", "0x400000"), ("4 lanes per LP", "0x3000000"), ("8 lanes per LP", "0x4000000"), ("16 lanes per LP", "0x5000000"),
        ("a wavefront per LP, 16 per workgroup", "0x7000000"), ("a wavefront per LP, 8 per workgroup", "0x8000000"),
        ("a wavefront per LP, 16 per workgroup, reset kernel + loading instantiation", "0x27000000")]


@pytest.mark.parametrize("start", U.STARTS)
def test_most_lps_of_the_slowest_load_see_no_tick(start):
    ld = _load(0.002, 0.1, 40)
    for n in U.SIZES:
        if n >= 17:
            idle = int((_first(n, start, ld)["generated"] == 0).sum())
            assert 2 * idle >= n and idle < n, (n, idle)       # (and not all of them: somebody runs the request loop)
    ld = _load(8.0, 0.1, 0.02, then=True)
    for n in U.SIZES:
        if n >= 17:
            w = _first(n, start, ld)
            assert 2 * int((w["generated"] == 0).sum()) >= n and w["generated"].sum() > 0, n
            assert U.expected(n, start, ld, ld.shapes(start)[1][1])["completed"].min() >= 1      # ... and everybody works in window two


@pytest.mark.parametrize("start", U.STARTS)
def test_the_overloaded_load_enters_window_two_with_requests_waiting_everywhere(start):
    ld = _load(20.0, 0.3, 2)
    for n in U.SIZES:
        w = _first(n, start, ld)
        assert (w["queue_depth"] > 0).all() and (w["active"] == 1).all(), n


@pytest.mark.parametrize("start", U.STARTS)
def test_the_long_loads_need_several_steps_of_the_wave_kernel(start):
    for mean in (0.02, 0.001):
        ld = _load(60.0, mean, 7)
        assert ld.sizes == (17, 65)
        for n in ld.sizes:
            assert _first(n, start, ld)["generated"].min() > 256, (n, mean)        # (a step is 128 requests)


@pytest.mark.parametrize("start", U.STARTS)
def test_the_light_load_ends_with_requests_in_service_and_nobody_waiting(start):
    ld = _load(60.0, 0.001, 0.3)
    for n in U.SIZES:
        w = _first(n, start, ld)
        assert (w["queue_depth"] == 0).all(), (n, int((w["queue_depth"] > 0).sum()))
        if n >= 17:
            assert (w["active"] == 1).any(), n


def test_windows_do_not_change_what_the_oracle_computes():
    """_execute_until per window on one heap == one run to the last end (the property the two-window cases rest on)."""
    ld = _load(20.0, 0.3, 2)
    for start in U.STARTS:
        name, ends = ld.shapes(start)[2]
        two = U.expected(65, start, ld, ends)
        one = U.oracle_outputs(65, U.oracle_run(65, ld.rate, ld.mean, ends[-1:], start, ld.seed))
        assert U.differences(two, one) == []
        assert two["tot_final"] > ends[-1] and two["sink_t"].min() > start


@pytest.mark.parametrize("rate,mean", U.RING_LOADS)
@pytest.mark.parametrize("start", U.RING_STARTS)
def test_ring_windows_begin_at_every_slot_of_both_rings(rate, mean, start):
    """The 16 windows of the ring-position case begin, across 64 LPs, at all 24 ring slots -- and so at all 8 refill offsets --
    of the arrival and of the service stream (the base load; the overloaded one is measured, it is there for its waiting requests)."""
    seen_a, seen_s = {int(1 % U.RING)}, {0}                 # window one: arrival 0 drawn by the bootstrap, no service drawn
    waiting = 0
    for k in range(len(U.ring_ends(start)) - 1):            # the state after window k is where window k + 1 begins
        w = U.ring_expected(rate, mean, start, k)
        a, s = U.stream_positions(w)
        seen_a |= set((a % U.RING).tolist())
        seen_s |= set((s % U.RING).tolist())
        waiting += int((w["queue_depth"] > 0).sum())
    if (rate, mean) == U.RING_LOADS[0]:
        assert len(seen_a) == U.RING and len(seen_s) == U.RING, (sorted(seen_a), sorted(seen_s))
        assert {x % U.REFILL for x in seen_a} == set(range(U.REFILL)) == {x % U.REFILL for x in seen_s}
    else:
        assert waiting >= 64 * 14                            # lanes enter (almost) every window with requests waiting


@pytest.mark.parametrize("n", U.GROUP_SIZES)
@pytest.mark.parametrize("start", U.GROUP_STARTS)
def test_most_windows_of_the_group_case_end_inside_a_tick_group(n, start):
    """... so that the next window begins by finishing that group: Request -> idle worker -> a service draw in event order."""
    inside = sum(int(U.inside_a_tick_group_of_an_idle_server(U.group_expected(n, start, k)).sum()) for k in range(U.GROUP_WINDOWS - 1))
    assert inside >= (U.GROUP_WINDOWS - 1) * 3 // 4, inside
    assert U.group_expected(n, start, U.GROUP_WINDOWS - 1)["completed"].min() > 256


def test_differences_and_verdict_name_the_field_and_the_side():
    ld = _load(8.0, 0.1, 2)
    want = _first(17, 0, ld)
    assert U.differences(want, want) == [] and U.first_difference(want, want) is None
    bad = dict(want)
    bad["total_service_bits"] = want["total_service_bits"].copy()
    bad["total_service_bits"][5] += 1                        # one ulp in one LP
    d = U.differences(bad, want)
    assert [k for k, _ in d] == ["total_service_bits"] and "LP 5" in d[0][1]
    short = dict(want, sink_t=want["sink_t"][:-1])
    assert "sink_t" in U.first_difference(short, want)
    v = U.verdict(want, "left", bad, "right", want)
    assert "left EQUALS the oracle" in v and "right DIFFERS from the oracle in ['total_service_bits']" in v
    with pytest.raises(ValueError):
        want["generated"][0] = 1                             # shared expectations are read-only
