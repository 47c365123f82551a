"""GPU: every kernel a uniform grid can run on, each ALONE against the C oracle, on the table of tests/uniform_cases.py.

tests/test_gpu_wide.py compares these kernels with one another (hs_station_wave and hs_station_wide against the one-lane
hs_station_run<1, false, true, true>), so a difference there blames nobody, and a forced kernel that is silently not taken
compares the one-lane kernel with itself.  Here the reference is always the oracle -- summary totals and `final_time_ns`, the
per-kind histogram, every per-LP statistic (`total_service_s` bit for bit), every Sink record's time and `created_at` -- and
`run_path()` is asserted after every window: the forced kernel in window one, the one-lane kernel in every later one (an engine
that has run is no longer fresh).  A failure names the load, the kernel, the window shape and the first differing field and LP.

1. the table: sizes x starts, all loads x kernels x window shapes in one id;
2. the one-lane kernel's LDS rings: windows that begin at every ring slot and refill offset of both streams, and windows that
   begin inside the group the election stopped in;
3. repeatability: the same run ten times in one process between engines of other sizes, and once more in fresh processes whose
   device allocations are poisoned (HS_POISON_ALLOC)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import uniform_cases as U

pytestmark = pytest.mark.gpu


# ---- 1. the table
@pytest.mark.parametrize("start", U.STARTS)
@pytest.mark.parametrize("n", U.SIZES)
def test_every_kernel_alone_against_the_oracle(n, start):
    bad, runs = [], 0
    for ld in U.loads_for(n):
        for shape, ends in ld.shapes(start):
            want = U.expected(n, start, ld, ends)
            for vname, flags in U.variants():
                got = U.run_engine(n, ld.rate, ld.mean, ends, start, ld.seed, flags)
                runs += 1
                d = U.differences(got, want)
                if d:
                    bad.append(f"{ld.name}, {vname}, {shape}: differs in {[k for k, _ in d]}: {d[0][1]}")
    assert runs == len(U.loads_for(n)) * 7 * 3 - 7            # (the continued load has two shapes)
    assert not bad, f"{len(bad)} of {runs} runs differ from the oracle:\n" + "\n".join(bad[:24])


# ---- 2. ring positions of the one-lane kernel
@pytest.mark.parametrize("rate,mean", U.RING_LOADS, ids=["base", "overloaded"])
@pytest.mark.parametrize("start", U.RING_STARTS)
def test_one_lane_kernel_windows_begin_at_every_ring_slot(start, rate, mean):
    """16 windows on 64 LPs.  After every window the per-LP statistics equal an oracle run of the same prefix of windows; the
    windows began at all 24 slots (so at all 8 refill offsets) of both rings -- computed from what the ENGINE reports; at the
    end everything is compared.  The overloaded load is there for lanes that enter a window with requests waiting (they leave
    the lean body); its coverage is whatever its counts give."""
    ends = U.ring_ends(start)
    seen = np.zeros((2, U.RING), bool)
    seen[0, 1 % U.RING] = seen[1, 0] = True                    # window one: the bootstrap drew arrival 0, no service drawn yet
    bad = []

    def after(i, eng):
        got = U.engine_lp_outputs(eng)
        d = U.differences(got, U.ring_expected(rate, mean, start, i))
        if d:
            bad.append(f"after window {i} (end {ends[i]}): differs in {[k for k, _ in d]}: {d[0][1]}")
        if i + 1 < len(ends):
            arr_k, svc_k = U.stream_positions(got)
            seen[0, arr_k % U.RING] = True
            seen[1, svc_k % U.RING] = True

    got = U.run_engine(U.RING_LPS, rate, mean, ends, start, U.RING_SEED, U.ONE_LANE, each_window=after)
    d = U.differences(got, U.ring_expected(rate, mean, start, len(ends) - 1))
    if d:
        bad.append(f"at the end: differs in {[k for k, _ in d]}: {d[0][1]}")
    assert not bad, "\n".join(bad)
    if (rate, mean) == U.RING_LOADS[0]:
        assert seen.all(), f"windows began at arrival slots {np.flatnonzero(seen[0]).tolist()}, service slots {np.flatnonzero(seen[1]).tolist()} only"


@pytest.mark.parametrize("n", U.GROUP_SIZES)
@pytest.mark.parametrize("start", U.GROUP_STARTS)
def test_one_lane_kernel_windows_begin_inside_the_elected_group(start, n):
    """400 windows on one (and on three) light LPs: nearly every window ends with the election of an idle Server's tick, so the next
    begins by finishing that group in event order -- the consumer lane draws a service time through its own LDS columns while the
    producer wavefront is already running.  (The producer used to refill those columns by draw index under that lane: now and
    then the lane popped another draw's value -- a wrong departure and `total_service_s` in one LP, nondeterministically; this
    test then failed in at least one of its ids in each of three runs.)"""
    ends = U.group_ends(start)
    bad = []

    def after(i, eng):
        if len(bad) < 8:
            d = U.differences(U.engine_lp_outputs(eng), U.group_expected(n, start, i))
            if d:
                bad.append(f"after window {i} (end {ends[i]}): differs in {[k for k, _ in d]}: {d[0][1]}")

    got = U.run_engine(n, U.GROUP_RATE, U.GROUP_MEAN, ends, start, U.GROUP_SEED, U.ONE_LANE, each_window=after)
    d = U.differences(got, U.group_expected(n, start, len(ends) - 1))
    if d:
        bad.append(f"at the end: differs in {[k for k, _ in d]}: {d[0][1]}")
    assert not bad, "\n".join(bad)


# ---- 3. repeatability
@pytest.mark.parametrize("which", range(len(U.REPEAT_LOADS)), ids=["base", "overloaded"])
def test_repeated_runs_in_one_process_equal_the_oracle(which):
    runs, bad = U.repeat_sequence(which, repeats=10)
    assert runs == 70
    assert not bad, f"{len(bad)} of {runs} runs differ from the oracle:\n" + "\n".join(bad[:24])


@pytest.mark.parametrize("poison", ["0xAB", "0xFF"])
def test_nothing_depends_on_what_the_allocator_hands_out(poison):
    """HS_POISON_ALLOC (csrc/hs_host.hpp dev_alloc): every device allocation filled with that byte before use, in a fresh process so
    that the poison is what the engines see (tools/uniform_seq.py: the sequences of the test above)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "uniform_seq.py"), "10"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HS_POISON_ALLOC=poison))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "n = 140 bad = 0" in r.stdout, r.stdout[-3000:]
