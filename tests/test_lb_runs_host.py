"""CPU: the sizes tests/test_gpu_lb_runs.py crosses, pinned on the source text, and the sort plan's place in the ABI.  No GPU."""
import os
import re

from happy_simulator_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_load_balancer_sorts_tiles_and_windows_are_the_sizes_the_gpu_tests_cross():
    """tests/test_gpu_lb_runs.py makes runs longer than the halo and the tile of the run fix-up kernels (it reads both from
    hs_lb_sort_plan) and radix passes of more than 2 * W + 1 tiles of 4 096 elements (held as literals there): when one of them
    moves, this test fails instead of those cases silently crossing nothing."""
    lb = open(os.path.join(N.CSRC, "hs_lb.hip")).read()
    radix = open(os.path.join(N.CSRC, "hs_radix.hpp")).read()
    assert "constexpr int kSegTile = 1024, kSegHalo = 32;" in lb
    assert lb.count("__shared__ uint64_t lk[kSegTile + 2 * kSegHalo];") == 3           # segments, rr_assign, sink_finish stage the same window
    assert "out[4] = kSegTile; out[5] = kSegHalo;" in lb                                # ... and the plan reports these two
    assert "constexpr int kLbQCap = 60;" in lb              # bursts_one_client under debug flag 2 queues 56 arrivals of one nanosecond
    threads = int(re.search(r"constexpr int kRadixThreads = (\d+);", radix).group(1))
    items = int(re.search(r"constexpr int kRadixItems = (\d+);", radix).group(1))
    assert "constexpr int kRadixTile = kRadixThreads * kRadixItems;" in radix and threads * items == 4096
    assert "constexpr int kRadixBits = 8;" in radix                                    # (hs_lb_latency_stats skips tb % 8 bits)
    assert radix.count("constexpr int W = 16;") == 1 and "t -= used;" in radix         # the look-back window
    import test_gpu_lb_runs as T

    assert (T.K_RADIX_TILE, T.K_LOOK_BACK_W) == (4096, 16)


def test_the_sort_plan_is_declared_bound_and_read_only():
    hdr = open(os.path.join(ROOT, "include", "hs_engine.h")).read()
    assert "int hs_lb_sort_plan(const hs_lb *h, int32_t out[6]);" in hdr               # const handle: it reports, it sets nothing
    assert "hs_lb_sort_plan" in N.EXPORTED_SYMBOLS
    assert N.LB_RUN_DENSE == 1 << 6 and re.search(r"#define HS_LB_RUN_DENSE\s+\(1 << 6\)", hdr)
    lib = N.build() and N.lib()
    assert lib.hs_lb_sort_plan(None, None) == N.HS_E_INVALID
