"""CPU: the set-up plan (csrc/hs_plan.hpp, host only) sends a grid to the uniform-kind kernel -- which divides by the rate and by
lambda = 1 / mean with the multiply + FMA sequence and does not test the divisor (csrc/hs_device.hpp const_div_fast) -- only if every
LP's two divisors are ones the sequence is exact for.  A divisor with an all-ones significand is not; such a grid runs on the
generic one-lane kernel, which keeps the test (tests/test_gpu_grid_interior.py compares its results with the oracle).

The plan needs no device, so a small host program is compiled against the header and run here."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROGRAM = r"""
#include "hs_plan.hpp"
#include <cstdio>
#include <cstdlib>
// argv: pairs of (rate, mean) as hexadecimal floats; prints "<rc> <uni_grid>" per pair for a 64-LP Poisson -> Exp -> Sink grid
int main(int argc, char **argv) {
    const int n = 64;
    for (int a = 1; a + 1 < argc; a += 2) {
        std::vector<double> rate(n, strtod(argv[a], nullptr)), mean(n, strtod(argv[a + 1], nullptr));
        std::vector<uint8_t> sk(n, (uint8_t)HS_SRC_POISSON), vk(n, (uint8_t)HS_LAT_EXPONENTIAL), eg(n, (uint8_t)HS_EGRESS_SINK);
        hs_config cfg{};
        cfg.struct_size = sizeof cfg; cfg.n_lp = n; cfg.mode = HS_MODE_SINGLE; cfg.horizon_ns = 5000000000ll; cfg.seed = 42;
        hs_stations st{};
        st.src_kind = sk.data(); st.src_rate = rate.data(); st.svc_kind = vk.data(); st.svc_mean_s = mean.data(); st.egress = eg.data();
        hs::StationPlan p;
        std::string err;
        const int rc = hs::plan_stations(cfg, st, p, err);
        std::printf("%d %d\n", rc, (int)p.uni_grid);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    from happy_simulator_amd import _native as N

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to compile the plan for the host"
    d = tmp_path_factory.mktemp("uni_gate")
    src, exe = d / "plan_main.hip", d / "plan_main"
    src.write_text(PROGRAM)
    subprocess.run([hipcc, "--cuda-host-only", "-O1", "-std=c++17", "-I", N.CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=300)
    return str(exe)


def _uni_grid(exe, pairs):
    args = [x.hex() for pair in pairs for x in pair]
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    rows = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(len(pairs))]
    assert all(rc == 0 for rc, _ in rows), rows
    return [bool(u) for _, u in rows]


def test_reciprocals_never_have_an_all_ones_significand():
    """Why the lambda case below uses the exponent clause: RN(1 / m) = 2^k (2 - 2^-52) would need m = 2^-(k+1) (1 + j 2^-52) with
    0.25 < j < 0.75, and j is a whole number.  The nearest candidates on either side show it."""
    ones = float(np.nextafter(2.0, 0.0))
    for m in (0.5, float(np.nextafter(0.5, 1.0))):
        assert 1.0 / m != ones
    assert 1.0 / 0.5 > ones > 1.0 / float(np.nextafter(0.5, 1.0))


def test_divisors_the_sequence_is_not_exact_for_leave_the_uniform_kernel(plan_program):
    ones = float(np.nextafter(2.0, 0.0))                      # a rate whose significand is all ones
    assert np.float64(ones).view(np.uint64) & np.uint64((1 << 52) - 1) == np.uint64((1 << 52) - 1)
    tiny = 2.0 ** -201                                        # lambda = 2^201: outside the exponents the sequence stays normal for
    got = _uni_grid(plan_program, [(8.0, 0.1), (ones, 0.1), (8.0, tiny), (ones, tiny), (float(np.nextafter(ones, 0.0)), 0.1),
                                   (8.0, 2.0 ** -198)])
    assert got == [True, False, False, False, True, True]
