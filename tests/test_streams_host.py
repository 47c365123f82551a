"""CPU: the SOURCE TEXT of the stream functions of csrc/hs_device.hpp -- hs_log, exp1_from_uniform, res53, philox4x32_10 and
Stream::init / next_uniform / next2 / next4 -- against the oracle, bit for bit, at the chosen inputs of tests/stream_cases.py.

The header is compiled for the host (g++ -O2 -ffp-contract=off with the stand-in for <hip/hip_runtime.h> of
tools/profile_cost.py, as tools/simpson_split_check.py does) into a stand-alone program that only evaluates: it reads inputs
from a file and writes the raw result bits; the comparison with the oracle's values happens here.  (Comparing hs::hs_log with
hs_log_ref inside one C++ program compares nothing: the compiler folds the two identical functions.)
tests/test_gpu_streams.py asks the same of what hipcc makes of the header, through the hs_debug_log / _philox / _stream_walk hooks.

Also here: the checks that the oracle's array entries are its scalar ones, and the accuracy of the definition itself against
mpmath -- the device inherits that bound through bit equality and gets no tolerance of its own.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hs_streams_py as PY  # noqa: E402
from oracle import hs_oracle as O  # noqa: E402
from profile_cost import HIP_STANDIN  # noqa: E402

CSRC = os.path.join(ROOT, "happy_simulator_amd", "csrc")

MAIN = r"""
#include "hs_device.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace hs;

template <class T> static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T> static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

// every input file starts with two int64: n and (walks only) n_steps
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const char mode = argv[1][0];
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const std::vector<int64_t> head = take<int64_t>(in, 2);
    const size_t n = (size_t)head[0];
    if (mode == 'l') {             // x[n], u[n] -> hs_log(x)[n], exp1_from_uniform(u)[n]
        const std::vector<double> x = take<double>(in, n), u = take<double>(in, n);
        std::vector<double> a(n), b(n);
        for (size_t i = 0; i < n; ++i) { a[i] = hs_log(x[i]); b[i] = exp1_from_uniform(u[i]); }
        put(out, a); put(out, b);
    } else if (mode == 'p') {      // {c0, c1, c2, c3, k0, k1}[n] -> the block[n]
        const std::vector<uint32_t> c = take<uint32_t>(in, 6 * n);
        std::vector<uint32_t> o(4 * n);
        for (size_t i = 0; i < n; ++i) {
            const U4 r = philox4x32_10(c[6 * i], c[6 * i + 1], c[6 * i + 2], c[6 * i + 3], c[6 * i + 4], c[6 * i + 5]);
            o[4 * i] = r.x; o[4 * i + 1] = r.y; o[4 * i + 2] = r.z; o[4 * i + 3] = r.w;
        }
        put(out, o);
    } else if (mode == 'w') {      // seed[n], sid[n], k0[n], steps[n_steps] -> draws[n][sum(steps)], k_end[n]
        const size_t n_steps = (size_t)head[1];
        const std::vector<uint64_t> seed = take<uint64_t>(in, n), sid = take<uint64_t>(in, n), k0 = take<uint64_t>(in, n);
        const std::vector<uint8_t> steps = take<uint8_t>(in, n_steps);
        std::vector<double> draws;
        std::vector<uint64_t> k_end(n);
        for (size_t i = 0; i < n; ++i) {
            Stream s;
            s.init(seed[i], sid[i], k0[i]);
            for (uint8_t st : steps) {
                if (st == 4) { double u[4]; s.next4(u); draws.insert(draws.end(), u, u + 4); }
                else if (st == 2) { double u[2]; s.next2(u); draws.insert(draws.end(), u, u + 2); }
                else if (st == 1) draws.push_back(s.next_uniform());
                else return 2;
            }
            k_end[i] = s.k;
        }
        put(out, draws); put(out, k_end);
    } else return 2;
    return fclose(out) == 0 ? 0 : 2;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """-> run(mode, head, *arrays) -> the bytes the program wrote"""
    d = str(tmp_path_factory.mktemp("streams_host"))
    os.makedirs(os.path.join(d, "hip"))
    with open(os.path.join(d, "hip", "hip_runtime.h"), "w") as f:
        f.write(HIP_STANDIN)
    with open(os.path.join(d, "main.cpp"), "w") as f:
        f.write(MAIN)
    exe = os.path.join(d, "streams_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", d, "-I", CSRC, os.path.join(d, "main.cpp"), "-o", exe])

    def run(mode, head, *arrays):
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(np.array(head, np.int64).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([exe, mode, src, dst], timeout=120)
        with open(dst, "rb") as f:
            return f.read()

    return run


def _host_log(run, x, u):
    raw = np.frombuffer(run("l", (len(x), 0), x, u), np.float64)
    assert len(raw) == 2 * len(x)
    return raw[:len(x)], raw[len(x):]


def test_the_input_sets_are_what_they_claim():
    a, b, (j, u, xc) = SC.set_a(), SC.set_b(), SC.set_c()
    assert len(a) == SC.N_A == 4135 and len(b) == SC.N_B == 4_247_552 and len(j) == len(u) == len(xc) == SC.N_C == 4219
    assert SC.N_B_BINADE == 4 * 2**20       # (hi = 0 meets its own low word 0 twice: 4 x 2^20 inputs, one fewer distinct)
    for x in (a, b, xc):
        assert (x >= 2.0**-53).all() and (x <= 1.0).all()                      # hs_log's domain
    assert ((b[:SC.N_B_BINADE] >= 0.5) & (b[:SC.N_B_BINADE] < 1.0)).all()
    hi = (SC.bits(b[:2**20]) >> np.uint64(32)) & np.uint64(0xFFFFF)
    np.testing.assert_array_equal(hi, np.arange(2**20, dtype=np.uint64))        # every high word of the binade
    assert sorted({int(e) for e in np.frexp(b[SC.N_B_BINADE:])[1] - 1}) == list(range(-53, -1))
    assert float(a[-1]) == 1.0 and SC.mk(-1, 0x6A09C, 0)[()] in a
    for x in (a, b):
        w = 1.0 - SC.uniforms_for(x)
        assert (w >= 2.0**-53).all() and (w <= 1.0).all()
    rows, kat = SC.philox_rows()
    assert rows.shape == (4099, 6) and kat.shape == (3, 4)
    pats = SC.walk_patterns()
    assert sorted(pats) == ["fours", "mixed", "ones", "twos"] and all(len(p) == 64 for p in pats.values())
    seed, sid, k0 = SC.walks()
    assert len(seed) == 52
    # the 2^33 values carry the block index from 2^32 - 1 to 2^32 inside next4 (its blocks are b = (k + 1) >> 1 and b + 1) and
    # between the cached half and the block of next2 (b = (k + 1) >> 1), at both parities of k
    for pat, first_block in (("fours", 2**32 - 1), ("twos", 2**32)):
        parities = set()
        for start in SC.WALK_K0:
            k = start
            for s in pats[pat]:
                if (k + 1) >> 1 == first_block:
                    parities.add(k & 1)
                k += int(s)
        assert parities == {0, 1}, (pat, parities)


def test_oracle_array_entries_are_the_scalar_ones():
    """O.log_v / uniform_v / philox_v are what the references of both stream tests are computed with: they must be O.log, O.uniform
    and O.philox, and the pure-Python statement, on all of A, all of C and every 64th value of B."""
    a, b, (_, _, xc) = SC.set_a(), SC.set_b(), SC.set_c()
    for name, x, want in (("A", a, SC.log_reference("A")), ("C", xc, SC.log_reference("C")),
                          ("B", b[::64], SC.log_reference("B")[::64])):
        assert not SC.first_difference(np.array([O.log(float(v)) for v in x]), want, x, f"O.log on {name}")
        assert not SC.first_difference(np.array([PY.hs_log(float(v)) for v in x]), want, x, f"PY.hs_log on {name}")
    rows, kat = SC.philox_rows()
    got = O.philox_v(rows)
    np.testing.assert_array_equal(got[:3], kat)
    for r, g in zip(rows.tolist(), got.tolist()):
        assert O.philox(r[:4], r[4:]) == g == list(PY.philox4x32_10(r[:4], r[4:]))
    seed, sid, k0 = (v.tolist() for v in SC.walks())
    want, _ = SC.walk_reference("ones")
    for w in range(0, len(seed), 5):
        for i in (0, 1, 2, 11, 12, 13, 63):
            assert want[w, i] == O.uniform(seed[w], sid[w], k0[w] + i) == PY.uniform(seed[w], sid[w], k0[w] + i)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_hs_log_and_exp1_match_the_oracle(host_program, name):
    x = {"A": SC.set_a, "B": SC.set_b, "C": lambda: SC.set_c()[2]}[name]()
    u = SC.set_c()[1] if name == "C" else SC.uniforms_for(x)
    got_log, got_exp1 = _host_log(host_program, x, u)
    bad = SC.first_difference(got_log, SC.log_reference(name), x, f"hs_log on set {name}")
    assert not bad, bad
    bad = SC.first_difference(got_exp1, SC.exp1_reference(name), u, f"exp1_from_uniform on set {name}")
    assert not bad, bad
    assert (got_log[x < 1.0] < 0.0).all()
    if name == "C":
        assert int(SC.bits(got_exp1)[0]) == SC.NEG_ZERO_BITS               # u = 0: E = -0.0
        assert got_exp1[-1] == -O.log(2.0**-53) and abs(got_exp1[-1] - SC.LONGEST_DRAW) < 1e-13


def test_host_philox_blocks_match_the_oracle(host_program):
    rows, kat = SC.philox_rows()
    got = np.frombuffer(host_program("p", (len(rows), 0), rows), np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(got[:3], kat)
    want = O.philox_v(rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{len(bad)} rows differ; the first is {[hex(v) for v in rows[bad[0]]]}: got {[hex(v) for v in got[bad[0]]]}"


@pytest.mark.parametrize("pattern", ["ones", "twos", "fours", "mixed"])
def test_host_stream_walks_match_the_oracle(host_program, pattern):
    seed, sid, k0 = SC.walks()
    steps = SC.walk_patterns()[pattern]
    want, want_k = SC.walk_reference(pattern)
    raw = host_program("w", (len(seed), len(steps)), seed, sid, k0, steps)
    got = np.frombuffer(raw[:want.size * 8], np.float64).reshape(want.shape)
    got_k = np.frombuffer(raw[want.size * 8:], np.uint64)
    for w in range(len(seed)):
        bad = SC.first_difference(got[w], want[w], np.arange(want.shape[1], dtype=np.float64),
                                  f"walk '{pattern}' of seed {int(seed[w]):#x}, sid {int(sid[w]):#x} from k0 {int(k0[w]):#x} (input = draw)")
        assert not bad, bad
    np.testing.assert_array_equal(got_k, want_k)


def test_the_definition_of_hs_log_is_faithfully_rounded():
    """The oracle's worst error against the true log(x), in ulps of the true value, over all of A, all of C and every 64th value
    of B: strictly below 1 ulp (faithful rounding -- the project's bound, as tests/test_oracle_rng.py asserts against libm).
    Measured when this test was written: 0.8342 ulp at x = 0x1.67980ffffffffp-1, over 74 722 inputs (printed by every run)."""
    mp = pytest.importorskip("mpmath")
    import math

    a, b, (_, _, xc) = SC.set_a(), SC.set_b(), SC.set_c()
    x = np.concatenate([a, xc, b[::64]])
    got = np.concatenate([SC.log_reference("A"), SC.log_reference("C"), SC.log_reference("B")[::64]])
    worst, worst_x = mp.mpf(0), None
    with mp.workprec(200):
        for xv, gv in zip(x.tolist(), got.tolist()):
            if xv == 1.0:
                assert gv == 0.0
                continue
            true = mp.log(mp.mpf(xv))
            err = abs(mp.mpf(gv) - true) / mp.mpf(math.ulp(float(true)))
            if err > worst:
                worst, worst_x = err, xv
    print(f"worst error of hs_log: {float(worst):.4f} ulp at x = {worst_x.hex()} over {len(x)} inputs")
    assert worst < 1, f"hs_log is off by {float(worst):.4f} ulp at x = {worst_x.hex()} ({len(x)} inputs)"
