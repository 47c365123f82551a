"""GPU: what hipcc makes of the stream functions of csrc/hs_device.hpp -- hs_log, exp1_from_uniform, res53, philox4x32_10 and
Stream::init / next_uniform / next2 / next4 -- against the oracle at the chosen inputs of tests/stream_cases.py, through the
hs_debug_log / hs_debug_philox / hs_debug_stream_walk hooks.

Every comparison is bit equality on uint64 views (so -0.0 and +0.0 differ), no input is skipped or sampled, and a failure names
the first input that differs.  The accuracy of the definition itself is measured on the CPU (tests/test_streams_host.py): the
device has no tolerance of its own, it inherits the oracle's bound through the equality asserted here.
"""
import numpy as np
import pytest

import stream_cases as SC
from oracle import hs_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_hs_log_and_exp1_match_the_oracle(name):
    from happy_simulator_amd.engine import debug_log

    x = {"A": SC.set_a, "B": SC.set_b, "C": lambda: SC.set_c()[2]}[name]()
    u = SC.set_c()[1] if name == "C" else SC.uniforms_for(x)
    assert len(x) == len(u) == {"A": 4135, "B": 4_194_304 + 53_248, "C": 4219}[name]
    got_log, got_exp1 = debug_log(x, u)
    bad = SC.first_difference(got_log, SC.log_reference(name), x, f"hs_log on set {name}")
    assert not bad, bad
    bad = SC.first_difference(got_exp1, SC.exp1_reference(name), u, f"exp1_from_uniform on set {name}")
    assert not bad, bad
    assert (got_log[x < 1.0] < 0.0).all()
    if name == "A":
        assert float(x[-1]) == 1.0 and int(SC.bits(got_log)[-1]) == 0          # hs_log(1.0) = +0.0
    if name == "C":
        assert u[0] == 0.0 and int(SC.bits(got_exp1)[0]) == SC.NEG_ZERO_BITS   # u = 0: E = -0.0
        assert u[-1] == 1.0 - 2.0**-53 and got_exp1[-1] == -O.log(2.0**-53) and abs(got_exp1[-1] - SC.LONGEST_DRAW) < 1e-13


def test_device_philox_blocks_match_the_oracle():
    from happy_simulator_amd.engine import debug_philox

    rows, kat = SC.philox_rows()
    assert len(rows) == 3 + 4096
    got = debug_philox(rows)
    np.testing.assert_array_equal(got[:3], kat)                   # the Random123 known answers, all 128 bits
    want = O.philox_v(rows)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{len(bad)} rows differ; the first is {[hex(v) for v in rows[bad[0]]]}: got {[hex(v) for v in got[bad[0]]]}"


@pytest.mark.parametrize("pattern", ["ones", "twos", "fours", "mixed"])
def test_device_stream_walks_match_the_oracle(pattern):
    from happy_simulator_amd.engine import debug_stream_walk

    seed, sid, k0 = SC.walks()
    steps = SC.walk_patterns()[pattern]
    assert len(seed) == 52 and len(steps) == 64
    want, want_k = SC.walk_reference(pattern)
    got, got_k = debug_stream_walk(seed, sid, k0, steps)
    assert got.shape == want.shape
    for w in range(len(seed)):
        bad = SC.first_difference(got[w], want[w], np.arange(want.shape[1], dtype=np.float64),
                                  f"walk '{pattern}' of seed {int(seed[w]):#x}, sid {int(sid[w]):#x} from k0 {int(k0[w]):#x} (input = draw)")
        assert not bad, bad
    np.testing.assert_array_equal(got_k, want_k)
