"""CPU: the refusal of a negative start when lowering, and -- as documentation, not as evidence about the project's code -- the
binary64 facts the engines' absolute-time gates are designed around (csrc/hs_device.hpp).  The arithmetic tests below check a numpy
restatement of the mask and Python's own float operations; the device's code is compared with Python's exact ints in
tests/test_gpu_time_range.py (hs_debug_time_ops), and whole runs are placed on both sides of every gate there."""
import math

import numpy as np
import pytest

import happy_simulator_amd as hs
from happy_simulator_amd import Instant
from happy_simulator_amd.lowering import UnsupportedTopology

TWO52 = float(1 << 52)


def i64_from_whole_d(d):
    """hs_device.hpp i64_from_whole_d: the bits under an exponent of 2^52 after adding 2^52 (valid for whole d in [0, 2^52))."""
    return int((np.array([d + TWO52], np.float64).view(np.uint64)[0]) & np.uint64((1 << 52) - 1))


def _edges():
    out = []
    for k in (39, 40, 44, 50, 51, 52, 53, 62):
        out += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    rng = np.random.default_rng(52)
    return out + [int(v) for v in np.exp2(rng.uniform(0.0, 62.0, 2000)).astype(np.int64)]


def test_whole_ns_mask_is_exact_exactly_below_2_52():
    """(A restatement of the mask in numpy: it documents why the gates stop at 2^52, and what the LB defect looked like.)"""
    for t in _edges():
        if t < (1 << 52):
            assert float(t) == t and i64_from_whole_d(float(t)) == t, t
        else:
            assert i64_from_whole_d(float(t)) != t, t
    # the defect the LB gate let through: a departure S + 2^52 became about S / 2 -- an instant before the run's end
    for s in (1, 565_956_456 * 2, 1_999_999_999):
        assert abs(i64_from_whole_d(float(s + (1 << 52))) - s / 2) <= 1


def test_binary64_truncation_equals_int_conversion_in_range():
    """ns_from_seconds_d = trunc(x * 1e9) equals int(x * 1_000_000_000) as a value wherever the product fits int64, and whole ns
    survive float() only below 2^53 -- why the binary64 paths stop at 2^52 with room for one step."""
    for t in _edges():
        x = float(t) / 1_000_000_000
        assert math.trunc(x * 1e9) == int(x * 1_000_000_000)
        assert (float(t) == t) == (t <= (1 << 53) or t % (1 << (t.bit_length() - 53)) == 0)


def test_longest_draw_bound():
    """exp1_from_uniform(u) = -log(1 - u) with u a 53-bit fraction in [0, 1): at most -log(2^-53) = 36.74 means.  Every gate and
    every int64 refusal uses 36.8 as that bound."""
    assert -math.log(2.0 ** -53) < 36.8
    # the station gate (horizon < 2^51, rates > 1e-3, means < 1e4): one step more stays below 2^52
    assert (1 << 51) + 36.8 / 1e-3 * 1e9 < TWO52 and (1 << 51) + 36.8 * 1e4 * 1e9 < TWO52


def test_negative_start_is_refused_when_lowering():
    sink = hs.Sink()
    server = hs.Server("srv", service_time=hs.ExponentialLatency(0.1), downstream=sink)
    source = hs.Source.poisson(rate=8, target=server)
    sim = hs.Simulation(start_time=Instant(-1_000_000_000), end_time=Instant(1_000_000_000), sources=[source],
                        entities=[server, sink])
    with pytest.raises(UnsupportedTopology, match="start_time"):
        sim.run()
