"""The chosen inputs at which the stream functions of csrc/hs_device.hpp (hs_log, exp1_from_uniform, philox4x32_10, res53,
Stream::next_uniform / next2 / next4) are pinned to the oracle: shared by tests/test_streams_host.py (the header compiled
for the host) and tests/test_gpu_streams.py (what hipcc makes of it).  Everything is deterministic; the only random
numbers are the seeded Philox rows.  Every array is built once and handed out read-only.

mk(e, hi, lo) is the binary64 with unbiased exponent e, high 20 significand bits hi and low 32 significand bits lo.

  A  edges (4 135): every exponent -53 .. -1 x 13 high words (the ends of the field, its middle, and 0x6a09a .. 0x6a09f around
     0x6a09c, where (hx + 0x95f64) & 0x100000 switches k) x 6 low words, and x = 1.0.
  B  the whole reduced range (4 194 304 + 53 248): all 2^20 high words of the binade [0.5, 1) -- both sides of the k switch and
     every reduced argument f of [sqrt(2)/2 - 1, sqrt(2) - 1) -- x 4 low words, and every 4 099th high word with the same low
     words at each other exponent -53 .. -2 (the dk * ln2 terms).  Laid out low word by low word, so that B[::64] still holds
     all four of them.
  C  the draws nearest to zero (4 219): u = j * 2^-53 for j in 0 .. 4095 and 2^k - 1, 2^k, 2^k + 1 for k in 12 .. 53, as far as
     1 - u >= 2^-53 (the last one is j = 2^53 - 1, the longest draw -log(2^-53)); 2^12 - 1 is counted once.
"""
import functools

import numpy as np

A_HI = (0, 1, 2, 0x6A09A, 0x6A09B, 0x6A09C, 0x6A09D, 0x6A09E, 0x6A09F, 0x7FFFF, 0x80000, 0xFFFFE, 0xFFFFF)
A_LO = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
EXPONENTS = tuple(range(-53, 0))
N_A, N_B_BINADE, N_B, N_C = 4135, 4_194_304, 4_194_304 + 53_248, 4219
B_STRIDE = 4099
NEG_ZERO_BITS = 0x8000000000000000
LONGEST_DRAW = 36.7368005696771          # -log(2^-53)

KAT_ROWS = (   # Random123 kat_vectors, philox4x32-10: (ctr, key, expected) -- the three of tests/test_oracle_rng.py
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)
N_PHILOX_RANDOM = 4096

WALK_STEPS = 64
# every ordered pair of {1, 2, 4}, each call at both parities of k within two periods; it opens with two next4 so that the walks
# from 2^33 - 6 and 2^33 - 3 carry the block index inside next4 here too
_MIXED = (4, 4, 1, 4, 2, 1, 1, 2, 2, 4)
WALK_K0 = (0, 1, 2, 3, *range(2**33 - 6, 2**33 + 2), 2**40 + 1)
WALK_STREAMS = ((42, 0), (42, (5 << 3) | 1), (2**63 + 12345, (2**40 << 3) | 2), (2**64 - 1, 2**64 - 1))


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def mk(e, hi, lo) -> np.ndarray:
    e, hi, lo = np.broadcast_arrays(np.asarray(e, np.int64), np.asarray(hi, np.int64), np.asarray(lo, np.int64))
    bits = ((e + 1023).astype(np.uint64) << np.uint64(52)) | (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return bits.view(np.float64)


def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def set_a() -> np.ndarray:
    e, hi, lo = np.meshgrid(np.array(EXPONENTS), np.array(A_HI), np.array(A_LO), indexing="ij")
    x = np.concatenate([mk(e, hi, lo).ravel(), [1.0]])
    assert len(x) == N_A == len(np.unique(bits(x)))
    return _frozen(x)


def _b_low_words(hi: np.ndarray) -> list:
    return [np.zeros_like(hi), np.full_like(hi, 0xFFFFFFFF), np.full_like(hi, 0x80000000), (hi * 2654435761) % 2**32]


@functools.lru_cache(maxsize=None)
def set_b() -> np.ndarray:
    hi = np.arange(2**20, dtype=np.int64)
    parts = [mk(-1, hi, lo) for lo in _b_low_words(hi)]
    assert sum(len(p) for p in parts) == N_B_BINADE
    hs = hi[::B_STRIDE]
    e = np.repeat(np.array(EXPONENTS[:-1]), len(hs))
    hs = np.tile(hs, len(EXPONENTS) - 1)
    parts += [mk(e, hs, lo) for lo in _b_low_words(hs)]
    x = np.concatenate(parts)
    assert len(x) == N_B
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def set_c():
    """-> (j, u = j * 2^-53, x = 1 - u); both are exact."""
    js = set(range(4096))
    for k in range(12, 54):
        js.update(j for j in (2**k - 1, 2**k, 2**k + 1) if j <= 2**53 - 1)       # 1 - u >= 2^-53
    j = np.array(sorted(js), np.uint64)
    assert len(j) == N_C
    u = j.astype(np.float64) * 2.0**-53          # j < 2^53: the conversion and the scaling are exact
    x = 1.0 - u
    assert u[0] == 0.0 and x[0] == 1.0 and u[-1] == 1.0 - 2.0**-53 and x[-1] == 2.0**-53
    assert all(int(v * 2**53) == int(w) for v, w in zip(u, j))
    return _frozen(j), _frozen(u), _frozen(x)


def uniforms_for(x: np.ndarray) -> np.ndarray:
    """A second route to hs_log for sets A and B, through exp1_from_uniform: u = x (so 1 - u stays inside hs_log's domain
    [2^-53, 1]), and u = 0 where x = 1."""
    return np.where(x < 1.0, x, 0.0)


@functools.lru_cache(maxsize=None)
def philox_rows():
    """-> (rows [3 + 4096][6] uint32 = c0 .. c3, k0, k1; the known answers of the first three rows)."""
    kat = np.array([c + k for c, k, _ in KAT_ROWS], np.uint32)
    rnd = np.random.default_rng(0x5EED).integers(0, 2**32, (N_PHILOX_RANDOM, 6), dtype=np.uint64).astype(np.uint32)
    rows = np.concatenate([kat, rnd])
    assert rows.shape == (3 + N_PHILOX_RANDOM, 6)
    return _frozen(rows), _frozen(np.array([o for _, _, o in KAT_ROWS], np.uint32))


@functools.lru_cache(maxsize=None)
def walk_patterns() -> dict:
    mixed = (_MIXED * 7)[:WALK_STEPS]
    pats = {"ones": (1,) * WALK_STEPS, "twos": (2,) * WALK_STEPS, "fours": (4,) * WALK_STEPS, "mixed": mixed}
    assert {(a, b) for a, b in zip(mixed, mixed[1:])} == {(a, b) for a in (1, 2, 4) for b in (1, 2, 4)}
    k, seen = 0, set()
    for s in mixed:                              # (from an odd k0 the parities are the other way round)
        seen.add((s, k & 1))
        k += s
    assert seen == {(s, p) for s in (1, 2, 4) for p in (0, 1)}
    return {name: _frozen(np.array(p, np.uint8)) for name, p in pats.items()}


@functools.lru_cache(maxsize=None)
def walks():
    """-> (seed[52], sid[52], k0[52]) uint64: every k0 with every (seed, sid)."""
    rows = [(seed, sid, k0) for seed, sid in WALK_STREAMS for k0 in WALK_K0]
    assert len(rows) == 52 and len(WALK_K0) == 13
    seed, sid, k0 = (np.array(c, np.uint64) for c in zip(*rows))
    return _frozen(seed), _frozen(sid), _frozen(k0)


@functools.lru_cache(maxsize=None)
def walk_reference(pattern: str):
    """Value i of a walk is the oracle's uniform(seed, sid, k0 + i); k_end = k0 + sum(steps)."""
    from oracle import hs_oracle as O

    seed, sid, k0 = walks()
    total = int(walk_patterns()[pattern].sum(dtype=np.int64))
    want = np.stack([O.uniform_v(int(s), int(i), int(k), total) for s, i, k in zip(seed, sid, k0)])
    return _frozen(want), _frozen(k0 + np.uint64(total))


@functools.lru_cache(maxsize=None)
def log_reference(name: str) -> np.ndarray:
    """hs_log_ref (oracle/hs_rng_ref.h) of set "A", "B" or "C" (of C's x = 1 - u), by the oracle's array entry."""
    from oracle import hs_oracle as O

    x = {"A": set_a, "B": set_b, "C": lambda: set_c()[2]}[name]()
    return _frozen(O.log_v(x))


@functools.lru_cache(maxsize=None)
def exp1_reference(name: str) -> np.ndarray:
    """-hs_log_ref(1 - u) of the uniforms that go with the set: uniforms_for(x) for A and B, C's own u."""
    from oracle import hs_oracle as O

    u = set_c()[1] if name == "C" else uniforms_for({"A": set_a, "B": set_b}[name]())
    return _frozen(-O.log_v(1.0 - u))


def first_difference(got: np.ndarray, want: np.ndarray, inputs: np.ndarray, what: str) -> str:
    """'' if the two arrays agree in every bit (-0.0 and +0.0 differ), else a message that names the first input that differs."""
    g, w = bits(got).ravel(), bits(want).ravel()
    assert g.shape == w.shape, (got.shape, want.shape)
    bad = np.flatnonzero(g != w)
    if not len(bad):
        return ""
    i = int(bad[0])
    x = np.ascontiguousarray(inputs, np.float64).ravel()[i]
    return (f"{what}: {len(bad)} of {len(g)} inputs differ; the first is #{i}, input {float(x).hex()} "
            f"(bits {int(bits(np.array([x]))[0]):#018x}): got {int(g[i]):#018x}, want {int(w[i]):#018x}")
