"""One table of uniform grids (Source.poisson -> Server(Exp, one worker) -> Sink per LP) for every kernel that runs them --
hs_station_run<1, false, true, true>, hs_station_wide<4 / 8 / 16>, hs_station_wave<16 / 8> (fresh and loading) with
hs_station_wide_finish -- and what the C oracle says about each case.  tests/test_uniform_cases_host.py checks the table on the
CPU (the conditions each load is there for hold for the oracle's own numbers); tests/test_gpu_uniform_kernels_oracle.py runs
every kernel alone against it; tests/test_gpu_wide.py takes its verdicts from it.

The loads are values of tests/test_gpu_wide.py::test_wave_kernel_on_random_uniform_grids' own lists, at the corners nothing
else pins to the oracle:

| load (rate, mean, span s) | why |
|---|---|
| 0.002, 0.1, 40 | most LPs see no tick in a window |
| 0.05, 0.8, 40 | a handful of long services per LP |
| 8, 0.1, 2 | the headline load |
| 60, 0.001, 0.3 | one request in service at the end, nobody waiting |
| 60, 0.02, 0.3 | overloaded: the buffer grows |
| 20, 0.3, 2 | every LP enters window two with requests waiting and one in service |
| 3, 0.8, 7 | long services, a few waiting |
| 60, 0.02, 7 and 60, 0.001, 7 (17 and 65 LPs) | several 128-request steps of the wave kernel: carries and the double-buffered sums |
| 8, 0.1, 0.02 continued to 2 s | a first window in which most LPs see no tick |

Every case runs from three starts, once to `start + span` and twice as two windows (second end at 1.3 x and 2 x the span)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

SIZES = (1, 17, 63, 64, 65, 513, 1025)
STARTS = (0, 17, 1_500_000_000)
ONE_LANE = 1 << 22
LOADING = 1 << 29           # keep the reset kernel: hs_station_wave's loading instantiation


@dataclass(frozen=True)
class Load:
    rate: float
    mean: float
    span_ns: int
    seed: int = 1234
    sizes: tuple = SIZES
    then_ns: int | None = None      # the only second end (instead of 1.3 x and 2 x the span), as a span from the start

    @property
    def name(self):
        return f"rate {self.rate:g} mean {self.mean:g} span {self.span_ns / 1e9:g} s"

    def shapes(self, start):
        """(name, window ends): the last end is the run's end, the ones before it are windows."""
        e1 = start + self.span_ns
        if self.then_ns is not None:
            return (("one run", (e1,)), ("continued", (e1, start + self.then_ns)))
        return (("one run", (e1,)), ("second end 1.3 x", (e1, start + self.span_ns * 13 // 10)), ("second end 2 x", (e1, start + 2 * self.span_ns)))


def _s(x):
    return int(round(x * 1e9))


LOADS = (
    Load(0.002, 0.1, _s(40)),
    Load(0.05, 0.8, _s(40)),
    Load(8.0, 0.1, _s(2)),
    Load(60.0, 0.001, _s(0.3), seed=15),       # (a seed at which no LP of any size has anyone waiting at the first end)
    Load(60.0, 0.02, _s(0.3)),
    Load(20.0, 0.3, _s(2)),
    Load(3.0, 0.8, _s(7)),
    Load(60.0, 0.02, _s(7), seed=5, sizes=(17, 65)),
    Load(60.0, 0.001, _s(7), seed=5, sizes=(17, 65)),
    Load(8.0, 0.1, _s(0.02), then_ns=_s(2)),
)


def loads_for(n):
    return tuple(ld for ld in LOADS if n in ld.sizes)


# ---- ring positions of the one-lane kernel: hs_station_run<1, false, true, true> keeps value k of a stream in slot k % RING of an LDS
# ring and refills REFILL values from a multiple of REFILL at or below the position a window starts at (HS_KRING / HS_KREFILL)
RING, REFILL = 24, 8
RING_LPS, RING_SEED = 64, 9
RING_LOADS = ((8.0, 0.1), (20.0, 0.3))          # the base case; overloaded: lanes enter a window with requests waiting
RING_STARTS = (0, 1_500_000_000)


def ring_ends(start):
    return tuple(int(start + x) for x in np.linspace(0.13e9, 4.9e9, 16))


def stream_positions(out):
    """Where the next window's arrival and service streams begin, per LP: the bootstrap drew arrival 0."""
    return 1 + out["generated"], out["completed"] + out["active"]


@functools.lru_cache(maxsize=None)
def ring_expected(rate, mean, start, k):
    """The oracle after the first k + 1 ends of ring_ends(start)."""
    ends = ring_ends(start)[:k + 1]
    out = oracle_outputs(RING_LPS, oracle_run(RING_LPS, rate, mean, ends, start, RING_SEED))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- windows that begin inside a group: every run_until ends with the election of ONE event beyond its end, the first of its
# nanosecond's group; the next window finishes that group in event order before anything else.  With a single light LP almost every
# window ends on the tick of an idle Server, so the next one begins by drawing a service time outside the request-order loop.
GROUP_SIZES, GROUP_STARTS, GROUP_SEED, GROUP_WINDOWS = (1, 3), (0, 1_500_000_000), 15, 400
GROUP_RATE, GROUP_MEAN = 60.0, 0.001


def group_ends(start):
    return tuple(int(start + x) for x in np.linspace(0.02e9, 7e9, GROUP_WINDOWS))


@functools.lru_cache(maxsize=None)
def group_expected(n, start, k):
    """The oracle after the first k + 1 ends of group_ends(start)."""
    out = oracle_outputs(n, oracle_run(n, GROUP_RATE, GROUP_MEAN, group_ends(start)[:k + 1], start, GROUP_SEED))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def inside_a_tick_group_of_an_idle_server(out):
    """Per LP: the Source's tick has been processed, its Request is not enqueued yet, and the worker is idle."""
    return (out["generated"] > out["accepted"]) & (out["active"] == 0)


# ---- what is compared: one flat dict per run, the same keys for the oracle and an engine ------------------------------------------
FIELDS = ("tot_events", "tot_final", "tot_completed", "tot_sink_records", "by_kind", "generated", "accepted", "completed",
          "queue_depth", "active", "total_service_bits", "sink_counts", "sink_t", "sink_created")
PER_LP = ("generated", "accepted", "completed", "queue_depth", "active", "total_service_bits", "sink_counts")


def oracle_outputs(n, r):
    """An oracle Result of O.mm1_chains(n) in the engine's terms (nodes: n Sources, then Server, Sink per chain)."""
    srv = np.arange(n) * 2 + n
    sinks = sorted(r.sinks)
    counts = np.array([len(r.sinks[i][0]) for i in sinks], np.int64)
    return {
        "tot_events": int(r.events_processed), "tot_final": int(r.final_time_ns), "tot_completed": int(r.completed[srv].sum()),
        "tot_sink_records": int(counts.sum()), "by_kind": np.asarray(r.events_by_kind, np.int64),
        "generated": r.generated[:n].astype(np.int64), "accepted": r.accepted[srv].astype(np.int64),
        "completed": r.completed[srv].astype(np.int64), "queue_depth": r.depth[srv].astype(np.int64),
        "active": r.active[srv].astype(np.int64),
        "total_service_bits": np.ascontiguousarray(r.total_service_s[srv], np.float64).view(np.int64),      # bit for bit
        "sink_counts": counts,
        "sink_t": np.concatenate([r.sinks[i][0] for i in sinks]) if sinks else np.zeros(0, np.int64),
        "sink_created": np.concatenate([r.sinks[i][1] for i in sinks]) if sinks else np.zeros(0, np.int64),
    }


def engine_outputs(eng):
    s = eng.summary()
    st = eng.lp_stats()
    counts, t, cr = eng.read_sinks()
    return {
        "tot_events": int(s.events_processed), "tot_final": int(s.final_time_ns), "tot_completed": int(s.requests_completed),
        "tot_sink_records": int(s.sink_records), "by_kind": np.asarray(s.events_by_kind, np.int64),
        "generated": st["generated"], "accepted": st["accepted"], "completed": st["completed"], "queue_depth": st["queue_depth"],
        "active": st["active"].astype(np.int64),
        "total_service_bits": np.ascontiguousarray(st["total_service_s"], np.float64).view(np.int64),
        "sink_counts": counts, "sink_t": t, "sink_created": cr,
    }


def engine_lp_outputs(eng):
    """The per-LP statistics alone (no Sink records, no summary): what a test reads between windows."""
    st = eng.lp_stats()
    return {"generated": st["generated"], "accepted": st["accepted"], "completed": st["completed"], "queue_depth": st["queue_depth"],
            "active": st["active"].astype(np.int64),
            "total_service_bits": np.ascontiguousarray(st["total_service_s"], np.float64).view(np.int64)}


def differences(got, want, fields=None):
    """[(field, description of the first difference)] in FIELDS order; empty: equal."""
    out = []
    for k in fields or FIELDS:
        if k not in got or k not in want:
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape:
            out.append((k, f"{k}: {a.size} values, the oracle has {b.size}"))
        elif a.ndim == 0:
            if a != b:
                out.append((k, f"{k}: {a} != oracle {b}"))
        else:
            bad = np.flatnonzero(a != b)
            if bad.size:
                i = int(bad[0])
                where = f"LP {i}" if k in PER_LP else f"index {i}"
                out.append((k, f"{k}: {bad.size} of {a.size} differ, first at {where}: {a[i]} != oracle {b[i]}"))
    return out


def first_difference(got, want, fields=None):
    d = differences(got, want, fields)
    return d[0][1] if d else None


def verdict(a, name_a, b, name_b, want):
    """Which of two sides that disagree equals the oracle, and where the other leaves it."""
    da, db = differences(a, want), differences(b, want)
    parts = []
    for name, d in ((name_a, da), (name_b, db)):
        parts.append(f"{name} EQUALS the oracle" if not d else f"{name} DIFFERS from the oracle in {[k for k, _ in d]} ({d[0][1]})")
    return "; ".join(parts)


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------
def oracle_run(n, rate, mean, ends, start, seed):
    from oracle import hs_oracle as O

    g = O.mm1_chains(n, rate=rate, mean=mean)
    return O.run(g, int(ends[-1]), start_ns=int(start), seed=int(seed), windows=[int(e) for e in ends[:-1]])


@functools.lru_cache(maxsize=None)
def _expected(n, start, li, ends):
    ld = LOADS[li]
    out = oracle_outputs(n, oracle_run(n, ld.rate, ld.mean, ends, start, ld.seed))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)          # shared between tests: nobody changes it
    return out


def expected(n, start, load, ends):
    """The oracle's outputs for one case and one window shape; computed once per process."""
    return _expected(int(n), int(start), LOADS.index(load), tuple(int(e) for e in ends))


# ---- the engine's side -----------------------------------------------------------------------------------------------------------
def force(k):
    """Debug flags: 4 / 8 / 16 lanes per LP (hs_station_wide); 64 / 65: a wavefront per LP, 16 / 8 LPs per workgroup (hs_station_wave)."""
    return ({4: 3, 8: 4, 16: 5, 64: 7, 65: 8}[k]) << 24


def variants():
    """(name, debug flags) of every kernel a fresh uniform grid can run on."""
    return (("one lane per LP", ONE_LANE), ("4 lanes per LP", force(4)), ("8 lanes per LP", force(8)), ("16 lanes per LP", force(16)),
            ("a wavefront per LP, 16 per workgroup", force(64)), ("a wavefront per LP, 8 per workgroup", force(65)),
            ("a wavefront per LP, 16 per workgroup, reset kernel + loading instantiation", force(64) | LOADING))


def lanes_of(path):
    from happy_simulator_amd import _native as N

    return (path >> N.RUN_LANES_SHIFT) & 0xFF


def kernel_of(path):
    from happy_simulator_amd import _native as N

    return path & (N.RUN_ONE_LANE | N.RUN_ONE_LANE_UNI | N.RUN_WIDE | N.RUN_WAVE | N.RUN_TANDEM | N.RUN_SINGLE_HEAP)


def expected_uniform_kernel(n, horizon, lanes, f64=True):
    """hs_engine.hip wide_lanes for a fresh uniform grid without debug flags: (kernel bit, lanes per LP or LPs per workgroup);
    `lanes`: CUs x 4 SIMDs x 64 of the device."""
    from happy_simulator_amd import _native as N

    if not f64:
        return N.RUN_ONE_LANE, 0
    wave_ok = horizon < (1 << 39)
    if wave_ok and n * 16 <= lanes:
        return N.RUN_WAVE, 8
    if wave_ok and n * 3 <= lanes * 2:
        return N.RUN_WAVE, 16
    if n * 16 <= lanes:
        return N.RUN_WIDE, 8
    if n * 4 <= lanes:
        return N.RUN_WIDE, 4
    return N.RUN_ONE_LANE_UNI, 0


def device_lanes():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * 64


def expected_path(flags, n, horizon, fresh=True):
    """(kernel bit, lanes) run_path() must report for a uniform grid under these debug flags; an engine that has run before
    continues on the one-lane kernel whatever the flags say."""
    from happy_simulator_amd import _native as N

    forced = (flags >> 24) & 0xF
    if not fresh or flags & ONE_LANE:
        return N.RUN_ONE_LANE_UNI, 0
    if forced == 7:
        return N.RUN_WAVE, 16
    if forced == 8:
        return N.RUN_WAVE, 8
    if forced:
        return N.RUN_WIDE, 1 << (forced - 1)
    return expected_uniform_kernel(n, horizon, device_lanes())


def check_path(path, flags, n, horizon, fresh, what=""):
    kernel, lanes = expected_path(flags, n, horizon, fresh)
    assert kernel_of(path) == kernel and lanes_of(path) == lanes, \
        f"{what}: run_path {hex(path)}, expected kernel bit {kernel} with {lanes} lanes (flags {hex(flags)}, {'fresh' if fresh else 'continued'})"


def run_engine(n, rate, mean, ends, start, seed, flags, each_window=None):
    """A uniform grid through the window ends on the kernel the flags ask for; run_path() is asserted after every window.
    each_window(i, eng) is called after window i.  Returns engine_outputs."""
    from happy_simulator_amd import _native as N
    from happy_simulator_amd.engine import StationArrays, StationEngine

    st = StationArrays.uniform(n, rate=rate, mean=mean)
    with StationEngine(st, mode=N.MODE_SINGLE, horizon_ns=int(ends[-1]), start_ns=int(start), seed=int(seed)) as eng:
        eng.set_debug_flags(flags)
        for i, e in enumerate(ends):
            eng.run_until(int(e))
            check_path(eng.run_path(), flags, n, int(ends[-1]), i == 0, f"window {i}")
            if each_window is not None:
                each_window(i, eng)
        return engine_outputs(eng)


def from_run(out):
    """The dict tests/test_gpu_wide.py::_run returns, in this module's terms."""
    o = {k: out[k] for k in FIELDS if k in out}
    o["active"] = np.asarray(out["active"]).astype(np.int64)
    o["total_service_bits"] = np.ascontiguousarray(out["total_service_s"], np.float64).view(np.int64)
    return o


# ---- repeatability: the same cases over and over in one process, between engines of other sizes ----------------------------------
REPEAT_N, REPEAT_START = 513, 0
REPEAT_LOADS = ((8.0, 0.1, 2_000_000_000), (20.0, 0.3, 2_000_000_000))


def repeat_load(which):
    (ld,) = [x for x in LOADS if (x.rate, x.mean, x.span_ns) == REPEAT_LOADS[which] and x.then_ns is None]
    return ld


def _scribble(n, seed):
    """An engine of another size, run briefly and destroyed: its allocations go back to the allocator written to."""
    from happy_simulator_amd import _native as N
    from happy_simulator_amd.engine import StationArrays, StationEngine

    with StationEngine(StationArrays.uniform(n, rate=8.0, mean=0.1), mode=N.MODE_SINGLE, horizon_ns=500_000_000, seed=seed) as eng:
        eng.run_until(500_000_000)
        eng.summary()


def repeat_sequence(which, repeats=10):
    """Every variant `repeats` times on REPEAT_N LPs (two windows, second end at 1.3 x), engines of 3 000 and of 17 LPs created
    and destroyed in between; every run against the oracle.  Returns (runs, [what differed])."""
    ld = repeat_load(which)
    name, ends = ld.shapes(REPEAT_START)[1]
    want = expected(REPEAT_N, REPEAT_START, ld, ends)
    bad, runs = [], 0
    for rep in range(repeats):
        for vname, flags in variants():
            _scribble(3000 if runs % 2 == 0 else 17, seed=runs + 1)
            got = run_engine(REPEAT_N, ld.rate, ld.mean, ends, REPEAT_START, ld.seed, flags)
            runs += 1
            d = differences(got, want)
            if d:
                bad.append(f"{ld.name}, {vname}, repeat {rep}: differs in {[k for k, _ in d]}: {d[0][1]}")
    return runs, bad
