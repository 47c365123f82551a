"""The live reference's results as recorded under tests/golden/live_*/, and the one writer of those files.

A `Recorded(directory, key_prefix, recorder)` reads tests/golden/<directory>/part_*.npz, written by tests/golden/<recorder> (run where
the reference is installed).  `get(name, *args)` returns what the reference computed for that key when it was recorded -- the same
dicts of integers, floats and arrays, bit for bit.  A key without a recording raises KeyError with the case's name and the recorder
to run: a test that needs it fails by name, it is never skipped.  `write(cases)` replaces the directory's parts.

A part file holds the arrays of its cases and an `index` (JSON: key -> [skeleton, array names]); `write_parts` closes a part once
the estimate of its compressed size passes `part_bytes`, so that every committed file stays under 1 MiB.
"""
from __future__ import annotations

import glob
import hashlib
import json
import os
import zlib

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_PART_BYTES = 833_000              # tests/golden/live_reference/part_002.npz: no later part is larger than this one
PART_BYTES = 640 * 1024                # the estimate a part is closed at


def _key(name, args):
    blob = json.dumps([name, list(args)], sort_keys=True, default=repr)
    return hashlib.sha256(blob.encode()).hexdigest()[:20]


def _encode(obj, arrays):
    """obj -> a JSON value; numpy arrays go to `arrays` and are referenced by index (dict keys, tuples and scalar types kept)."""
    if isinstance(obj, np.ndarray):
        arrays.append(obj)
        return {"nd": len(arrays) - 1}
    if isinstance(obj, dict):
        return {"dict": [[_encode(k, arrays), _encode(v, arrays)] for k, v in obj.items()]}
    if isinstance(obj, tuple):
        return {"tuple": [_encode(v, arrays) for v in obj]}
    if isinstance(obj, list):
        return [_encode(v, arrays) for v in obj]
    if isinstance(obj, np.generic):
        arrays.append(np.asarray(obj))
        return {"np": len(arrays) - 1}
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    raise TypeError(f"cannot record a {type(obj).__name__}")


def _decode(v, arrays):
    if isinstance(v, list):
        return [_decode(x, arrays) for x in v]
    if isinstance(v, dict):
        if "nd" in v:
            return arrays[v["nd"]]
        if "np" in v:
            return arrays[v["np"]][()]
        if "tuple" in v:
            return tuple(_decode(x, arrays) for x in v["tuple"])
        return {_decode(k, arrays): _decode(x, arrays) for k, x in v["dict"]}
    return v


def read_parts(rec_dir):
    """{key: (skeleton, arrays)} of every part file of `rec_dir`."""
    store = {}
    for path in sorted(glob.glob(os.path.join(rec_dir, "*.npz"))):
        with np.load(path, allow_pickle=False) as z:
            index = json.loads(bytes(z["index"]).decode())
            for key, (skeleton, names) in index.items():
                store[key] = (skeleton, [z[n] for n in names])
    return store


def write_parts(rec_dir, cases, part_bytes=PART_BYTES, first=None, max_part_bytes=None):
    """{key: (skeleton, arrays)} -> rec_dir/part_NNN.npz in key order, each closed at an estimate of `part_bytes` compressed.
    first=None replaces what was there; first=n leaves the stored parts as they are and numbers the new ones from n."""
    os.makedirs(rec_dir, exist_ok=True)
    if first is None:
        for path in glob.glob(os.path.join(rec_dir, "*.npz")):
            os.remove(path)
    part, index, size, n = {}, {}, 0, first or 0

    def flush():
        nonlocal part, index, size, n
        if index:
            part["index"] = np.frombuffer(json.dumps(index, separators=(",", ":")).encode(), np.uint8)
            np.savez_compressed(os.path.join(rec_dir, f"part_{n:03d}.npz"), **part)
            n += 1
        part, index, size = {}, {}, 0

    for key in sorted(cases):
        skeleton, arrays = cases[key]
        est = len(zlib.compress(json.dumps(skeleton).encode())) + sum(
            len(zlib.compress(np.ascontiguousarray(a).tobytes())) for a in arrays) + 256 * (len(arrays) + 1)
        if index and size + est > part_bytes:
            flush()
        names = [f"{key}_{i}" for i in range(len(arrays))]
        for nm, a in zip(names, arrays):
            part[nm] = np.asarray(a)
        index[key] = (skeleton, names)
        size += est
    flush()
    if max_part_bytes is not None:
        for path in glob.glob(os.path.join(rec_dir, "*.npz")):
            assert os.path.getsize(path) <= max_part_bytes, (path, os.path.getsize(path))


class Recorded:
    def __init__(self, directory, key_prefix, recorder, part_bytes=PART_BYTES, max_part_bytes=MAX_PART_BYTES):
        self.rec_dir = os.path.join(GOLDEN_DIR, directory)
        self.key_prefix, self.recorder = key_prefix, recorder
        self.part_bytes, self.max_part_bytes = part_bytes, max_part_bytes
        self._store = None

    def key(self, name, *args):
        return _key(f"{self.key_prefix}:{name}", args)

    def get(self, name, *args):
        if self._store is None:
            self._store = read_parts(self.rec_dir)
        k = self.key(name, *args)
        try:
            skeleton, arrays = self._store[k]
        except KeyError:
            what = f"{name}{tuple(a.get('name', '...') if isinstance(a, dict) else a for a in args)!r}"[:160]
            raise KeyError(f"no recorded reference result for {what} (key {k}): run tests/golden/{self.recorder} where the "
                           "reference is installed") from None
        return _decode(skeleton, arrays)

    def write(self, cases):
        """{key: result} -> the directory's part_NNN.npz, replacing what was there."""
        encoded = {}
        for k, result in cases.items():
            arrays = []
            encoded[k] = (_encode(result, arrays), arrays)
        write_parts(self.rec_dir, encoded, self.part_bytes, max_part_bytes=self.max_part_bytes)


# the two oldest families were recorded at the part size of tests/reference_runs.py and without the cap on a part's size
STRATEGIES = Recorded("live_strategies", "strategies", "make_golden_strategies.py", part_bytes=900 * 1024, max_part_bytes=None)
RATE_LIMITER = Recorded("live_rate_limiter", "rate_limiter", "make_golden_rate_limiter.py", part_bytes=900 * 1024, max_part_bytes=None)
FAULTS = Recorded("live_faults", "faults", "make_golden_faults.py")
HEALTH = Recorded("live_health", "health", "make_golden_health.py")
RESILIENCE = Recorded("live_resilience", "resilience", "make_golden_resilience.py")
CLIENT = Recorded("live_client", "client", "make_golden_client.py")
