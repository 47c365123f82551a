"""The live reference's results for the Client tests, recorded under tests/golden/live_client/ by
tests/golden/make_golden_client.py (run where the reference is installed).  `get(name, *args)` returns what the reference computed
for that key when it was recorded -- the same dicts of integers, floats and arrays, bit for bit.  A key without a recording raises
KeyError with the key's name: a test that needs it fails by name, it is never skipped.  Format and part size limit as
tests/fault_reference.py (MAX_PART_BYTES)."""
from __future__ import annotations

import glob
import json
import os
import zlib

import numpy as np

from fault_reference import MAX_PART_BYTES, PART_BYTES
from reference_runs import GOLDEN_DIR, _decode, _encode, _key

REC_DIR = os.path.join(GOLDEN_DIR, "live_client")
_store = None


def key(name, *args):
    return _key("client:" + name, args)


def _load():
    global _store
    if _store is None:
        _store = {}
        for path in sorted(glob.glob(os.path.join(REC_DIR, "*.npz"))):
            with np.load(path, allow_pickle=False) as z:
                index = json.loads(bytes(z["index"]).decode())
                for k, (skeleton, names) in index.items():
                    _store[k] = (skeleton, [z[n] for n in names])
    return _store


def get(name, *args):
    k = key(name, *args)
    try:
        skeleton, arrays = _load()[k]
    except KeyError:
        what = f"{name}{tuple(a.get('name', '...') if isinstance(a, dict) else a for a in args)!r}"[:160]
        raise KeyError(f"no recorded reference result for {what} (key {k}): run tests/golden/make_golden_client.py where the "
                       "reference is installed") from None
    return _decode(skeleton, arrays)


def write(cases):
    """{key: result} -> tests/golden/live_client/part_NNN.npz, replacing what was there."""
    os.makedirs(REC_DIR, exist_ok=True)
    for path in glob.glob(os.path.join(REC_DIR, "*.npz")):
        os.remove(path)
    part, index, size, n = {}, {}, 0, 0

    def flush():
        nonlocal part, index, size, n
        if index:
            part["index"] = np.frombuffer(json.dumps(index, separators=(",", ":")).encode(), np.uint8)
            np.savez_compressed(os.path.join(REC_DIR, f"part_{n:03d}.npz"), **part)
            n += 1
        part, index, size = {}, {}, 0

    for k in sorted(cases):
        arrays = []
        skeleton = _encode(cases[k], arrays)
        est = len(zlib.compress(json.dumps(skeleton).encode())) + sum(
            len(zlib.compress(np.ascontiguousarray(a).tobytes())) for a in arrays) + 256 * (len(arrays) + 1)
        if index and size + est > PART_BYTES:
            flush()
        names = [f"{k}_{i}" for i in range(len(arrays))]
        for nm, a in zip(names, arrays):
            part[nm] = np.asarray(a)
        index[k] = (skeleton, names)
        size += est
    flush()
    for path in glob.glob(os.path.join(REC_DIR, "*.npz")):
        assert os.path.getsize(path) <= MAX_PART_BYTES, (path, os.path.getsize(path))
