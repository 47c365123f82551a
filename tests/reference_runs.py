"""The upstream reference's results for the CPU tests that compare against it, recorded under tests/golden/live_reference/.

`REF.run_case(spec)` (and every other run function of tests/golden/make_golden.py) returns what the live reference computed for
that spec when it was recorded: the same `(out, meta)` values, bit for bit (every run is seeded).  `REF.value(name, fn)` does the
same for a zero-argument function that reads the reference directly (constructor defaults, presets, printed summaries).  The
tests therefore need nothing outside the repository.

To re-record after a change to the specs or to make_golden.py, run the tests that use REF where the reference is installed
(tests/golden/refshim.py: HS_REFERENCE_ROOT) with HS_RECORD_REFERENCE=1:

    HS_RECORD_REFERENCE=1 python -m pytest tests/test_oracle_live_reference.py tests/test_host_api.py -m live_reference

Every result computed in that session replaces the recording in tests/golden/live_reference/ when the session ends.  A spec with
no recorded result fails its test by name; it is never skipped.
"""
from __future__ import annotations

import atexit
import glob
import hashlib
import json
import os
import sys
import zlib

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REC_DIR = os.path.join(GOLDEN_DIR, "live_reference")
RECORD = os.environ.get("HS_RECORD_REFERENCE") == "1"
PART_BYTES = 900 * 1024                 # compressed bytes per file (every committed file stays under 1 MiB)


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


def _make_golden():
    """tests/golden/make_golden.py, which imports the live reference (recording only)."""
    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden

    return make_golden


class _Recorded:
    def __init__(self):
        self._loaded = None
        self._fresh = {}

    def _store(self):
        if self._loaded is None:
            self._loaded = {}
            for path in sorted(glob.glob(os.path.join(REC_DIR, "*.npz"))):
                with np.load(path, allow_pickle=False) as z:
                    index = json.loads(bytes(z["index"]).decode())
                    for key, (skeleton, names) in index.items():
                        self._loaded[key] = (skeleton, [z[n] for n in names])
        return self._loaded

    def _lookup(self, key, what):
        try:
            skeleton, arrays = self._store()[key]
        except KeyError:
            raise KeyError(f"no recorded reference result for {what} (key {key}): re-record with HS_RECORD_REFERENCE=1 "
                           "(tests/reference_runs.py)") from None
        return _decode(skeleton, arrays)

    def _record(self, key, result):
        arrays = []
        skeleton = _encode(result, arrays)
        self._fresh[key] = (skeleton, arrays)
        return _decode(skeleton, arrays)        # the caller sees exactly what a replay returns

    def value(self, name, fn):
        """What `fn()` returned on the live reference when it was recorded."""
        key = _key("value:" + name, ())
        if not RECORD:
            return self._lookup(key, name)
        _make_golden()                          # (installs the reference's import path)
        return self._record(key, fn())

    def attr(self, name):
        """make_golden.<name> (a constant) as recorded."""
        return self.value("attr:" + name, lambda: getattr(_make_golden(), name))

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def run(*args):
            key = _key(name, args)
            if not RECORD:
                return self._lookup(key, f"{name}{tuple(args)!r}"[:200])
            return self._record(key, getattr(_make_golden(), name)(*args))

        return run

    def _save(self):
        """Write every result recorded in this session, merged over the stored ones, into files of at most PART_BYTES."""
        if not self._fresh:
            return
        stored = self._store()
        if not any(key in stored for key in self._fresh):
            # only new results: new part files behind the stored ones, which stay byte for byte as they are
            n0 = len(glob.glob(os.path.join(REC_DIR, "*.npz")))
            self._write_parts(self._fresh, n0)
            return
        cases = {}
        for key, (skeleton, arrays) in self._store().items():
            cases[key] = (skeleton, arrays)
        cases.update(self._fresh)
        os.makedirs(REC_DIR, exist_ok=True)
        for path in glob.glob(os.path.join(REC_DIR, "*.npz")):
            os.remove(path)
        self._write_parts(cases, 0)

    @staticmethod
    def _write_parts(cases, first):
        """cases -> part_<first>.npz, part_<first + 1>.npz, ... of at most PART_BYTES each."""
        os.makedirs(REC_DIR, exist_ok=True)
        part, index, size, n = {}, {}, 0, first

        def flush():
            nonlocal part, index, size, n
            if index:
                part["index"] = np.frombuffer(json.dumps(index, separators=(",", ":")).encode(), np.uint8)
                np.savez_compressed(os.path.join(REC_DIR, f"part_{n:03d}.npz"), **part)
                n += 1
            part, index, size = {}, {}, 0

        for key in sorted(cases):
            skeleton, arrays = cases[key]
            est = len(zlib.compress(json.dumps(skeleton).encode())) + sum(
                len(zlib.compress(np.ascontiguousarray(a).tobytes())) for a in arrays) + 256 * (len(arrays) + 1)
            if index and size + est > PART_BYTES:
                flush()
            names = [f"{key}_{i}" for i in range(len(arrays))]
            for nm, a in zip(names, arrays):
                part[nm] = np.asarray(a)
            index[key] = (skeleton, names)
            size += est
        flush()


REF = _Recorded()
if RECORD:
    atexit.register(REF._save)
