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
import os
import sys

from recorded import GOLDEN_DIR, _decode, _encode, _key, read_parts, write_parts

REC_DIR = os.path.join(GOLDEN_DIR, "live_reference")
RECORD = os.environ.get("HS_RECORD_REFERENCE") == "1"
PART_BYTES = 900 * 1024                 # compressed bytes per file (every committed file stays under 1 MiB)


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
            self._loaded = read_parts(REC_DIR)
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
            write_parts(REC_DIR, self._fresh, PART_BYTES, first=len(glob.glob(os.path.join(REC_DIR, "*.npz"))))
            return
        write_parts(REC_DIR, {**stored, **self._fresh}, PART_BYTES)


REF = _Recorded()
if RECORD:
    atexit.register(REF._save)
