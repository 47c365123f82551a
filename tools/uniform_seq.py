#!/usr/bin/env python3
"""Run the repeatability sequences of tests/uniform_cases.py (every uniform-grid kernel, ten times each, between engines of other
sizes, each run against the C oracle) in ONE process and say which runs differ.  tests/test_gpu_uniform_kernels_oracle.py runs it in
a fresh process with HS_POISON_ALLOC set: nothing an engine reads may depend on what the allocator hands out.
usage: uniform_seq.py [repeats]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import uniform_cases as U

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
n = 0
bad = []
for which in range(len(U.REPEAT_LOADS)):
    try:
        runs, b = U.repeat_sequence(which, repeats)
        n += runs
        bad += b
    except Exception as e:  # noqa
        n += 1
        bad.append(f"EXC {type(e).__name__}: {str(e)[:300]}")
for b in bad:
    print(b)
print("n =", n, "bad =", len(bad))
