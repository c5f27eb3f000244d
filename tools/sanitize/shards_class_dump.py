#!/usr/bin/env python3
"""The designed jobs of tests/shard_wrapped_sets.py as files for tools/sanitize/shards_class_main.cpp: python3 shards_class_dump.py DIR.
Job k's file j is DIR/jKKK_J.bin; the program takes the files of one job as one set (the names sort in order)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import shard_wrapped_sets as S      # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
jobs = [v[0] for _, v in sorted(S.cases().items())] + [v[0] for _, v in sorted(S.declined().items())] + [S.four_line_job()]
for k, files in enumerate(jobs):
    for j, data in enumerate(files):
        with open(os.path.join(out, "j%03d_%d.bin" % (k, j)), "wb") as f:
            f.write(data)
print("%d jobs" % len(jobs))
