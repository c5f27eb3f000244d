"""Writes the gzip sets of tests/gzip_sets.py into a directory for tools/sanitize/gzip_main.cpp: every regular file once per chunk
size, the declined files and the seeded bit flips at theirs; the chunk size and the expected reason are part of the name
(NAME.c<chunk>.r<reason>.gz; r-1 for the flips: whatever comes).
    python3 tools/sanitize/gzip_dump.py DIR"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import gzip_sets  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
files = {}
for k, (v, text) in gzip_sets.regular().items():
    for c in gzip_sets.CHUNKS:
        files["r_%s.c%d.r0" % (k, c)] = v
files.update({"d_%s.c%d.r%d" % (k, c, r): v for k, (v, c, r) in gzip_sets.declined().items()})
files.update({"a_%s.c%d.r0" % (k, c): v for k, (v, c, text) in gzip_sets.accepted_at_a_larger_chunk().items()})
files.update({"f_%03d.c%d.r-1" % (i, gzip_sets.FLIP_CHUNK): v for i, v in enumerate(gzip_sets.bit_flips())})
for k, v in files.items():
    with open(os.path.join(out, k + ".gz"), "wb") as f:
        f.write(v)
print(len(files), "files in", out)
