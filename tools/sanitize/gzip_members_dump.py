"""Writes the sets of tests/gzip_member_sets.py (plain gzip of several members) into a directory for
tools/sanitize/gzip_members_main.cpp: every regular file once per chunk size, the declined files and the seeded bit flips at theirs;
the chunk size and the expected reason are part of the name (NAME.c<chunk>.r<reason>.gz; r-1 for the flips: whatever comes).
    python3 tools/sanitize/gzip_members_dump.py DIR"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import gzip_member_sets as sets  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
files = {}
for k, v in sets.regular().items():
    for c in sets.CHUNKS:
        files["r_%s.c%d.r0" % (k, c)] = v
for k, (v, text) in sets.fastx_members().items():
    files["x_%s.c0.r0" % k] = v
files.update({"d_%s.c%d.r%d" % (k, c, r): v for k, (v, c, r, m) in sets.declined()[0].items()})
files.update({"f_%03d.c%d.r-1" % (i, sets.FLIP_CHUNK): v for i, v in enumerate(sets.bit_flips())})
for k, v in files.items():
    with open(os.path.join(out, k + ".gz"), "wb") as f:
        f.write(v)
print(len(files), "files in", out)
