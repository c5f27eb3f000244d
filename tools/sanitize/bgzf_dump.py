"""Writes the BGZF sets of tests/bgzf_sets.py into a directory, one file each, for tools/sanitize/bgzf_main.cpp: the expected member
and reason are part of the name (NAME.m<member>.r<reason>.bgzf; the seeded bit flips carry none: NAME.bgzf).
    python3 tools/sanitize/bgzf_dump.py DIR"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import bgzf_sets  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
files = {"r_%s.m0.r0" % k: v for k, v in bgzf_sets.regular().items()}
files.update({"d_%s.m%d.r%d" % (k, m, r): v for k, (v, m, r) in bgzf_sets.damaged().items()})
files.update({"n_%s.m%d.r%d" % (k, m, bgzf_sets.NOT_BGZF): v for k, (v, m, pos) in bgzf_sets.not_bgzf().items()})
files.update({"f_%03d" % i: v for i, (v, m) in enumerate(bgzf_sets.bit_flips())})
for k, v in files.items():
    with open(os.path.join(out, k + ".bgzf"), "wb") as f:
        f.write(v)
print(len(files), "files in", out)
