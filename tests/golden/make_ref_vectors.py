#!/usr/bin/env python3
"""Record the compiled reference's answers on the inputs of the oracle-vs-reference tests
(tests/test_oracle_vs_ref.py, tests/test_oracle_consensus.py) into tests/golden/ref_vectors.json.gz.

Run from the repository root where oracle/_ref/libcrass_ref.so is built (oracle/Makefile, with the reference sources
present):
    python tests/golden/make_ref_vectors.py
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import orc, refvec                      # noqa: E402
from tests import test_oracle_consensus, test_oracle_vs_ref   # noqa: E402

if orc.ref() is None:
    sys.exit("oracle/_ref is not built: the reference's answers cannot be recorded here")
rec = {}
for mod in (test_oracle_vs_ref, test_oracle_consensus):
    rec.update(refvec.record(mod.RECORDS))
# (mtime 0: the same answers give the same file)
with open(refvec.PATH, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
    f.write(json.dumps(rec, sort_keys=True, separators=(",", ":")).encode())
print("%s: %d records" % (os.path.relpath(refvec.PATH, ROOT), len(rec)))
