"""Answers of the compiled reference (oracle/_ref) on the inputs the oracle-vs-reference tests draw, recorded in
tests/golden/ref_vectors.json.gz by tests/golden/make_ref_vectors.py where the reference sources are present.

The tests check the oracle against these recorded answers everywhere, and the recording itself against the live
reference library wherever oracle/_ref is built, so the suite needs nothing outside the repository."""
import gzip
import hashlib
import json
import os

from tests import orc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors.json.gz")
_cache = None


def digest(cases):
    """stable digest of a test's input stream (bytes shown as hex)"""
    def enc(x):
        if isinstance(x, (bytes, bytearray)):
            return "b:" + bytes(x).hex()
        if isinstance(x, (list, tuple)):
            return [enc(y) for y in x]
        return x
    return hashlib.sha256(json.dumps(enc(cases), separators=(",", ":")).encode()).hexdigest()


def plain(x):
    """tuples -> lists, as the answers come back from JSON"""
    return json.loads(json.dumps(x))


def load():
    global _cache
    if _cache is None:
        with gzip.open(PATH, "rt") as f:
            _cache = json.load(f)
    return _cache


def answers(name, cases, live=None):
    """the reference's recorded answers for `cases` (checked against live(cases) where oracle/_ref is built)"""
    rec = load()[name]
    assert rec["inputs"] == digest(cases), (
        "%s: the test's input stream no longer matches the recording; re-record with tests/golden/make_ref_vectors.py" % name)
    got = live(cases) if live is not None and orc.ref() is not None else None
    if got is not None:
        assert plain(got) == rec["answers"], "%s: the live reference disagrees with the recording" % name
    return rec["answers"]


def record(records):
    """{name: (inputs function, live function)} -> {name: {"inputs": digest, "answers": ...}} (needs oracle/_ref)"""
    out = {}
    for name, (cases_fn, live) in records.items():
        cases = cases_fn()
        got = live(cases)
        assert got is not None, name
        out[name] = {"inputs": digest(cases), "answers": plain(got)}
    return out
