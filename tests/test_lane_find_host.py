"""The lane kernel's packed seed find (crass_amd/csrc/lane_find.h: find_packed) against the serial rule it replaces, on the
host: tools/lane_find_main.cpp holds both, runs every designed case (a match at offset 0, at npos - 1, at npos only, at t and
t + 8, poly-A against the zero bases past a read's end, npos == 1, every plen, every chunk count) and a million random draws of
which about half match, and exits non-zero on the first difference.  Built here with the host compiler.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("lane_find") / "lane_find_main")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "crass_amd", "csrc"),
                           os.path.join(ROOT, "tools", "lane_find_main.cpp"), "-o", out])
    return out


def test_packed_find_is_the_serial_rule(program):
    r = subprocess.run([program, "1000000"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"lane_find ok: (\d+) designed cases, (\d+) random draws \((\d+) with a match\)", r.stdout)
    assert m, r.stdout
    n_designed, n_random, n_match = map(int, m.groups())
    assert n_designed >= 5000 and n_random >= 1000000
    assert 0.35 * n_random <= n_match <= 0.65 * n_random          # about half the draws match
