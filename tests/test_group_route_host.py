"""The router and the gatherer of a group's fetches (crass_amd/csrc/group_route.h: route, scatter, gather) against the obvious
per-index loop, on the host: tools/sanitize/group_route_main.cpp holds both and runs 1 to 5 ranks with shards of 0, 1 and a few
records in every arrangement (empty first, middle and last ranks), no index, every index once in a random order, 300 random
indices with repeats, an index base of 0 and of 77, local and global indices, and a carried string for some records of a rank's
first part; it exits non-zero on the first difference.  Built here with the host compiler.  No GPU needed."""
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
    out = str(tmp_path_factory.mktemp("group_route") / "group_route_main")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "crass_amd", "csrc"),
                           os.path.join(ROOT, "tools", "sanitize", "group_route_main.cpp"), "-o", out])
    return out


def test_route_and_gather_are_the_per_index_loop(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"group_route ok: (\d+) jobs, (\d+) fetches", r.stdout)
    assert m, r.stdout
    n_jobs, n_fetches = map(int, m.groups())
    assert n_jobs == 3 + 9 + 27 + 81 + 243                 # every arrangement of {0, 1, 4} records over 1 .. 5 ranks
    assert n_fetches == 4 * (3 * n_jobs - 2 * 5)           # (the all-empty job of every rank count has the empty pick only)
