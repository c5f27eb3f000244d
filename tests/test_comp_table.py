"""crass_amd/csrc/comp_table.h: the one reverse-complement table of host and device code.  The 128 expected bytes were printed
by build_comp_table (merge.cpp) of the commit before the header existed; they are a record, not computed from the header."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crass_amd", "csrc")

EXPECTED = bytes.fromhex(
    "000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"
    "202122232425262728292a2b2c2d2e2f303132333435363738393a3b3c3d3e3f"
    "405456474845464344494a4d4c4b4e4f505159534141425758525a5b5c5d5e5f"
    "407476676865666364696a6d6c6b6e6f707179736161627778727a7b7c7d7e7f")

PROGRAM = r"""
#include <cstdio>
#include "comp_table.h"
static_assert(sizeof(crass::CompTable) == 128, "one byte per 7-bit code");
int main() { return fwrite(crass::kCompTable.v, 1, 128, stdout) == 128 ? 0 : 1; }
"""


def test_header_table_is_the_recorded_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "table.cpp", tmp_path / "table"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    got = subprocess.run([str(exe)], capture_output=True, check=True).stdout
    assert len(EXPECTED) == 128 and len(got) == 128
    assert [i for i in range(128) if got[i] != EXPECTED[i]] == []


def test_no_upload_is_left():
    for root, _, files in os.walk(CSRC):
        if os.path.basename(root) == "_obj":
            continue
        for f in files:
            if f.endswith((".hip", ".cpp", ".h")):
                text = open(os.path.join(root, f), errors="replace").read()
                assert "upload_comp_table" not in text and "upload_fetch_comp_table" not in text, f
