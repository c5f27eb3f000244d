#!/usr/bin/env python3
"""Writes the inputs of tests/fastx_sets.py (regular, tile-edge, irregular, 300 random draws) into a directory, one file each, for
tools/sanitize/fastx_scan_main.cpp:   python3 tools/sanitize/fastx_scan_dump.py DIR"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import fastx_sets

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
T = 4096
sets = {"reg_" + k: v for k, v in fastx_sets.regular().items()}
sets.update({"edge_" + k: v for k, v in fastx_sets.tile_edge(T).items()})
sets.update({"irr_" + k: v[0] for k, v in fastx_sets.irregular(T).items()})
rng = random.Random(5)
sets.update({"rnd_%03d" % k: fastx_sets.random_input(rng) for k in range(300)})
for name, data in sets.items():
    with open(os.path.join(out, name + ".fx"), "wb") as f:
        f.write(data)
print(len(sets), "files in", out)
