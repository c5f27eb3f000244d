#!/bin/bash
# Hardware counters of the kernels matching a pattern, in a counters-only run of bench.py (no tracing beside it):
#   tools/pmc_counters.sh <out dir> <kernel regex> "<counter names>" [bench.py arguments ...]
# Counters that `rocprofv3 --list-avail` does not offer are named as missing and left out of the run.  BENCH=<path> measures
# another tree's bench.py (an A/B against a parent build).  Prints, per matching kernel and grid, each counter's average per launch.
set -u
out=$1; pat=$2; want=$3; shift 3
here=$(cd "$(dirname "$0")/.." && pwd)
bench=${BENCH:-$here/bench.py}
mkdir -p "$out"
if [ ! -s "$out/list_avail.txt" ]; then timeout -k 10 120 rocprofv3 --list-avail > "$out/list_avail.txt" 2>&1; fi
have=""
for c in $want; do
  if grep -q -w "$c" "$out/list_avail.txt"; then have="$have $c"; else echo "counter $c: not offered by this machine (missing)"; fi
done
[ -n "$have" ] || { echo "no counter of the list is available"; exit 2; }
cd "$(dirname "$bench")" || exit 2
TMPDIR=/tmp timeout -k 10 420 rocprofv3 --pmc $have --output-format csv -d "$out/rp" -o r -- python3 "$bench" "$@" > "$out/bench.json" 2> "$out/err.txt"
rc=$?
[ $rc -eq 0 ] || { echo "rocprofv3 run ended with status $rc"; tail -5 "$out/err.txt"; exit $rc; }
f=$(find "$out/rp" -name "*counter_collection.csv" | head -1); [ -n "$f" ] && cp "$f" "$out/pmc.csv"; rm -rf "$out/rp"
python3 - "$out/pmc.csv" "$pat" <<'PY'
import csv, sys, collections, re
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(sys.argv[1])):
    k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("crass::", "")
    if re.search(sys.argv[2], k): acc[k + " grid=" + r.get("Grid_Size", "?")][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, v in acc.items():
    print(k, {c: round(sum(x) / len(x)) for c, x in v.items()}, "launches", len(next(iter(v.values()))))
PY
