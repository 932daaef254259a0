#!/bin/bash
# GPU-box helper: sweep wf_trace's reservation rule (trace_reservation: smallest size kMin, share 1 / (waves * D)) on a workload.
# The variants are built beforehand, where the compiler is, one library per pair and the parent's rule beside them:
#   tools/build_variants.sh parent="-DYAFGPU_TRACE_BATCH_SHRINK=0 -DYAFGPU_TRACE_STATIC_FIRST=0 -DYAFGPU_TRACE_BATCH_MIN=64 -DYAFGPU_TRACE_BATCH_DIV=2" k64_d4="-DYAFGPU_TRACE_BATCH_MIN=64 -DYAFGPU_TRACE_BATCH_DIV=4" ...
# (add -DYAFGPU_TRACE_EXIT_LOG=1 for the libraries tools/exit_times.py reads).  Every library of the sweep runs in this one job,
# alternating, parent first in every round; the job stops at the first run that fails.
# usage: tools/sweep_batch.sh <outfile> <workload> <rounds> <name> ...      (names of libyafaray_amd/variants/<name>.so)
set -o pipefail
cd "$(dirname "$0")/.."
out="$1"; wl="$2"; rounds="$3"; shift 3
: > "$out"
for rep in $(seq 1 "$rounds"); do
for name in "$@"; do
	line=$(env YAFARAY_LIBRARY="$PWD/libyafaray_amd/variants/$name.so" timeout -k 10 300 python3 bench.py --gpus 1 --workload "$wl" --steps 60 --warmup 5 2>/dev/null | tail -1) || { echo "$wl $name $rep failed" | tee -a "$out"; exit 1; }
	echo "$wl $name $rep $(python3 -c 'import json, sys; d = json.loads(sys.argv[1]); print(d["value"], d["ms_per_step"])' "$line")" | tee -a "$out"
done; done
