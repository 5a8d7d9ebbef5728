#!/bin/bash
# rocprofv3 kernel trace of the bench command with its side measurements (bench.py --full, no CPU baseline), on an MI355X.
# Usage: tools/prof_bench.sh OUT_DIR  ->  OUT_DIR/bench_under_rocprof.json, OUT_DIR/bench_kernel_summary.txt
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "${1:?usage: tools/prof_bench.sh OUT_DIR}"
out="$(cd "$1" && pwd)"
export SELAVI_TUNE_CACHE="$out/tune.json"
python "$R/bench.py" --steps 2 --warmup 1 --full --no-cpu-baseline > "$out/pre.log" 2>&1      # fills the tune cache so the trace holds no timing passes
rm -rf "$out/trace"
rocprofv3 --kernel-trace --stats -d "$out/trace" -o out -- python "$R/bench.py" --steps 10 --warmup 3 --full --no-cpu-baseline > "$out/bench_under_rocprof.json" 2> "$out/bench.err"
python "$R/tools/rocprof_summary.py" "$(find "$out/trace" -name "*.db" | head -1)" 70 > "$out/bench_kernel_summary.txt" 2>&1
head -12 "$out/bench_kernel_summary.txt"
