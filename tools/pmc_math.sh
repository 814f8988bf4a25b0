# SQ counters of the headline Trainer step in one math (x6 | x3 | bf16), one rocprofv3 run of its own
# per math (counters only, beside the kernel trace that names the launches); per-kernel sums →
# OUT/pmc_math_<math>.json. usage: bash tools/pmc_math.sh OUT MATH [MATH ...]
set -e
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "$1" && cd "$1" && pwd); shift
for M in "$@"; do
  (cd /tmp && TMPDIR=/tmp timeout -s KILL 240 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU SQ_INSTS_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY \
     -d "$O/pmc_$M" -o run --output-format csv -- python3 "$R/tools/math_bench.py" --only "$M" > "$O/pmc_$M.log" 2>&1)
  python3 "$R/tools/pmc_math_sum.py" "$O/pmc_$M" "$O/pmc_math_$M.json"
done
