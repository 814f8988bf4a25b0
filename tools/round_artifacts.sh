# Round artifacts: full bench (with cpu_baseline), kernel-trace stats, HBM PMC passes.
# usage: bash tools/round_artifacts.sh TAG
set -e
R=$GRAFT_REPO_ROOT; T=${1:-r01}
O=${OUT:-$R/bench_out}; mkdir -p $O
cd $R
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/${T}_pytest_gpu.log 2>&1
tail -1 $O/${T}_pytest_gpu.log
cd /tmp && export TMPDIR=/tmp
B="$R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-f32-leg"
timeout -k 10 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/${T}_pmcA -o run --output-format csv -- python3 $B > $O/${T}_pmcA.log 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/${T}_pmcB -o run --output-format csv -- python3 $B > $O/${T}_pmcB.log 2>&1
cd $R && python3 tools/pmcsum.py $O/${T}_pmc_summary.json $O/${T}_pmcA $O/${T}_pmcB > /dev/null
cp $O/${T}_pmc_summary.json profiles/pmc_summary.json
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/${T}_stats -o run --output-format csv -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-f32-leg > $O/${T}_stats_bench.json 2> $O/${T}_stats_bench.err
cd $R && timeout -k 10 400 python3 bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
cat $O/${T}_bench.json
python3 tools/profsum.py $O/${T}_stats > $O/${T}_kernel_summary.txt
head -8 $O/${T}_kernel_summary.txt
