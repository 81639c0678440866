#!/bin/bash
# Regenerates the evidence under profiles/ on a GPU box (run from the repo root): bash scripts/profile_round.sh TAG OUT_DIR
#   kernel-trace stats of the bench command, the two PMC passes (never combined with other trace domains), the un-profiled
#   bench line, the per-layer sweep.  Every bench run is a --full one (breakdown legs, synthesiser roofline; the un-profiled
#   line also the CPU baseline).  Outputs land in OUT_DIR; copy what is to be judged into profiles/.
set -e
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
TAG=${1:-r01}
OUT=${2:?usage: profile_round.sh TAG OUT_DIR}
mkdir -p "$OUT"
python scripts/layer_sweep.py > $OUT/${TAG}_layer_sweep.txt 2>&1
python scripts/layer_sweep.py --math fp32 > $OUT/${TAG}_layer_sweep_direct_kernels.txt 2>&1
python bench.py --steps 4 --warmup 1 --full 2> $OUT/${TAG}_bench.err | tail -1 > $OUT/${TAG}_bench.json.log
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/${TAG}_prof.log 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmc_fetch -- python3 bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/${TAG}_pmc_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_pmc_write -- python3 bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/${TAG}_pmc_write.log 2>&1
python scripts/pmc_traffic.py $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write $OUT/${TAG}_pmc_traffic.json > $OUT/${TAG}_pmc_summary.log 2>&1
find $OUT/${TAG}_pmc_fetch $OUT/${TAG}_pmc_write -name "*counter_collection.csv" -delete
rocprofv3 --kernel-trace --pmc MfmaUtil GRBM_GUI_ACTIVE --output-format csv -d $OUT/${TAG}_pmc_mfma -- python3 bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/${TAG}_pmc_mfma.log 2>&1
python scripts/pmc_mfma_util.py $OUT/${TAG}_pmc_mfma $OUT/${TAG}_pmc_mfma_util.json > $OUT/${TAG}_pmc_mfma_summary.log 2>&1
find $OUT/${TAG}_pmc_mfma -name "*.csv" -delete
rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE --output-format csv -d $OUT/${TAG}_pmc_lds -- python3 bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/${TAG}_pmc_lds.log 2>&1
python scripts/pmc_lds.py $OUT/${TAG}_pmc_lds $OUT/${TAG}_pmc_lds.json > $OUT/${TAG}_pmc_lds_summary.log 2>&1
find $OUT/${TAG}_pmc_lds -name "*.csv" -delete
find $OUT/${TAG}_prof -name "*kernel_trace.csv" -delete
cp $OUT/${TAG}_prof/*/*kernel_stats.csv $OUT/${TAG}_bench_kernel_stats.csv
echo profiled
