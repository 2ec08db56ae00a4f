#!/bin/bash
# kernel timeline of one pair's settled steps (run ON the GPU box): tools/pair_trace.sh <tag> <base> <query>
set -e -o pipefail
TAG=${1:?tag}; BASE=${2:?base}; QUERY=${3:?query}
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${RJ_OUT:-$R/runs}; mkdir -p $OUT   # (raw outputs of the tools: git-ignored)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt_${BASE}_${QUERY} -o g -- python3 $R/bench.py --full --base $BASE --query $QUERY --no-cpu-baseline --no-secondary --steps 10 --warmup 5 > $OUT/${TAG}_kt_${BASE}_${QUERY}.log 2>&1
cd $R
python3 tools/trace_tables.py $OUT/${TAG}_kt_${BASE}_${QUERY}/g_kernel_trace.csv --steps 2 --skip 6 > $OUT/${TAG}_step_trace_${BASE}_${QUERY}.txt
python3 tools/trace_tables.py $OUT/${TAG}_kt_${BASE}_${QUERY}/g_kernel_trace.csv --regimes > $OUT/${TAG}_regimes_${BASE}_${QUERY}.csv
