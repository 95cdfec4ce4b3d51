#!/bin/bash
# HBM traffic of the train step's kernels: FETCH_SIZE and WRITE_SIZE in separate passes (MI355X_MICROARCH.md, HBM section)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${1:?usage: tools/pmc_traffic.sh <absolute output dir>  (then: python tools/pmc_traffic_summary.py <that dir>)}; mkdir -p $O
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $C --kernel-trace -d $O/$C -o out --output-format csv -- python3 $R/bench.py --full --no-secondary --no-cpu-baseline --steps 6 --warmup 2 --no-graph > $O/$C.log 2>&1 || exit 1
done
