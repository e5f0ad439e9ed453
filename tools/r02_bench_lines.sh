#!/bin/bash
# The committed bench lines of round 2 (run through gpurun; copy gpurun_out/r02lines/*.json into profiles/).
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out/r02lines
mkdir -p $O
cd $R
run() { n=$1; shift; timeout 400 "$@" 2>$O/$n.err | tail -1 > $O/r02_bench_$n.json; }
run default_driver python bench.py --full --steps 20 --warmup 5
run default python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline
CSPN_RESIDENT=off run default_multilaunch python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-train-leg --cold-sets 0
run sparse python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --sparse
run kitti python bench.py --full --workload kitti --steps 100 --warmup 10 --no-cpu-baseline
run pac5 python bench.py --full --workload pac5 --steps 100 --warmup 10 --no-cpu-baseline
run kitti_b1 python bench.py --full --workload kitti --batch 1 --steps 200 --warmup 20 --no-cpu-baseline
run nyu_b3 python bench.py --full --workload nyu --batch 3 --steps 200 --warmup 20 --no-cpu-baseline
run kitti_b1_graph python bench.py --full --workload kitti --batch 1 --steps 200 --warmup 20 --no-cpu-baseline --graph on --no-train-leg --no-per-step-leg --cold-sets 0
run nyu_b3_graph python bench.py --full --workload nyu --batch 3 --steps 200 --warmup 20 --no-cpu-baseline --graph on --no-train-leg --no-per-step-leg --cold-sets 0
CSPN_RESIDENT=off run kitti_b1_multilaunch python bench.py --full --workload kitti --batch 1 --steps 200 --warmup 20 --no-cpu-baseline --no-train-leg --no-per-step-leg --cold-sets 0
CSPN_RESIDENT=off run nyu_b3_multilaunch python bench.py --full --workload nyu --batch 3 --steps 200 --warmup 20 --no-cpu-baseline --no-train-leg --no-per-step-leg --cold-sets 0
run train_b3 python bench.py --full --workload train --steps 10 --warmup 3
for f in $O/*.json; do echo "$(basename $f): $(python -c "import json,sys; d=json.load(open('$f')); print(round(d['value']), d['ms_per_step'])")"; done
