set -e
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$ROOT/gpurun_out
cd /tmp && export TMPDIR=/tmp
for wl in partseg pointnet_bin pointnet_fp; do
  rocprofv3 --kernel-trace -d $OUT/wl_$wl -o run --output-format csv -- python3 $ROOT/bench.py --full --workload $wl --no-cpu-baseline --steps 6 --warmup 2 > $OUT/wl_$wl.log 2>&1
  python3 $ROOT/tools/step_trace.py $(find $OUT/wl_$wl -name "*kernel_trace.csv" | head -1) > $OUT/wl_${wl}_step_kernels.txt
  python3 $ROOT/tools/step_trace.py $(find $OUT/wl_$wl -name "*kernel_trace.csv" | head -1) x > $OUT/wl_${wl}_step_sequence.txt
  rm -rf $OUT/wl_$wl
done
