# One pass at the end of a work block, on the GPU box: GPU tests, smoke, kernel-trace stats, HBM and SQ counter passes, then the
# full bench (after the HBM pass, so that its roofline.traffic quotes a profile of this very build).
#   bash scripts/round_end_pass.sh r03b tests      GPU tests + smoke (~9 min)
#   bash scripts/round_end_pass.sh r03b profiles   traces, counter passes, bench.py --full (~10 min)
# Outputs go to $PASS_OUT (default: pass_out/ in the repo root).
# Every step's exit status is recorded in $PASS_OUT/<tag>_steps_<what>.txt and the script exits non-zero if any step failed
# (a failed pytest must not leave a "complete" profile set behind).
set -u
T=$1
WHAT=${2:-all}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
export PASS_OUT=${PASS_OUT:-$ROOT/pass_out}
OUT=$PASS_OUT
mkdir -p "$OUT"
export TMPDIR=/tmp
FAIL=0
: > $OUT/${T}_steps_${WHAT}.txt
step() { local name=$1; shift; "$@"; local rc=$?; echo "$name rc=$rc" >> $OUT/${T}_steps_${WHAT}.txt; [ $rc -ne 0 ] && FAIL=1; return 0; }
if [ "$WHAT" != profiles ]; then
step gpu_tests bash -c "timeout -k 10 900 python -m pytest tests -m gpu -q --timeout=500 -p no:cacheprovider > $OUT/${T}_gpu_tests.log 2>&1"; tail -3 $OUT/${T}_gpu_tests.log
# (smoke() on the prebuilt library: `make` on the box would rebuild everything when file times do not survive the copy)
step smoke bash -c "timeout -k 10 300 python -c \"import __graft_entry__ as g; g.smoke()\" > $OUT/${T}_smoke.log 2>&1"; tail -1 $OUT/${T}_smoke.log
fi
if [ "$WHAT" != tests ]; then
Q="--steps 4 --warmup 2 --no-extras --no-cpu-baseline --no-parity --no-pdip --no-host-io"
step kernel_trace bash -c "cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_kt -- python3 $ROOT/bench.py $Q > $OUT/${T}_cdu_bench_under_rocprof.json 2> $OUT/${T}_kt.err"
find $OUT/${T}_kt -name '*kernel_stats.csv' -exec cp {} $OUT/${T}_cdu_b100000_kernel_stats.csv \;
find $OUT/${T}_kt -name '*kernel_trace.csv' -exec cp {} $OUT/${T}_cdu_b100000_kernel_trace.csv \;
python3 scripts/timeline.py $OUT/${T}_cdu_b100000_kernel_trace.csv > $OUT/${T}_cdu_b100000_timeline.txt 2>/dev/null
step pmc_hbm bash -c "timeout -k 10 400 bash scripts/pmc_hbm.sh cdu_b100000 --steps 1 --warmup 2 --no-extras --no-cpu-baseline --no-parity --no-pdip --no-host-io"; cp profiles/pmc_hbm_cdu_b100000.json $OUT/
step pmc_hbm_nn bash -c "timeout -k 10 300 bash scripts/pmc_hbm.sh nn_b1048576 --workload nn --steps 1 --warmup 1"; cp profiles/pmc_hbm_nn_b1048576.json $OUT/ 2>/dev/null
step pmc_hbm_cstrs bash -c "timeout -k 10 300 bash scripts/pmc_hbm.sh cstrs_b10000 --workload cstrs --batch 10000 --steps 2 --warmup 1 --no-extras --no-cpu-baseline --no-parity --no-pdip --no-host-io"; cp profiles/pmc_hbm_cstrs_b10000.json $OUT/ 2>/dev/null
step pmc_sq bash -c "timeout -k 10 400 bash scripts/pmc_sq.sh ${T} --steps 1 --warmup 2 --no-extras --no-cpu-baseline --no-parity --no-pdip --no-host-io"; cp profiles/${T}_pmc_sq.json $OUT/
step bench bash -c "NNMPC_BENCH_DETAIL=$OUT/${T}_bench_detail.json timeout -k 10 700 python bench.py --full > $OUT/${T}_cdu_b100000_bench.json 2> $OUT/${T}_bench.err"; tail -c 300 $OUT/${T}_bench.err
fi
rm -rf $OUT/${T}_kt $OUT/pmc_hbm_cdu_b100000 $OUT/pmc_hbm_nn_b1048576 $OUT/pmc_hbm_cstrs_b10000 $OUT/pmc_${T} $OUT/${T}_cdu_b100000_kernel_trace.csv
cat $OUT/${T}_steps_${WHAT}.txt
exit $FAIL
