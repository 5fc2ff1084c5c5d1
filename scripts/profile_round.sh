#!/bin/bash
# Round profile of one bench workload on the GPU box (run through gpurun from the repo root):
#   bash scripts/profile_round.sh r02 flat8g [brief]
# Writes raw rocprofv3 output under gpurun_out/prof_<tag>_<workload>/ ; scripts/summarize_profiles.py copies the summaries
# that DESIGN.md quotes into profiles/.  Counter passes are separate runs (never combined with tracing domains other than
# the kernel trace), in the order: timing (bench line) -> kernel trace/stats -> FETCH_SIZE -> FETCH_SIZE without the early
# exit (calibration of the counter on this access pattern) -> WRITE_SIZE -> SQ counters.  `brief` stops after the FETCH_SIZE
# passes (a before/after comparison of the bytes a kernel fetches needs no more).  A pass that fails or runs into its time
# limit ends the script: nothing more is started on a device that may have faulted.
set -u
TAG=${1:-r03}
WL=${2:-flat8g}
BRIEF=${3:-}
ROOT=$PWD
OUT=$ROOT/gpurun_out/prof_${TAG}_$WL
mkdir -p $OUT
export TMPDIR=/tmp
BENCH="python $ROOT/bench.py --workload $WL --steps 5 --warmup 1 --no-cpu-baseline --no-extra --no-variants --no-every-row --check 0"
pass() { # name, command ...
  local name=$1
  shift
  "$@" > $OUT/$name.log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then
    echo "profile_round.sh: pass $name ended with status $rc (see $OUT/$name.log): stopping" >&2
    exit $rc
  fi
}
cd /tmp
timeout -k 10 600 python $ROOT/bench.py --workload $WL --steps 10 --warmup 2 --full --no-extra > $OUT/bench.json 2> $OUT/bench.log
rc=$?
if [ $rc -ne 0 ]; then
  echo "profile_round.sh: the bench run ended with status $rc (see $OUT/bench.log): stopping" >&2
  exit $rc
fi
pass trace timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- $BENCH
pass pmc_fetch timeout -k 10 420 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- $BENCH
if [ "$WL" = flat8g ] || [ "$WL" = flat128g ]; then
  pass pmc_fetch_noee env GANON_HIP_ABLATE=early_exit timeout -k 10 420 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_noee -- $BENCH
fi
if [ "$BRIEF" != brief ]; then
  pass pmc_write timeout -k 10 420 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- $BENCH
  pass pmc_sq timeout -k 10 420 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_INSTS_LDS --output-format csv -d $OUT/pmc_sq -- $BENCH
fi
cd $ROOT
python scripts/summarize_profiles.py $TAG $WL
rc=$?
if [ $rc -ne 0 ]; then
  echo "profile_round.sh: summarize_profiles.py ended with status $rc: profiles/ was not refreshed" >&2
fi
exit $rc
