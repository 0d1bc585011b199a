#!/bin/bash
# Interleaved same-box A/B of two builds of the library: bash tools/ab/ab_libs.sh <libA.so> <libB.so> [rounds] [bench.py arguments ...]
# (MLSP_HIP_LIB selects the library; every run has its own time limit, and the first run that fails ends the script)
A=$1; B=$2; R=${3:-3}
shift 3 2>/dev/null || shift $#
for i in $(seq $R); do
  for l in $A $B; do
    printf "%s " "$l"
    MLSP_HIP_LIB=$l timeout -k 10 300 python bench.py --no-cpu-baseline --no-secondary --no-fp32-leg "$@" 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('%.3f ms/step' % d['ms_per_step'])" || exit 1
  done
done
