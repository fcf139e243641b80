#!/bin/bash
# round 6: workgroups per cell (qsplit) of analog_f1_mean_kernel for weight_analogs (measured for the regression and the plain mean before)
export SD_DOWNSCALE_LIB=$PWD/scikit-downscale_amd/lib/libsd_downscale_dev.so
run() {  # label, extra bench args
  local label=$1; shift
  timeout 300 python bench.py --full --config 4 --steps ${STEPS:-4} --warmup 1 --no-cpu-baseline "$@" 2>/dev/null | python -c "
import json,sys;d=json.loads(sys.stdin.readline());r=d['roofline'];print('$label', round(d['ms_per_step'],2), 'ms', round(d['value']/1e6,3), 'M cells/s', round(r['frac'],4), {k: round(v*r['launches_per_step'][k],2) for k,v in r['per_kernel_avg_ms'].items()})"
}
for qs in 1 2 4; do
  SD_ANALOG_QSPLIT=$qs run "weight qsplit=$qs" --analog-kind weight_analogs --parity-only
done
for qs in 1 2 4; do
  SD_ANALOG_QSPLIT=$qs run "regr   qsplit=$qs" --analog-estimator regression --parity-only
done
