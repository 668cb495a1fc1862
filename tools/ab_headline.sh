#!/bin/bash
# Same-box A/B of two builds of the native libraries: genomeworks_amd/lib (candidate) against genomeworks_amd/lib_old
# (baseline), alternating, headline only. usage (on the GPU box, repo root): bash tools/ab_headline.sh [rounds] [bench args]
# AB_BASELINE_ENV="NAME=VALUE ...": a same-binary A/B instead -- both arms run genomeworks_amd/lib, the baseline arm with these
# variables set (e.g. GW_POA_HOST_INPUT=0), and nothing is moved.
# Every bench run has its own time limit (AB_RUN_TIMEOUT seconds, default 300); the first run that fails ends the script.
ROUNDS=${1:-3}
shift
ARGS=${@:---sub-configs none --steps 20 --warmup 3 --no-cpu-baseline}
mkdir -p gpurun_out/ab
run() { # $1 = label, further arguments: NAME=VALUE for the run's environment
    label=$1; shift
    out=$(env "$@" timeout -k 10 ${AB_RUN_TIMEOUT:-300} python bench.py --full $ARGS 2>/dev/null)
    rc=$?
    [ $rc -ne 0 ] && { echo "$label: bench.py ended with status $rc"; return $rc; }
    printf '%s\n' "$out" | python -c "
import json,sys
d=json.loads([l for l in sys.stdin if l.startswith('{')][0])
print('$label', 'kernel_ms', d['roofline']['kernel_ms'], 'step_ms', d['ms_per_step'], 'gcups', d['value'], 'golden', d['equals_oracle_golden'])"
}
for i in $(seq $ROUNDS); do
    run candidate || exit 1
    if [ -n "${AB_BASELINE_ENV:-}" ]; then
        run baseline $AB_BASELINE_ENV || exit 1
        continue
    fi
    mv genomeworks_amd/lib genomeworks_amd/lib_new && mv genomeworks_amd/lib_old genomeworks_amd/lib
    run baseline; rc=$?
    mv genomeworks_amd/lib genomeworks_amd/lib_old && mv genomeworks_amd/lib_new genomeworks_amd/lib
    [ $rc -ne 0 ] && exit 1
done
exit 0
