#!/bin/bash
# GPU box: interleaved A/B of the plain bench line (one timed region per run) under library
# and environment variants.  Stops at the first failing run.
#   bash tools/bench_ab.sh OUTDIR ROUNDS "label|lib.so|VAR=val,VAR=val" ... -- [bench args]
# An empty lib runs the product library.  One line per run: label, round, ms_per_step, value,
# also appended to OUTDIR/ab.txt (stderr of the runs: OUTDIR/err.txt).
# (profiles/step_shards/: FFM_STEP_SHARDS=1..4 against the parent's library.)
set -o pipefail
export TMPDIR=/tmp
OUT=$1; ROUNDS=$2; shift 2
ENTRIES=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do ENTRIES+=("$1"); shift; done
[ "$1" == "--" ] && shift
mkdir -p "$OUT"
pick='import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print("%.5f ms_per_step %.4f Gas/s" % (d["ms_per_step"], d["value"]/1e9))'
for r in $(seq 1 $ROUNDS); do
  for ent in "${ENTRIES[@]}"; do
    IFS='|' read -r label lib kv <<< "$ent"
    kv=${kv//,/ }
    libenv=""; [ -n "$lib" ] && libenv="FFM_LIB_PATH=$PWD/$lib"
    v=$(env $kv $libenv timeout -k 10 120 python3 bench.py --gpus 1 "$@" 2>>"$OUT/err.txt" | python3 -c "$pick") || { echo "FAILED $label round $r"; tail -5 "$OUT/err.txt"; exit 1; }
    echo "$label round$r $v" | tee -a "$OUT/ab.txt"
  done
done
