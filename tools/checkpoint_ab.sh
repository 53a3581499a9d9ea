#!/bin/bash
# bench.py of the parent commit's tree and of this tree in alternating processes on one device (profiles/checkpoint/bench_ab.jsonl).
# usage: tools/checkpoint_ab.sh <directory holding the parent commit's bench.py, rigl_amd/ and oracle/> <out.jsonl> [runs]
# The parent's Python runs against the library built from THIS tree (RIGL_HIP_LIB), whose symbols are a superset of its own.
# Stops at the first process that fails.
set -o pipefail
parent=${1:?directory of the parent tree}; out=${2:?output file}; runs=${3:-3}
here=$(cd "$(dirname "$0")/.." && pwd)
lib=$here/rigl_amd/lib/librigl_hip.so
: > "$out"
for run in $(seq 1 "$runs"); do
  for tree in parent this; do
    for wl in resnet50:100 wrn22:300; do
      w=${wl%%:*}; s=${wl##*:}
      if [ $tree = parent ]; then dir=$parent; else dir=$here; fi
      res=$(cd "$dir" && RIGL_HIP_LIB=$lib timeout -k 10 150 python bench.py --gpus 1 --workload "$w" --steps "$s" --warmup 20 --no-cpu-baseline 2>/dev/null | tail -1)
      rc=$?; [ $rc -eq 0 ] || { echo "bench $tree $w: exit status $rc"; exit $rc; }
      echo "{\"tree\": \"$tree\", \"run\": $run, \"workload\": \"$w\", \"result\": $res}" | tee -a "$out" | cut -c1-200
    done
  done
done
