#!/bin/bash
# On the GPU box: the headline step (config 2) with each library named, alternated REPS times, at margins 0.2 (the
# bench's) and 5.0 (every pair hinge-active).  A name is `product` (graphembeddings_amd/libge_hip.so) or the tag of
# graphembeddings_amd/_variants/libge_<tag>.so (tools/dev/build_variant.py; `parent` = the parent commit's build);
# `<name>:nohandle` runs it without a pipeline handle, preparation on the caller's stream.
# usage: tools/dev/ab_prepare_chunks.sh LOG REPS name...      (LOG: the file the lines go to; it is printed at the end)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$1; REPS=$2; shift 2
mkdir -p "$(dirname "$OUT")"
: > "$OUT"
for rep in $(seq 1 "$REPS"); do
  for margin in 0.2 5.0; do
    for spec in "$@"; do
      t=${spec%%:*}
      if [ "$t" = product ]; then L=""; else L=$ROOT/graphembeddings_amd/_variants/libge_$t.so; fi
      NH=0; [ "$spec" != "$t" ] && NH=1
      echo "== $spec margin $margin (rep $rep)" >> "$OUT"
      GE_LIB=$L GE_MARGIN=$margin GE_NO_HANDLE=$NH timeout -k 10 120 python3 "$ROOT/tools/dev/prepare_chunks_probe.py" 2> "$OUT.err" | grep '^{' >> "$OUT"
      rc=${PIPESTATUS[0]}
      if [ "$rc" != 0 ]; then echo "probe failed ($rc): $spec" >> "$OUT"; tail -5 "$OUT.err" >> "$OUT"; cat "$OUT"; exit 1; fi
    done
  done
done
rm -f "$OUT.err"
cat "$OUT"
