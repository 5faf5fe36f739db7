#!/bin/bash
# tools/debug/serial_vs_overlap.sh <workload> -- masked pass: stand-alone kernel durations (the -DOVRFSR_SERIAL build, ab/serial.so)
# vs the overlapped product library, via rocprofv3 kernel-trace stats
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
W=${1:-C3r}
python3 tools/variant_fresh.py serial -DOVRFSR_SERIAL || tools/build_variant.sh serial -DOVRFSR_SERIAL || exit 1
for S in serial product; do
  L=$PWD/ab/serial.so; [ $S = product ] && L=$PWD/openvr_fsr_amd/libopenvr_fsr_amd.so
  rm -rf /tmp/svo_$S
  OVRFSR_LIB=$L rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/svo_$S -o kt -- python bench.py --no-cpu --no-extras --no-verify --pmc off --workload $W --steps 10 --warmup 2 --pairs 8 > /tmp/svo_$S.log 2>&1
  echo "== $S ($L)"; grep '^{"metric"' /tmp/svo_$S.log | tail -1 | python -c "
import sys, json
s = sys.stdin.read().strip()
if s:
    d = json.loads(s); print('pairs/s', d['value'], 'ms/step', d['ms_per_step'])
else:
    print('(no bench line: see /tmp/svo_$S.log)')"
  find /tmp/svo_$S -name '*kernel_stats.csv' -exec grep ovrfsr {} \; | cut -c1-160
done
