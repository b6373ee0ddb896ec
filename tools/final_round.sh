#!/bin/bash
# End-of-round measurement set (GPU box), every step under its own time limit and chained:
#   the whole -m gpu suite (no -x: every failure is listed), smoke(), the bench with every
#   leg (`python bench.py --full --steps 20 --warmup 5`), then rocprofv3 --kernel-trace --stats
#   of that very command (its dQ + dK/dV averages reproduce roofline.frac), then the PMC passes
#   of the attention kernels (HBM traffic per launch, D = 64 and D = 256).
#   bash tools/final_round.sh [tag] [skip-pmc]
#   PHASE=a: the suite, smoke() and the bench only; PHASE=b: the profiled bench and the PMC
#   passes only (two gpurun calls under the 20-minute limit); default both.
#   Every log and result goes to $OUT (default out/) as <tag>_<what>, the suite's measured
#   parity errors to <tag>_parity_metrics.jsonl.
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-out}
mkdir -p "$OUT"
T=${1:-r05}
P="$OUT/$T"
PHASE=${PHASE:-ab}
if [[ $PHASE == *a* ]]; then
VDIFF_TEST_METRICS="${P}_parity_metrics.jsonl" timeout -k 10 1100 python3 -u -m pytest tests \
  -m gpu -q --timeout 300 --timeout-method thread -p no:cacheprovider > "${P}_gpu_tests.log" 2>&1
rc=$?
grep -E "passed|failed" "${P}_gpu_tests.log" | tail -2; grep FAILED "${P}_gpu_tests.log" | head
case $rc in 0|1) ;; *) echo "pytest rc=$rc: stopping"; exit $rc;; esac
timeout -k 10 600 python3 -c "import __graft_entry__ as g; g.smoke()" > "${P}_smoke.log" 2>&1 \
  || { tail -20 "${P}_smoke.log"; exit 1; }
tail -1 "${P}_smoke.log"
timeout -k 10 900 python3 -u bench.py --full --steps 20 --warmup 5 > "${P}_bench.json" \
  2> "${P}_bench.err" || { echo "bench rc=$?"; tail -20 "${P}_bench.err"; exit 1; }
tail -c 300 "${P}_bench.json"; echo
fi
[[ $PHASE == *b* ]] || exit 0
rm -rf /tmp/prof_${T}
timeout -k 10 1000 rocprofv3 --kernel-trace --stats -d /tmp/prof_${T} -o run -- \
  python3 -u bench.py --full --steps 20 --warmup 5 > "${P}_bench_profiled.json" \
  2> "${P}_bench_profiled.err" \
  || { echo "rocprof rc=$?"; tail -20 "${P}_bench_profiled.err"; exit 1; }
db=$(find /tmp/prof_${T} -name '*.db' | head -n 1)
python3 tools/prof_summary.py "$db" > "${P}_kernel_stats.md"
head -12 "${P}_kernel_stats.md"
if [ -z "$2" ]; then
  PMC_OUT="${P}_pmc64" timeout -k 10 600 bash tools/pmc_attn.sh --only 64 > "${P}_pmc64.log" 2>&1 \
    || { echo "pmc64 rc=$?"; tail -5 "${P}_pmc64.log"; exit 1; }
  PMC_OUT="${P}_pmc256" timeout -k 10 600 bash tools/pmc_attn.sh --only 256 \
    > "${P}_pmc256.log" 2>&1 || { echo "pmc256 rc=$?"; tail -5 "${P}_pmc256.log"; exit 1; }
  echo pmc done
fi
