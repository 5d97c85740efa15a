# round-end checks: the whole -m gpu suite, smoke(), the default --full bench;
# logs and the bench line go to $OUT (default out/)
set -o pipefail
T=${T:-full}
OUT=${OUT:-out}; mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/gputest_$T.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $OUT/gputest_$T.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$T.log 2>&1 || exit 1
[ -n "$NO_BENCH" ] && exit 0
timeout -k 10 600 python -u bench.py --full > $OUT/bench_$T.json 2> $OUT/bench_$T.err || exit 1
