# full GPU suite + the complete (--full) bench line + smoke(), from the repository root; logs under $1 (default validate_out/).
# Stops at the first step that fails.
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-validate_out}
mkdir -p "$OUT"
( time python -m pytest tests -m gpu -x -q ) > "$OUT/gputest.log" 2>&1 &&
( time python bench.py --full ) > "$OUT/bench_full.log" 2>&1 &&
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
rc=$?
tail -n 6 "$OUT/gputest.log"; tail -c 1500 "$OUT/bench_full.log" 2>/dev/null; tail -n 3 "$OUT/smoke.log" 2>/dev/null
exit $rc
