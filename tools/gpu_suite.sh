# Full GPU verification: the C++ adapter check against the reference, then every -m gpu test.
#   bash tools/gpu_suite.sh [OUT]      records go under OUT (default: suite_out/)
set -o pipefail
OUT=${1:-suite_out}
mkdir -p "$OUT"
timeout -k 10 300 oracle/_ref/cpp/adapter_check > "$OUT/adapter_m.jsonl" 2> "$OUT/adapter_m.err"; rc=$?; echo adapter rc=$rc
case $rc in 124|134|137|139) exit $rc;; esac    # a hang, abort or fault: start nothing more on the GPU
grep -c '"ok": false' "$OUT/adapter_m.jsonl"
timeout -k 10 1000 python -u -m pytest -q --timeout 300 --timeout-method thread tests -m gpu > "$OUT/pytest_m.log" 2>&1; echo pytest rc=$?; tail -8 "$OUT/pytest_m.log"
