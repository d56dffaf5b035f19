# one GPU call of the round: the GPU test suite, the bench with every leg
# (--full), then PMC passes of the named workloads, then the headline alone (one
# stream, every other leg switched off) under rocprofv3 --kernel-trace --stats,
# whose average the line's single_stream kernel_ms must match.  A failing test
# does not stop the call; a crash, abort or time limit does.
# Usage: [OUT=dir] bash scripts/gpu_round.sh PREFIX [pmc workloads...]
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
OUT=${OUT:-$ROOT/run_out}
mkdir -p "$OUT"
P=${1:-r4c}; shift
fatal() { case $1 in 124|134|137|139) echo "fatal rc=$1 in $2"; exit $1;; esac; }
timeout -k 10 500 python -u -m pytest tests -m gpu -v -rs --timeout 150 --timeout-method thread > "$OUT/${P}_gpu_tests.txt" 2>&1
rc=$?; echo "tests rc=$rc"; fatal $rc tests
timeout -k 10 600 python bench.py --full > "$OUT/${P}_bench.jsonl" 2> "$OUT/${P}_bench.err" || exit 2
[ $# -gt 0 ] && { bash scripts/gpu_pmc.sh $P "$@" || exit 3; }
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/${P}_prof" -o run --output-format csv -- python3 "$ROOT/bench.py" --full --steps 20 --warmup 5 --configs "" --no-cpu-baseline --latency-qps 0 --host-rows 0 --host-rows-configs 0 --nan-variant 0 --no-tree-shard --streams 1 --c5-http-qps "" --c5-http-v2-qps "" > "$OUT/${P}_bench_prof.jsonl" 2>&1 || exit 5
