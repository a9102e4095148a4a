R=$(cd "$(dirname "$0")/../.." && pwd)
for t in . .wt_old . .wt_old; do cd "$R/$t"; python bench.py --full --no-cpu-baseline --repeats 5 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$t', d['value'], d['ms_per_step'], d['roofline']['kernels_ms'])"; done
