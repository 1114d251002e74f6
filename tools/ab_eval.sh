cd "$(dirname "$(readlink -f "$0")")/.." && OUT=${OUT:-bench_out} && mkdir -p $OUT || exit 1
for g in 320 256 224 192 160 128; do
COZK_EVAL_GX=$g timeout -k 10 200 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > $OUT/ab.json 2> $OUT/ab.err || exit 1
python -c "
import json
d=json.load(open('$OUT/ab.json')); k=d['roofline']['kernels']; print('gx $g', k['k_poly_eval_chi']['achieved'], k['k_poly_eval_chi']['avg_launch_ms'], d['phases_ms_per_step']['evaluate'], d['ms_per_step'])"
done
