# same-box A/B of environment switches: bash tools/ab_env.sh "VAR=1" "VAR2=x VAR3=y" ...  ("" = defaults)
cd "$(dirname "$(readlink -f "$0")")/.." && OUT=${OUT:-bench_out} && mkdir -p $OUT || exit 1
for rep in 1 2; do
for cfg in "$@"; do
  env $cfg timeout -k 10 200 python bench.py --full --steps 6 --warmup 1 --no-cpu-baseline > $OUT/ab.json 2> $OUT/ab.err || exit 1
  python -c "
import json
d=json.load(open('$OUT/ab.json')); k=d['roofline']['kernels']['k_msm_scatter_lds']
print('[$cfg]: step', d['ms_per_step'], 'commit', d['phases_ms_per_step']['commit'], 'scatter avg', k['avg_launch_ms'], 'gather avg', d['roofline']['avg_launch_ms'])
"
done
done
