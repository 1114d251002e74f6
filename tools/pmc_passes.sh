cd "$(dirname "$(readlink -f "$0")")/.." && OUT=${OUT:-bench_out} && mkdir -p $OUT && export TMPDIR=/tmp &&
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-full-step > $OUT/pmc_fetch.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-full-step > $OUT/pmc_write.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_THREAD_CYCLES_VALU --kernel-trace --output-format csv -d $OUT/pmc_sq -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-full-step > $OUT/pmc_sq.log 2>&1 &&
timeout -k 10 200 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_INST_CYCLES_VMEM SQ_WAIT_INST_ANY --kernel-trace --output-format csv -d $OUT/pmc_sq2 -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-full-step > $OUT/pmc_sq2.log 2>&1
python tools/pmc_summary.py $OUT/pmc_hbm.json $OUT/pmc_fetch $OUT/pmc_write > $OUT/pmc_hbm.txt 2>&1
python tools/pmc_summary.py $OUT/pmc_sq.json $OUT/pmc_sq $OUT/pmc_sq2 > $OUT/pmc_sq.txt 2>&1
find $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_sq $OUT/pmc_sq2 -name "*.csv" -size +2000k -delete
tail -3 $OUT/pmc_sq.log; tail -3 $OUT/pmc_sq2.log
