# usage (on the MI355X box): bash tools/profile_round.sh r02   -> $OUT/<tag>_* (copy what is to be judged into profiles/)
set -x
T=${1:-r06}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-prof_out}; mkdir -p $OUT     # where the results go (tools/prof_stats.sh writes there too)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_stats -- python bench.py --full --steps 100 --warmup 5 --no-cpu-baseline --no-secondary --no-kernel-timing --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
cp $(ls $OUT/p_stats/*/*kernel_stats.csv | head -1) $OUT/${T}_kernel_stats.csv
HASH=$(python -c "import bench; print(bench.source_hash())")      # bench.py quotes a summary only next to the kernel sources it was taken from
echo $HASH > $OUT/${T}_kernel_stats.csv.hash
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_stats16 -- python bench.py --full --compute-dtype bfloat16 --steps 100 --warmup 5 --no-cpu-baseline --no-secondary --no-kernel-timing --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
cp $(ls $OUT/p_stats16/*/*kernel_stats.csv | head -1) $OUT/${T}_kernel_stats_bf16.csv
echo $HASH > $OUT/${T}_kernel_stats_bf16.csv.hash
# configs[3] / [4]: stats + the kernel sequence of one step (before the bench lines: their roofline.frac quotes these summaries)
for C in 3 4; do bash tools/prof_stats.sh ${T}c$C --steps 100 --config $C --sustain-seconds 0 > /dev/null 2>&1; python tools/step_seq.py $OUT/${T}c${C}_kernel_trace.csv > $OUT/${T}_step_seq_config$C.txt; cp $OUT/${T}c${C}_kernel_stats.csv $OUT/${T}_kernel_stats_config$C.csv; echo $HASH > $OUT/${T}_kernel_stats_config$C.csv.hash; done
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/p_fetch -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/p_write -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
python tools/traffic_from_pmc.py $OUT/p_fetch $OUT/p_write $OUT/${T}_traffic.json | head -8
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/p_fetch16 -- python bench.py --full --compute-dtype bfloat16 --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/p_write16 -- python bench.py --full --compute-dtype bfloat16 --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
python tools/traffic_from_pmc.py $OUT/p_fetch16 $OUT/p_write16 $OUT/${T}_traffic_bf16.json | head -8
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --output-format csv -d $OUT/p_mfma -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-kernel-timing --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
python tools/pmc_summary.py $OUT/p_mfma > $OUT/${T}_pmc_mfma_raw.txt
python tools/mfma_util_from_pmc.py $OUT/${T}_pmc_mfma_raw.txt $OUT/${T}_mfma_util.json | head -8
for C in 3 4; do
  rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/p_fetchc$C -- python bench.py --full --config $C --steps 10 --warmup 3 --no-cpu-baseline --no-kernel-timing --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/p_writec$C -- python bench.py --full --config $C --steps 10 --warmup 3 --no-cpu-baseline --no-kernel-timing --no-feature-api --sustain-seconds 0 > /dev/null 2>&1
  python tools/traffic_from_pmc.py $OUT/p_fetchc$C $OUT/p_writec$C $OUT/${T}_traffic_config$C.json | head -4
  rm -rf $OUT/p_fetchc$C $OUT/p_writec$C
done
python tools/bench_configs.py > $OUT/${T}_configs.jsonl 2>/dev/null
python tools/step_calls.py float32 > $OUT/${T}_step_calls_fp32.txt 2>/dev/null
python tools/step_calls.py bfloat16 > $OUT/${T}_step_calls_bf16.txt 2>/dev/null
python tools/bench_bf16s.py 256 > $OUT/${T}_bf16_storage_gemm.txt 2>/dev/null
python tools/bench_features.py > $OUT/${T}_bench_features.txt 2>/dev/null
bash tools/feat_counters.sh ${T} > /dev/null 2>&1
# the bench lines last: their `roofline.traffic` quotes the PMC summaries of THIS build (matched by source hash), which have to
# sit in profiles/ when bench.py runs (on the box; the copies that are committed come from $OUT/)
: > $OUT/${T}_bench.err
cp $OUT/${T}_traffic.json $OUT/${T}_traffic_bf16.json $OUT/${T}_traffic_config3.json $OUT/${T}_traffic_config4.json profiles/
cp $OUT/${T}_kernel_stats*.csv $OUT/${T}_kernel_stats*.csv.hash profiles/
python bench.py --full > $OUT/${T}_bench.json 2>> $OUT/${T}_bench.err
python bench.py --full --compute-dtype bfloat16 > $OUT/${T}_bench_bf16.json 2>> $OUT/${T}_bench.err
python bench.py --full --config 3 > $OUT/${T}_bench_config3.json 2>> $OUT/${T}_bench.err
python bench.py --full --config 4 > $OUT/${T}_bench_config4.json 2>> $OUT/${T}_bench.err
bash tools/prof_stats.sh ${T}s32 --steps 100 --sustain-seconds 0 > /dev/null 2>&1; python tools/step_seq.py $OUT/${T}s32_kernel_trace.csv > $OUT/${T}_step_seq_fp32.txt
bash tools/prof_stats.sh ${T}s16 --steps 100 --compute-dtype bfloat16 --sustain-seconds 0 > /dev/null 2>&1; python tools/step_seq.py $OUT/${T}s16_kernel_trace.csv > $OUT/${T}_step_seq_bf16.txt
rm -f $OUT/${T}s32_* $OUT/${T}s16_* $OUT/${T}c3_* $OUT/${T}c4_*
rm -rf $OUT/p_stats $OUT/p_stats16 $OUT/p_fetch $OUT/p_write $OUT/p_fetch16 $OUT/p_write16 $OUT/p_mfma
cut -c1-600 $OUT/${T}_bench.json; cut -c1-300 $OUT/${T}_bench_bf16.json
