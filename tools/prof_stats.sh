# usage (GPU box): bash tools/prof_stats.sh <tag> [bench.py args...]  -> $OUT/<tag>_kernel_stats.csv (rocprofv3 --kernel-trace --stats of one bench run)
T=$1; shift
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-prof_out}; mkdir -p $OUT     # where the results go
cp $(ls $OUT/p_$T/*/*kernel_trace.csv | head -1) $OUT/${T}_kernel_trace.csv; rm -rf $OUT/p_$T
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_$T -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-secondary --no-kernel-timing --no-feature-api "$@" > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err
cp $(ls $OUT/p_$T/*/*kernel_stats.csv | head -1) $OUT/${T}_kernel_stats.csv
python -c "import bench; print(bench.source_hash())" > $OUT/${T}_kernel_stats.csv.hash      # bench.py quotes the summary only next to the same kernel sources
cp $(ls $OUT/p_$T/*/*kernel_trace.csv | head -1) $OUT/${T}_kernel_trace.csv; rm -rf $OUT/p_$T
python tools/stats_table.py $OUT/${T}_kernel_stats.csv | head -30
