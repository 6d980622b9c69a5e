# usage (GPU box): bash tools/prof_traffic.sh <tag> [bench.py args...] -> $OUT/<tag>_traffic.json (separate FETCH_SIZE / WRITE_SIZE passes)
T=$1; shift
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-prof_out}; mkdir -p $OUT     # where the results go
rm -rf $OUT/pf_$T $OUT/pw_$T
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pf_$T -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-kernel-timing "$@" > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pw_$T -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-secondary --no-kernel-timing "$@" > /dev/null 2>&1
python tools/traffic_from_pmc.py $OUT/pf_$T $OUT/pw_$T $OUT/${T}_traffic.json | head -16
rm -rf $OUT/pf_$T $OUT/pw_$T
