# the default bench line alone (after a change of bench.py that does not touch the timed path)
export GPU_MAX_HW_QUEUES=8
cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/r6_bench_only.sh OUT_DIR}
mkdir -p $O
python bench.py --full > $O/bench_default.json 2> $O/bench_default.log; echo "bench rc=$?"; tail -2 $O/bench_default.log
