set -x
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${1:?usage: bash tools/run_prof_r2.sh OUT_DIR}
cd $R
python bench.py --full --no-cpu-baseline > $O/r2_bench2.json 2> $O/r2_bench2.log; tail -3 $O/r2_bench2.log; cat $O/r2_bench2.json
rm -rf $O/r2_noov; mkdir -p $O/r2_noov
RE2E_IGEMM_LOG=1 RE2E_NO_OVERLAP=1 rocprofv3 --kernel-trace --stats --output-format csv -d $O/r2_noov -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-roofline > $O/r2_noov/out.json 2> $O/r2_noov/log.txt
tail -2 $O/r2_noov/out.json
python3 tools/igemm_table.py $O/r2_noov/log.txt $O/r2_noov/*/*_kernel_trace.csv > $O/r2_igemm_table.txt 2>&1
head -30 $O/r2_igemm_table.txt; tail -2 $O/r2_igemm_table.txt
cp $O/r2_noov/*/*_kernel_stats.csv $O/r2_noov_kernel_stats.csv
rm -f $O/r2_noov/*/*_kernel_trace.csv $O/r2_noov/*/*.db
