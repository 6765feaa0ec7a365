OUT=${T2FIT_PROFILE_OUT:-$PWD/profile_out}; mkdir -p $OUT
cd $GRAFT_REPO_ROOT
python -m pytest tests -x -q -m gpu > $OUT/final4_gpu_suite.log 2>&1 && python -c "import __graft_entry__ as g; g.smoke()" > $OUT/final4_smoke.log 2>&1 && python bench.py --full > $OUT/final4_bench.json 2> $OUT/final4_bench.err
tail -2 $OUT/final4_gpu_suite.log; tail -1 $OUT/final4_smoke.log
