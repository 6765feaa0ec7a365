# usage (on the GPU box, from the repo root): bash tools/profile_round.sh <tag>
# kernel-trace stats of the full bench command (python bench.py --full), then PMC passes (own runs) for HBM traffic and SQ counters
R=$PWD; OUT=${T2FIT_PROFILE_OUT:-$PWD/profile_out}; mkdir -p $OUT; TAG=$1; cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -- python3 $R/bench.py --full --cpu-seconds 0 > $OUT/prof_${TAG}.json 2> $OUT/prof_${TAG}.err
cat $OUT/prof_${TAG}.json
cd $R; bash tools/pmc_passes.sh "--solver lbfgsb --no-also" lbfgsb > /dev/null 2>&1; bash tools/pmc_passes.sh "--solver lm --precision f32" lmf32 > /dev/null 2>&1
python tools/pmc_summary.py lbfgsb persistent > $OUT/pmc_${TAG}_lbfgsb.txt; python tools/pmc_summary.py lmf32 persistent > $OUT/pmc_${TAG}_lmf32.txt
python tools/pmc_summary.py lbfgsb residuals > $OUT/pmc_${TAG}_residuals.txt
cat $OUT/pmc_${TAG}_lbfgsb.txt $OUT/pmc_${TAG}_lmf32.txt $OUT/pmc_${TAG}_residuals.txt | grep -E "FETCH|WRITE"
