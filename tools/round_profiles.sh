#!/bin/bash
# Everything the committed profiles/ of a round are made from, in ONE GPU-box call:  tools/round_profiles.sh <tag>
#   PMC passes + kernel stats + bench line (pmc_round.sh), engine-op kernel traces (profile_engine_ops.sh), summaries.
# The summaries land in profiles/; they are copied to $OUT/profiles_<tag>/ (OUT: default out/ at the repository root).
TAG=${1:-r06}
cd "$(dirname "$0")/.." || exit 1
export OUT=${OUT:-$PWD/out}; mkdir -p "$OUT"
bash tools/pmc_round.sh $TAG > $OUT/pmc_round_$TAG.log 2>&1
python3 tools/summarize_round.py $TAG > $OUT/summarize_round_$TAG.log 2>&1
bash tools/profile_engine_ops.sh > $OUT/profile_engine_ops_$TAG.log 2>&1
python3 tools/summarize_engine_ops.py $TAG > $OUT/summarize_engine_ops_$TAG.log 2>&1
# the line of record LAST: it folds in the summaries just written (they carry this build's source digest)
python3 bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err; tail -c 300 $OUT/bench_$TAG.json
mkdir -p $OUT/profiles_$TAG
cp profiles/${TAG}_bench_* profiles/${TAG}_engine_ops_* profiles/traffic_${TAG}.json $OUT/profiles_$TAG/ 2>/dev/null
cp $OUT/bench_$TAG.json $OUT/profiles_$TAG/${TAG}_bench_line.json 2>/dev/null
cp $OUT/*_$TAG.log $OUT/profiles_$TAG/ 2>/dev/null
rm -rf $OUT/pmc2_* $OUT/prof_* $OUT/eo_* $OUT/kt_* $OUT/kto   # raw traces are not kept
ls -la $OUT/profiles_$TAG
tail -3 $OUT/summarize_round_$TAG.log
