#!/bin/bash
# end-of-session evidence: full bench line, headline kernel trace + PMC traffic, train-step trace + PMC traffic
TAG=${1:-r03b}
# everything lands under $LOGS (the profile scripts write $LOGS/prof_<tag>*)
export LOGS=${LOGS:-bench_logs}
mkdir -p $LOGS
timeout -k 10 420 python -u bench.py --full > $LOGS/${TAG}_bench.log 2>&1 || exit 1
bash tools/run_profiles.sh $TAG > $LOGS/${TAG}_prof.log 2>&1 || exit 1
bash tools/run_train_profiles.sh $TAG 32 > $LOGS/${TAG}_trainprof.log 2>&1 || exit 1
echo FINAL_DONE
