#!/bin/bash
# Runs on the GPU box: profile of the full bench command (every line of `bench.py --full`) -> prof_bench/summary.txt (tools/prof_cmd.sh)
exec bash tools/prof_cmd.sh bench python $PWD/bench.py --full --cpu-seconds 0 $BENCH_ARGS
