#!/usr/bin/env bash
# round 6, final tree: the q4_0 configurations' evidence again (their kernel changed after the r06 evidence run: scale records), the 7B
# decomposition with the structure line, one bench line per other configuration as a cross-check on the same box
cd "$(dirname "$0")/../.." || exit 1
export LLMK_JOB_TAG=r06f
bash tests/host_tools/gpu_job.sh profcfg r06f llama2-7b_q4_0 --shape llama2-7b --type q4_0
bash tests/host_tools/gpu_job.sh profcfg r06f llama2-7b_q4_0_q6k --shape llama2-7b --type q4_0 --cls-q6k
bash tests/host_tools/gpu_job.sh profcfg r06f mistral-7b_q4_0_q6k --shape mistral-7b --type q4_0 --cls-q6k
LLMK_JOB_TAG=prof_r06f LLMK_BENCH_LIMIT=300 bash tests/host_tools/gpu_job.sh bench tinyllama_q4_0_bench --full --no-cpu-baseline --type q4_0
bash tests/host_tools/decomp.sh r06f_decomp7 "--shape llama2-7b --type q4_0" base nohbm debug debug:nosync d_nohbm:nosync
LLMK_JOB_TAG=prof_r06f LLMK_BENCH_LIMIT=300 bash tests/host_tools/gpu_job.sh bench tinyllama_f32_bench --full --no-cpu-baseline
LLMK_JOB_TAG=prof_r06f LLMK_BENCH_LIMIT=300 bash tests/host_tools/gpu_job.sh bench tinyllama_f16_bench --full --no-cpu-baseline --type f16
