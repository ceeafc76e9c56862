export LLMK_LIB=$PWD/llm.f90_amd/csrc/variants/libllmk_shapes.so
timeout 1500 python -m pytest tests/test_parity_gpu.py -m gpu -x -q -s -k "shapes_added_at_build_time" 2>&1 | grep "build-time\|passed\|failed\|Error" | cut -c1-300
for cfg in "--shape mistral-7b --type q4_0 --cls-q6k" "--shape llama3-8b --type q4_0 --cls-q6k" "--shape mistral-7b --type f16"; do
  LLMK_JOB_TAG=. LLMK_BENCH_LIMIT=900 bash tests/host_tools/gpu_job.sh benchl r06_shapes_bench --full --no-cpu-baseline $cfg
done
unset LLMK_LIB
LLMK_JOB_TAG=. LLMK_BENCH_LIMIT=900 bash tests/host_tools/gpu_job.sh benchl r06_shapes_bench --full --no-cpu-baseline --shape mistral-7b --type q4_0 --cls-q6k
