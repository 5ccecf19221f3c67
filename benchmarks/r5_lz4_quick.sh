#!/bin/bash
# Round 5: the LZ4 decoder's quick loop -- parity of the LZ4 GPU tests, the headline time (no side legs), the phase timers.
# bash benchmarks/r5_lz4_quick.sh [tag]
T=${1:-quick}
mkdir -p gpurun_out
timeout 600 python -m pytest tests/test_gpu_lz4.py -x -q 2>&1 | tail -3 > gpurun_out/r5_${T}_tests.log
for i in 1 2; do
timeout 300 python bench.py --full --no-cpu --no-e2e --no-others --steps 40 --warmup 20 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); print('ms', d['ms_per_step'], 'kernel', d['roofline'].get('kernel_ms_avg'), 'dists', {k: v.get('ms_per_step') for k, v in d.get('per_distribution', {}).items()} if isinstance(d.get('per_distribution'), dict) else d.get('per_distribution'))
" >> gpurun_out/r5_${T}_times.log
done
RCX_AB=1 timeout 300 python benchmarks/lz4_v8_profile.py text 4096 > gpurun_out/r5_${T}_prof.txt 2>&1
RCX_AB=1 timeout 300 python benchmarks/lz4_v8_profile.py text 256 >> gpurun_out/r5_${T}_prof.txt 2>&1
cat gpurun_out/r5_${T}_tests.log gpurun_out/r5_${T}_times.log gpurun_out/r5_${T}_prof.txt | grep -v amdgpu.ids
