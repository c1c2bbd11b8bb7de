#!/bin/bash
# A/B of the at-scale attention forms on one box: wave-per-tile launches (default, csrc/attn_wave.hip) against the length-class lists (DR4SR_ATTN_LISTS=1)
mkdir -p gpurun_out
(timeout 1200 python -m pytest tests/test_gpu_attn_wave.py -x -q -m gpu; echo rc=$?) > gpurun_out/attn_wave_tests.txt 2>&1
tail -5 gpurun_out/attn_wave_tests.txt
run() { echo -n "$1 B=$2 $3: "; env $1 timeout 300 python bench.py --full --no-cpu-baseline --no-strong --no-throughput-mode --no-deterministic-leg --batch $2 --steps 100 --repeats 5 $3 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); k=d['kernel_us_per_step']; print(round(d['ms_per_step'],4), round(d['value']), {x: k.get(x) for x in ('embqkv_fwd','attn_fwd','post_fwd','post_mid','attn_bwd','post_bwd','qkv_embed_bwd','wgrad_fused','adam')}, 'loss', round(d['final_loss'],5))"; }
for B in ${AB_SIZES:-8192 4096 32768}; do
  run X=1 $B; run DR4SR_ATTN_LISTS=1 $B
done 2>&1 | tee gpurun_out/attn_wave_ab.txt
if [ -n "$AB_D128" ]; then run X=1 8192 "--embed-dim 128"; run DR4SR_ATTN_LISTS=1 8192 "--embed-dim 128"; fi 2>&1 | tee -a gpurun_out/attn_wave_ab.txt
