#!/bin/bash
# Evidence for the fused split-fp32 ResBlock2 pair kernels
# (resblock_f32p_kernel<32|64|128>) in one infer_p2 step of the headline
# shape (tools/infer_breakdown.py), three separate runs (GPU box):
#   trace: rocprofv3 --kernel-trace --stats
#   p1:    counters - clock, MFMA busy, issue mix, SQ_WAIT_ANY
#   p2:    counters - SQ_WAIT_INST_ANY, LDS bank conflicts, vector memory
# usage: tools/pmc_pairs.sh OUTDIR        (run from the tree to profile)
# Report: python tools/pmc_pairs_report.py OUTDIR
export TMPDIR=/tmp
OUT=${1:-bench_logs/pmc_pairs}
mkdir -p $OUT
export STEPS=1
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o run -- python3 tools/infer_breakdown.py > $OUT/trace.log 2>&1 || exit 1
timeout -k 10 240 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY --output-format csv -d $OUT/p1 -o run -- python3 tools/infer_breakdown.py > $OUT/p1.log 2>&1 || exit 1
timeout -k 10 240 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS --output-format csv -d $OUT/p2 -o run -- python3 tools/infer_breakdown.py > $OUT/p2.log 2>&1 || exit 1
echo PMC_PAIRS_DONE
