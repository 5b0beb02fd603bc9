#!/bin/bash
# Compute-side PMC passes of the weighted against the unweighted MFMA Gram: the two --pmc
# passes of tools/pmc_compute.sh (never combined with trace domains, each its own run) around
# tools/bench_bootstrap.py, which launches both instantiations on the same rows in one process.
# usage (from the repository root): tools/pmc_bootstrap.sh <outdir> [config=c3]
#   writes <outdir>/p1, <outdir>/p2 (the counter CSVs), <outdir>/json1, json2 and <outdir>/p1.log, p2.log;
#   with <outdir> the directory tools/pmc_compute_summary.py reads for a tag, the summary is
#   python tools/pmc_compute_summary.py <tag> bootstrap_<config> "gram_mfma_kernel<double, false>;gram_mfma_kernel<double, true>"
set -o pipefail
out="$1"
cfg="${2:-c3}"
[ -n "$out" ] || { echo "usage: tools/pmc_bootstrap.sh <outdir> [config]" >&2; exit 2; }
root="$(pwd)"
mkdir -p "$out" || exit $?
out="$(cd "$out" && pwd)"
P1="GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_INSTS_VALU_MFMA_F64 SQ_INSTS_VALU"
P2="GRBM_GUI_ACTIVE SQ_INSTS_VALU_FLOPS_FP64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_VALU_MFMA_COEXEC_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_LDS"
i=0
for pass in "$P1" "$P2"; do
  i=$((i + 1))
  timeout -s KILL 240 rocprofv3 --pmc $pass --output-format csv -d "$out/p$i" -o run \
    -- python3 "$root/tools/bench_bootstrap.py" "$cfg" --reps 2 --outdir "$out/json$i" \
    > "$out/p$i.log" 2>&1 || exit $?
done
