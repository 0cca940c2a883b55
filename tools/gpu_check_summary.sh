# summary of tools/gpu_check.sh logs: bash tools/gpu_check_summary.sh <log directory>
D=${1:?the directory tools/gpu_check.sh wrote its logs to}
tail -1 $D/gs_parity.log
for f in rand c2 text c3 runs zeros dna; do printf "%-6s " $f; grep -o "^[0-9.]* ms .*GB/s\|digest [A-Z]*\|match [0-9.]*\|stitch [0-9.]*\|emit [0-9.]*\|tree [0-9.]*\|encode [0-9.]*" $D/gs_$f.log | tr '\n' ' '; echo; done
