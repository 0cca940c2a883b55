# summary of tools/gpu_ab.sh logs: VARS="..." KINDS="..." bash tools/gpu_ab_summary.sh <log directory>
D=${1:?the directory tools/gpu_ab.sh wrote its logs to}
for k in ${KINDS:-rand text dna runs}; do for v in A ${VARS:-b}; do printf "%-5s %-6s " $k $v; grep -o "^[0-9.]* ms .*GB/s\|match [0-9.]*\|emit [0-9.]*\|digest [A-Z]*" $D/ab_${v}_$k.log 2>/dev/null | tr '\n' ' '; echo; done; done
