#!/bin/bash
# Quick GPU check of the product build: bench kernel time (8 and 10 bit)
# with the oracle check of rank 0's frame.
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${QUICK_OUT:-$R/build/quick}
mkdir -p "$O"
for c in ${CONFIGS:-4k 4k-10bit}; do
    timeout -k 10 300 python3 "$R/bench.py" --full --no-cpu --no-families --steps 30 --warmup 3 --config $c > "$O/q_$c.json" 2> "$O/q_$c.err" || exit 1
    echo "$c $(grep -o '"kernel_us": [0-9.]*' "$O/q_$c.json") $(grep -o '"bit_exact_vs_oracle": [a-z]*' "$O/q_$c.json")"
done
