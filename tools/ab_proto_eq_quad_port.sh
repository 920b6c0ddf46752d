#!/bin/sh
# The quad ring's port, attribution and gate: runs the prototype's loop variants -- built
# beforehand, PROTO_VARIANT=<v> python tools/proto_eq_quad_ring.py for each -- alternating, ROUNDS times round, in one
# call, and prints per run the variant, the bit check's verdict, 512 chains' ns per sample and the lone wave's ticks per
# sample.  Every run has its own time limit and the first failure ends the script.
#   sh tools/ab_proto_eq_quad_port.sh [ROUNDS [VARIANT ...]] > table.txt
# Without a list of variants: round 15's (cur C1 C2 C3 nost nold nomem).  Round 17's gate, the library's loop C2 against the
# merged variants: sh tools/ab_proto_eq_quad_port.sh 3 C2 D1 D2 D1W D2W
set -u
here=$(dirname "$0")
rounds=${1:-3}
[ "$#" -gt 0 ] && shift
[ "$#" -gt 0 ] || set -- cur C1 C2 C3 nost nold nomem
r=1
while [ "$r" -le "$rounds" ]; do
    for v in "$@"; do
        bin="$here/bin/proto_eq_quad_ring"
        [ "$v" = cur ] || bin="${bin}_$v"
        out=$(timeout -k 10 120 "$bin") || { echo "round $r $v: FAILED"; echo "$out"; exit 1; }
        bits=$(echo "$out" | grep -c "^chain.*: 0 of .* (0 never written, 0 stray stores)")
        echo "$out" | grep -q "not checked" && bits="-"
        ns=$(echo "$out" | sed -n 's/.* = \([0-9.]*\) ns per sample.*/\1/p')
        tk=$(echo "$out" | sed -n 's/a lone wave: \([0-9.]*\) .*/\1/p')
        echo "round $r  $v  chains_bit_exact $bits  ns_per_sample $ns  lone_wave_ticks_per_sample $tk"
    done
    r=$((r + 1))
done
