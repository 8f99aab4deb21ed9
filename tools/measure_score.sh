#!/bin/bash
# GCI_score.py at CHM13 size on one MI355X ("GCI_score.py"): inputs, two timed end-to-end runs, a kernel-trace run and
# a PMC run of their own, and the summary.  usage: bash tools/measure_score.sh OUTDIR [SCALE]; the inputs go to $TMPDIR.
# Every step has a time limit of its own; the first failure ends the script.
set -u
cd "$(dirname "$0")/.."
out=$1
scale=${2:-1.0}
d=${TMPDIR:-/tmp}/gci_score_measure
mkdir -p "$out"
three="--hifi $d/hifi.depth.gz --nano $d/nano.depth.gz --two-type $d/two.depth.gz"
timeout -k 10 1200 python tools/measure_score.py make "$d" "$scale" > "$out/make.log" 2>&1 || { echo "make failed: $?"; tail -20 "$out/make.log"; exit 1; }
cp "$d/inputs.json" "$out/"
timeout -k 10 900 python tools/measure_score.py run "$d" "$out" > "$out/run.log" 2>&1 || { echo "run failed: $?"; tail -20 "$out/run.log"; exit 1; }
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/trace" -o score -- \
    python GCI_score.py -r "$d/ref.fa" $three -d "$d/out_trace" -o T -f > "$out/trace.log" 2>&1 || { echo "trace failed: $?"; tail -20 "$out/trace.log"; exit 1; }
# one counter per run: FETCH_SIZE and WRITE_SIZE together exceed what the hardware collects in one pass
for c in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d "$out/pmc/$c" -o score -- \
        python GCI_score.py -r "$d/ref.fa" --hifi "$d/hifi.depth.gz" -d "$d/out_pmc" -o P -f > "$out/pmc_$c.log" 2>&1 || { echo "pmc $c failed: $?"; tail -20 "$out/pmc_$c.log"; exit 1; }
done
timeout -k 10 120 python tools/measure_score.py summarize "$d" "$out"
