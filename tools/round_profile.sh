#!/bin/bash
# Everything the round's numbers come from, in one call on the GPU box: the bench line with --full, the rocprofv3 kernel stats
# of a plain bench run, the PMC passes (tools/prof_pmc.sh) and the inflate kernels' PMC passes.
# Usage: OUT_DIR=<directory for the outputs> bash tools/round_profile.sh <tag>
tag=${1:-rXX}
out=$(realpath -m "${OUT_DIR:?set OUT_DIR to the directory for the outputs}")
export TMPDIR=/tmp OUT_DIR=$out
mkdir -p "$out"
timeout 1500 python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"; echo "bench rc=$?"
(cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/${tag}_stats" -o bench -- python "$OLDPWD/bench.py" --steps 20 --warmup 3 > "$out/${tag}_bench_rocprof.json" 2> "$out/${tag}_bench_rocprof.err"); echo "stats rc=$?"
timeout 1800 bash tools/prof_pmc.sh $tag
python tools/pmc_summary.py "$out/pmc_${tag}" > "$out/${tag}_pmc_summary.txt" 2>&1
timeout 900 bash tools/prof_pmc_inflate.sh > "$out/${tag}_inflate_pmc.txt" 2>&1
tail -c 600 "$out/${tag}_bench.json"
