# Round-4 evidence, run on a GPU box from the repo root; outputs under evidence/r04 and evidence/prof_r04,
# summarised into profiles/r04_* by tools/summarize_profiles.py r04 (committed copies).
set -x
R=$(pwd)
mkdir -p evidence/r04
python bench.py --full > evidence/r04/bench_default.json 2> evidence/r04/bench_default.err
tail -c 400 evidence/r04/bench_default.json
python bench.py --unfused-tail --no-cpu-baseline --no-roofline 2>/dev/null | tail -1 > evidence/r04/bench_unfused_tail.json
python tools/step_breakdown.py --detail > evidence/r04/step_breakdown.txt 2>&1
bash tools/collect_profiles.sh r04 > evidence/r04/collect.log 2>&1
python tools/trace_gaps.py $(find evidence/prof_r04/trace -name step_kernel_trace.csv | head -1) > evidence/r04/step_timeline.txt 2>&1
python tools/head_tail_bench.py > evidence/r04/head_tail_bench.txt 2>&1
python bench.py --workload albef --full > evidence/r04/bench_albef.json 2> evidence/r04/bench_albef.err
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $R/evidence/prof_r04/albef_trace -o step --output-format csv -- python $R/bench.py --workload albef --steps 5 --warmup 2 --no-cpu-baseline --no-roofline > $R/evidence/r04/albef_trace.log 2>&1)
for set in "FETCH_SIZE" "WRITE_SIZE"; do
  name=$(echo "$set" | awk '{print tolower($1)}')
  (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --pmc $set --kernel-trace -d $R/evidence/prof_r04/albef_pmc_$name -o p --output-format csv -- python $R/bench.py --workload albef --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-graph > $R/evidence/r04/albef_pmc_$name.log 2>&1)
done
for f in "" "--fp8"; do python bench.py --batch 64 $f --no-cpu-baseline --no-roofline --steps 100 --warmup 10 2>/dev/null | tail -1; done > evidence/r04/bench_b64.json
ls -la evidence/r04 evidence/prof_r04 | head -40
