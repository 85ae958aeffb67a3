#!/bin/bash
# usage: tools/collect_round.sh rNN OUT   -- everything profiles/ holds for a round, from the tree as it is (one MI355X,
# ~25 min), into the folder OUT: the one tools/prof_bench.sh and its siblings write to and tools/copy_round.sh reads
tag=$1
out=${2:?usage: tools/collect_round.sh rNN OUT}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p "$out"
timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -4 > $out/${tag}_gpu_tests.txt
bash tools/bench_all.sh > $out/${tag}_bench_all.txt 2>&1
# (the headline's region alone: --no-secondary keeps the other configs' scan launches out of the scan kernel's average)
bash tools/prof_bench.sh ${tag} --steps 5 --warmup 2 --no-cpu-baseline --no-secondary > $out/${tag}_prof_bench.txt 2>&1
bash tools/pmc_bench.sh fetch FETCH_SIZE --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > $out/${tag}_pmc_fetch.txt 2>&1
bash tools/pmc_bench.sh write WRITE_SIZE --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > $out/${tag}_pmc_write.txt 2>&1
python tools/make_pmc_json.py ${tag} 1000000000 > $out/${tag}_make_pmc.txt 2>&1
cp profiles/${tag}_pmc_1Brows_16cols.json $out/ 2>/dev/null
for c in C2 C4 C5; do
  bash tools/prof_any.sh ${tag}_${c} tools/bench_configs.py --only $c --steps 3 > $out/${tag}_prof_${c}.txt 2>&1
done
bash tools/prof_any.sh ${tag}_ordered tools/bench_distinct.py --rows 1000000000 --steps 3 --ordered-only > $out/${tag}_prof_ordered.txt 2>&1
bash tools/prof_any.sh ${tag}_distinct tools/bench_distinct.py --rows 1000000000 --steps 3 --sparse-rows 1000000000 > $out/${tag}_prof_distinct.txt 2>&1
bash tools/prof_any.sh ${tag}_spearman tools/bench_spearman.py --rows 1000000000 --steps 3 > $out/${tag}_prof_spearman.txt 2>&1
# the pattern kernels (C3): kernel stats, bytes fetched, SQ counters -- one and three patterns, Utf8 and Utf8View
bash tools/prof_any.sh ${tag}_regex tools/bench_regex.py --steps 5 > $out/${tag}_prof_regex.txt 2>&1
bash tools/prof_any.sh ${tag}_regex_view tools/bench_regex.py --steps 5 --view > $out/${tag}_prof_regex_view.txt 2>&1
bash tools/pmc_any.sh ${tag}_rxf FETCH_SIZE tools/bench_regex.py --steps 3 > $out/${tag}_pmc_regex_fetch.txt 2>&1
bash tools/pmc_any.sh ${tag}_rxs "SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_WAVES" tools/bench_regex.py --steps 3 > $out/${tag}_pmc_regex_sq.txt 2>&1
# the list paths (sparse keys, strings): bytes fetched and written per pass
bash tools/pmc_any.sh ${tag}_lf FETCH_SIZE tools/bench_distinct.py --rows 1000000000 --steps 2 --sparse-rows 1000000000 > $out/${tag}_pmc_lists_fetch.txt 2>&1
bash tools/pmc_any.sh ${tag}_lw WRITE_SIZE tools/bench_distinct.py --rows 1000000000 --steps 2 --sparse-rows 1000000000 > $out/${tag}_pmc_lists_write.txt 2>&1
bash tools/pmc_any.sh ${tag}_sf FETCH_SIZE tools/bench_strings.py > $out/${tag}_pmc_strings_fetch.txt 2>&1
bash tools/pmc_any.sh ${tag}_sw WRITE_SIZE tools/bench_strings.py > $out/${tag}_pmc_strings_write.txt 2>&1
# a state per table: create -> update -> finalize -> destroy beside the warm step, and the last cold state's timeline
python tools/cold_step.py > $out/${tag}_cold_step.txt 2>&1
python tools/cold_step.py --rows 1000000 >> $out/${tag}_cold_step.txt 2>&1
bash tools/trace_cold_step.sh > $out/${tag}_cold_step_trace.txt 2>&1
# the experiments of the round whose outcome was "dropped": kept as evidence
python tools/exp_chunked_distinct.py > $out/${tag}_exp_chunked_distinct.txt 2>&1
bash tools/exp_sort_trace.sh 1000000000 TGX_SORT_DEBUG=1 > $out/${tag}_spearman_timeline.txt 2>&1
bash tools/trace_step_api.sh --force-distributed --rows 125000000 --steps 6 --warmup 3 2>&1 | grep -v hipEventQuery > $out/${tag}_shard_step_tail.txt
python tools/sim_bench_ranks.py > $out/${tag}_sim_ranks.txt 2>&1
# the round's whole bench line: the headline, the CPU baseline and the secondary configs
python bench.py --full > $out/${tag}_bench_1gpu.json 2> $out/${tag}_bench_1gpu.err
tail -3 $out/${tag}_gpu_tests.txt; tail -c 600 $out/${tag}_bench_1gpu.json
