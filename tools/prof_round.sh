#!/bin/bash
# rocprofv3 passes whose summaries are committed under profiles/ (run on the GPU box through gpurun): kernel trace + stats, and the
# FETCH_SIZE / WRITE_SIZE / VALUBusy counters in separate passes, for the headline batch (cfg 2) and for cfg 3 at S = 1024.
set -e
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
cd $R
O=${PROF_OUT:-prof_out/r2prof}
rm -rf $O && mkdir -p $O
# cfg 2 (headline): kernel trace + the two PMC passes
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats2 -o cfg2 -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-configs --sustain-seconds 0 > $O/bench_cfg2_stats.json 2> $O/bench_cfg2_stats.err
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch2 -o cfg2 -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-configs --sustain-seconds 0 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write2 -o cfg2 -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-configs --sustain-seconds 0 > /dev/null 2>&1
# cfg 3, S = 1024
rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats3 -o cfg3 -- python3 bench.py --full --config 3 --no-s1 --steps 10 --warmup 2 --no-cpu-baseline > $O/bench_cfg3_stats.json 2> $O/bench_cfg3_stats.err
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch3 -o cfg3 -- python3 bench.py --full --config 3 --no-s1 --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write3 -o cfg3 -- python3 bench.py --full --config 3 --no-s1 --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --pmc VALUBusy --output-format csv -d $O/valu3 -o cfg3 -- python3 bench.py --full --config 3 --no-s1 --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2>&1 || true
rocprofv3 --pmc VALUBusy --output-format csv -d $O/valu2 -o cfg2 -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-configs --sustain-seconds 0 > /dev/null 2>&1 || true
find $O -type f | xargs ls -la | head -60
# keep only the small CSVs (traces can be large)
find $O -name "*kernel_trace.csv" -size +20M -delete
du -sh $O
# summaries (small) next to the raw CSVs; the raw traces are dropped when large
python3 tools/summarize_profiles.py --tag round2 --stats $O/stats2 --fetch $O/fetch2 --write $O/write2 --outdir $O/summ --cmd "python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-configs --sustain-seconds 0" || true
python3 tools/summarize_profiles.py --tag round2_cfg3 --stats $O/stats3 --fetch $O/fetch3 --write $O/write3 --outdir $O/summ --cmd "python3 bench.py --full --config 3 --no-s1 --steps 3 --warmup 1 --no-cpu-baseline" || true
python3 tools/summarize_profiles.py --tag round2 --valu $O/valu2 --outdir $O/summ || true
python3 tools/summarize_profiles.py --tag round2_cfg3 --valu $O/valu3 --outdir $O/summ || true
find $O -type f -size +2M -delete
du -sh $O
