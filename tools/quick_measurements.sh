#!/bin/bash
# full -m gpu suite, smoke, the default bench line, the same under rocprofv3 --kernel-trace --stats, layer A/B tools: one box
root=$PWD; out=$root/measurements; mkdir -p $out; R=r06
python -m pytest tests -m gpu -q 2>&1 | tail -5 > $out/${R}_suite.txt; cat $out/${R}_suite.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 1200 python bench.py --full > $out/${R}_bench_line.json 2> $out/${R}_bench_line.err; echo "bench rc=$?"
python tools/show_bench.py $out/${R}_bench_line.json 2>/dev/null | head -24
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${R}_kstats -- python $root/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/${R}_bench_line_under_rocprof.json 2> $out/${R}_under_rocprof.err
cd $root
f=$(find $out/${R}_kstats -name "*kernel_stats.csv" | head -1); cp "$f" $out/${R}_kernel_stats_bench_1080p.csv; head -6 $out/${R}_kernel_stats_bench_1080p.csv | cut -c1-150
rm -rf $out/${R}_kstats
BATCH=16 python tools/bench_poly.py > $out/${R}_ab_polyphase.txt 2>/dev/null; BATCH=64 python tools/bench_poly.py >> $out/${R}_ab_polyphase.txt 2>/dev/null; cat $out/${R}_ab_polyphase.txt
