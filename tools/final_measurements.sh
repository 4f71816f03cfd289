root=${GRAFT_REPO_ROOT:-$PWD}
cd $root; out=$root/measurements; mkdir -p $out; R=r06
timeout 1200 python bench.py --full > $out/${R}_bench_line.json 2> $out/${R}_bench_line.err
echo "bench rc=$?"
python tools/show_bench.py $out/${R}_bench_line.json 2>/dev/null | head -30
python -c "
import json; d=json.load(open('$out/${R}_bench_line.json')); print('contract_v2', {k: d['contract_v2'][k] for k in ('value','ms_per_step','vs_headline','closed_loop_ok')}, d['contract_v2']['winograd_kernel']); print('pipelined', d['pipelined']['value'], 'hr pipelined', d['high_rate']['pipelined']['value'])"
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${R}_kstats -- python $root/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/${R}_bench_line_under_rocprof.json 2> $out/${R}_under_rocprof.err
cd $root
f=$(find $out/${R}_kstats -name "*kernel_stats.csv" | head -1); cp "$f" $out/${R}_kernel_stats_bench_1080p.csv; head -8 $out/${R}_kernel_stats_bench_1080p.csv | cut -c1-150
rm -rf $out/${R}_kstats
python -c "
import json; d=json.load(open('$out/${R}_bench_line_under_rocprof.json')); print('under rocprof', d['value'], d['roofline']['achieved'], d['roofline']['avg_launch_us'], d['roofline']['launches'])"
