# Round-end evidence: full GPU test suite, the default bench line, rocprofv3 kernel stats of the 512^2 and 2048^2 steps,
# PMC traffic of the conv launches (two separate --pmc passes, no trace domains besides --kernel-trace).
# Everything goes to $OUT (default: profile_out/round in the repository).
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; OUT=${OUT:-$R/profile_out/round}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
(timeout 1200 python -m pytest tests -q -m gpu -n 4 -rA --durations=10 2>&1) > $OUT/pytest.log 2>&1; tail -4 $OUT/pytest.log   # (pytest-xdist: 77 s instead of 282 s on one GPU)
(timeout 600 python bench.py --full) > $OUT/bench.log 2> $OUT/bench.err; tail -1 $OUT/bench.log | cut -c1-400
cd /tmp && export TMPDIR=/tmp
for sz in 512 2048; do
  rm -rf $OUT/prof$sz; mkdir -p $OUT/prof$sz
  timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof$sz -o b --output-format csv -- python $R/bench.py --size $sz --steps 18 --warmup 3 --full --no-extra --no-cpu-baseline > $OUT/prof$sz/log.txt 2>&1
done
cd "$R"; ls $OUT/prof512 | head -3
PMC=$OUT/pmc_traffic
OUT=$PMC bash tools/pmc_traffic.sh > $OUT/pmc.log 2>&1; python tools/pmc_traffic_summary.py $PMC $OUT/pmc_traffic_conv.json 2>> $OUT/pmc.log | cut -c1-400
python tools/pmc_per_launch.py $PMC > $OUT/pmc_per_launch_512.txt 2>> $OUT/pmc.log
SIZE=2048 OUT=$PMC bash tools/pmc_traffic.sh >> $OUT/pmc.log 2>&1; SIZE=2048 python tools/pmc_traffic_summary.py $PMC $OUT/pmc_traffic_conv_2048.json 2>> $OUT/pmc.log | cut -c1-400
python tools/pmc_per_launch.py $PMC > $OUT/pmc_per_launch_2048.txt 2>> $OUT/pmc.log
for cfg in "2048 2" "2048 4" "2048 8" "2896x2172 8"; do timeout 500 python tools/strip_bench.py $cfg 2>&1 | grep strip_bench; done > $OUT/strip_bench.txt
ST_AMD_TIMELINE=1 python bench.py --full --steps 30 --warmup 10 --no-extra --no-cpu-baseline 2>&1 | grep timeline | tail -3 > $OUT/timeline512.txt
(ST_FABRIC_SELF_HALO=1 ST_FABRIC_FORCE_COLLECTIVES=1 timeout 200 python tools/fabric_host_time.py 272 2896; ST_FABRIC_SELF_HALO=1 ST_FABRIC_FORCE_COLLECTIVES=1 timeout 200 python tools/fabric_host_time.py 256 2048) 2>&1 | grep "^\[fabric\]" > $OUT/fabric_host_time.txt
timeout 120 python tools/stylize_breakdown.py 2>&1 | grep breakdown > $OUT/stylize_breakdown.txt
