# HBM-side traffic of the conv launches of the bench step (two separate PMC passes, MI355X_MICROARCH.md "HBM").
# SIZE=2048 tools/pmc_traffic.sh : another image size (default 512, the bench workload)
# OUT=dir tools/pmc_traffic.sh : where the two passes go (default: profile_out/pmc_traffic in the repository)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/profile_out/pmc_traffic}
rm -rf "$OUT"; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/f -o f --output-format csv -- python $R/bench.py --size ${SIZE:-512} --steps 3 --warmup 2 --full --no-cpu-baseline --no-extra > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/w -o w --output-format csv -- python $R/bench.py --size ${SIZE:-512} --steps 3 --warmup 2 --full --no-cpu-baseline --no-extra > /dev/null 2>&1
ls $OUT/f $OUT/w
