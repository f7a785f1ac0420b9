# Population sweep of the bench line (kernel profile included) and a kernel trace at 4096.
# Lines, logs and the trace go under $OUT (default bench_out/scal).
set -o pipefail
ROOT=$(pwd)
O=${OUT:-bench_out/scal}
mkdir -p $O
for P in 64 256 1024 4096; do
  timeout -k 10 180 python -u bench.py --pop $P --steps 100 --warmup 10 --full --no-cpu-baseline > $O/bench_pop$P.json 2> $O/bench_pop$P.err || exit 1
done
for P in 64 512; do
  timeout -k 10 180 python -u bench.py --pop $P --hidden 32 --steps 100 --warmup 10 --full --no-cpu-baseline > $O/bench_h32_pop$P.json 2> $O/bench_h32_pop$P.err || exit 1
done
cd $O && export TMPDIR=${TMPDIR:-/tmp} && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d prof4096 -o run -- python3 $ROOT/bench.py --pop 4096 --steps 20 --warmup 5 --full --no-cpu-baseline > rp4096.json 2> rp4096.err
