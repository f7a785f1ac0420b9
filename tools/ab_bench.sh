# Alternating A/B bench of two libraries on one box.  Usage: bash tools/ab_bench.sh <libA> <libB> [rounds]
# (lines and logs under $OUT, default bench_out/ab)
set -o pipefail
A=$1; B=$2; N=${3:-3}
O=${OUT:-bench_out/ab}
mkdir -p $O
for i in $(seq 1 $N); do
  for L in $A $B; do
    SGMM_LIB=$L timeout -k 10 120 python -u bench.py --steps 400 --warmup 20 --full --no-cpu-baseline > $O/b.json 2> $O/b.err || { echo BENCH_FAIL $L; tail $O/b.err; exit 1; }
    python -c "import json,sys; d=json.load(open(sys.argv[2])); print(sys.argv[1], '%.4g'%d['value'], '%.2f us/gen'%(d['ms_per_step']*1e3), {k:round(v['avg_us'],2) for k,v in d['kernels'].items()})" $L $O/b.json
  done
done
