# A/B bench of two libraries at one population size.  Usage: bash tools/ab_pop.sh <libA> <libB> <pop> [rounds]
# (lines and logs under $OUT, default bench_out/ab)
set -o pipefail
A=$1; B=$2; P=$3; N=${4:-2}
O=${OUT:-bench_out/ab}
mkdir -p $O
for i in $(seq 1 $N); do
  for L in $A $B; do
    SGMM_LIB=$L timeout -k 10 150 python -u bench.py --pop $P --steps 50 --warmup 5 --full --no-cpu-baseline > $O/b.json 2> $O/b.err || { echo BENCH_FAIL $L; tail $O/b.err; exit 1; }
    python -c "import json,sys; d=json.load(open(sys.argv[3])); print(sys.argv[1], sys.argv[2], '%.4g'%d['value'], '%.2f us/gen'%(d['ms_per_step']*1e3), {k:round(v['avg_us'],2) for k,v in d['kernels'].items()})" $L $P $O/b.json
  done
done
