# Round evidence: bench line, rocprofv3 kernel-trace summary and PMC traffic.
# Usage (on the GPU box): bash tools/profile_round.sh r01   (output under $OUT/r01, default bench_out/r01)
set -o pipefail
R=${1:-r01}
O=${OUT:-bench_out}/$R
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $O
B="python bench.py --steps 100 --warmup 5 --full --no-cpu-baseline --profile-steps 10"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -o bench -- $B > $O/kt_bench.json 2> $O/kt.err || { echo "kernel-trace failed"; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch -o p -- $B > /dev/null 2> $O/fetch.err || { echo "pmc fetch failed"; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write -o p -- $B > /dev/null 2> $O/write.err || { echo "pmc write failed"; exit 1; }
python tools/pmc_traffic.py $O/fetch $O/write $O/pmc_traffic.json > /dev/null
cp $O/pmc_traffic.json profiles/${R}_pmc_traffic.json
timeout -k 10 300 python bench.py --full > $O/bench.json 2> $O/bench.err || { echo "bench failed"; exit 1; }
echo profile done
