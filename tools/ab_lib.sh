# Build a library from a git revision into tools/diag/libsgmm_<tag>.so (A/B timing:
# run with SGMM_LIB=<that file>).  The revision is built by its own build.py, so
# its own source list and flags apply.
# Usage: bash tools/ab_lib.sh <rev> <tag> [out.so]
set -e
R=${1:-HEAD}; T=${2:-head}
ROOT=$(git rev-parse --show-toplevel)
O=${3:-$ROOT/tools/diag/libsgmm_$T.so}
P=deep-reinforcement-learning-based-signal-gated-market-making_amd
D=$(mktemp -d); trap 'rm -rf "$D"' EXIT
git -C "$ROOT" archive "$R" $P include | tar -x -C "$D"
mkdir -p "$(dirname "$O")"
python3 "$D/$P/build.py" --out "$(realpath -m "$O")"
