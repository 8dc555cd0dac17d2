#!/bin/bash
# Round-6 measurement set: the full bench line (bench.py --full: every leg
# beside the headline), the kernel trace + FETCH_SIZE pass
# (tools/profile_round.sh), the SQ/LDS counter mix of the product kernel
# (tools/pmc_detail.sh) and the ablation ladder (tools/ablate.py).
#   bash tools/r6_round_profile.sh <tag>
set -euo pipefail
TAG=$1
# everything goes under the output root that the two scripts called below use
ROOT=$(sed -n 's|^OUT=\([^/]*\)/.*|\1|p' tools/profile_round.sh)
OUT=$ROOT/$TAG
mkdir -p $OUT
timeout -k 10 400 python3 bench.py --full > $OUT/bench.json 2> $OUT/bench.err
bash tools/profile_round.sh $TAG
bash tools/pmc_detail.sh $TAG 0 C
python3 tools/pmc_modes.py $ROOT/pmc_$TAG --out $OUT/pmc_detail.json
timeout -k 10 300 python3 tools/ablate.py --rules C --modes 0,3,2,7 --rounds 5 --reps 5 > $OUT/ablation.json 2> $OUT/ablation.err
