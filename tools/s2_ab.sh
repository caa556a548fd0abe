#!/bin/bash
# A/B of the stride-2 CostRegNet2D layers on the GPU box: the direct kernel (ADAMVS_S2_PAIRS=0) against the pair form (round 5).
# The cfg2 headline under both settings through tools/ab.sh (value, ms per step, phase table and CostRegNet2D layer times).
cd "$(dirname "$0")/.."
SHOW=5 tools/ab.sh s2ab "ADAMVS_S2_PAIRS=0|ADAMVS_S2_PAIRS=1" "cfg2="
