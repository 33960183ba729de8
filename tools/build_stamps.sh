#!/bin/bash
# Builds tools/probe/<kernel>_stamps.so: the product library with ONE source file (bg_mlp_chain, bg_mlp_chain_split, bg_mlp_chain_split_bwd, bg_wgrad_split, or bg_ppo
# for the rollout's actor_sample_kernel) compiled with the clock stamps of booster_gym_amd/csrc/bg_stamps.h, for that kernel's decoder (tools/mlp_chain_stamps.py,
# tools/chain_split_stamps.py, tools/chain_split_bwd_stamps.py, tools/wgrad_split_stamps.py, tools/actor_sample_stamps.py).  The compile and link lines are the Makefile's.
#   tools/build_stamps.sh bg_mlp_chain_split && BG_LIB=tools/probe/bg_mlp_chain_split_stamps.so python tools/chain_split_stamps.py
set -e
[ $# = 1 ] || { echo "usage: $0 bg_mlp_chain | bg_mlp_chain_split | bg_mlp_chain_split_bwd | bg_wgrad_split | bg_ppo" >&2; exit 2; }
K=$(basename "$1" .hip)
make -C "$(dirname "$0")/../booster_gym_amd/csrc" -j16 ../../tools/probe/${K}_stamps.so
