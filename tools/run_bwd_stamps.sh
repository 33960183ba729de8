# The backward split chain's test, then its clock stamps (library of tools/build_stamps.sh bg_mlp_chain_split_bwd, built beforehand), from the
# repository root: tools/run_bwd_stamps.sh [critic_wgs actor_wgs]
mkdir -p gpurun_out/r06
timeout -k 10 300 python -m pytest tests/test_gpu_mlp_chain_split_bwd.py -x -q 2>&1 | tail -4 > gpurun_out/r06/bwd_test_v3.log; cat gpurun_out/r06/bwd_test_v3.log
BG_LIB=$PWD/tools/probe/bg_mlp_chain_split_bwd_stamps.so timeout -k 10 200 python tools/chain_split_bwd_stamps.py $1 $2 2>&1
