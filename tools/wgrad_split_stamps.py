"""Where a 16-row block of the split weight-gradient kernel spends its cycles: per-wave sums of shader-clock cycles over all blocks (probe build
tools/build_stamps.sh bg_wgrad_split; BG_LIB=tools/probe/bg_wgrad_split_stamps.so python tools/wgrad_split_stamps.py [terms]).  Each of the four shapes
runs ALONE with the slices the six-layer plan of the update gives it.  Per shape, the median over all waves of the first 1024 workgroups: cycles per
block next to its MFMA cycles, the share of a block spent at its top in the counted wait + barrier and in issuing the copies that are still a burst
there (the copies dealt behind MFMAs are inside the rest), the epilogue, and the shader clock (loop cycles over its 100 MHz wall-clock ticks)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from booster_gym_amd import _lib
from booster_gym_amd.utils.model import plan_wgrad_slices
lib = _lib.load(); st = _lib.current_stream_ptr(); dev = "cuda:0"
lib.bg_probe_read_wgrad_split_stamps.restype = C.c_int; lib.bg_probe_read_wgrad_split_stamps.argtypes = [C.c_void_p, C.c_size_t]
terms = int(sys.argv[1]) if len(sys.argv) > 1 else 9
M = 98304
six = [(128, 256, 256), (256, 256, 256), (256, 64, 61), (128, 128, 128), (128, 256, 256), (256, 64, 47)]
slices, tw = plan_wgrad_slices([(co, ci) for co, ci, _ in six], M, 256, share_rows=True)
g = torch.Generator(device="cpu").manual_seed(3)
print(f"split weight gradients, {terms} products, M = {M}, each shape alone; cycles are medians over waves")
print("shape      slices  blocks  cycles/block  (MFMA)   wait+barrier   burst issue   epilogue cycles   clock GHz   launch us")
for k in (1, 0, 3, 2):
    (co, ci, cr), sl = six[k], slices[k]
    ks = 4 // tw[k]
    G = (torch.randn(M, co, generator=g) * 0.01).to(dev)
    A = torch.zeros(M, ci); A[:, :cr] = torch.nn.functional.elu(torch.randn(M, cr, generator=g)); A = A.to(dev)
    dW = torch.empty(co, cr, device=dev); sc = torch.empty(sl * co * ci, device=dev)
    arr = (_lib.WgradProblem * 1)()
    arr[0].G, arr[0].A, arr[0].dW, arr[0].scratch = G.data_ptr(), A.data_ptr(), dW.data_ptr(), sc.data_ptr()
    arr[0].M, arr[0].C_out, arr[0].C_in, arr[0].C_in_real, arr[0].slices, arr[0].tiles_per_workgroup = M, co, ci, cr, sl, tw[k]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(6):
        if it == 5: e0.record()
        _lib.check(lib.bg_mlp_weight_grad_group_split_partial(arr, 1, terms, st), "split")
    e1.record(); torch.cuda.synchronize()
    buf = np.zeros(1024 * 4 * 5, dtype=np.int64)
    assert lib.bg_probe_read_wgrad_split_stamps(buf.ctypes.data, buf.nbytes) == 0
    n = min(sl, 1024)  # one workgroup per slice: the shape's tiles share a workgroup
    t = buf.reshape(1024, 4, 5)[:n].astype(np.float64)
    nb2, w = M // 32, sl * ks
    blocks = np.array([max(2 * (nb2 * (s * ks + c + 1) // w) - 2 * (nb2 * (s * ks + c) // w) for c in range(ks)) for s in range(n)], dtype=np.float64)[:, None]
    med = lambda a: float(np.median(a))
    per_block, wait, issue = med(t[:, :, 2] / blocks), med(t[:, :, 0] / t[:, :, 2]), med(t[:, :, 1] / t[:, :, 2])
    ghz = med(t[:, :, 2] / np.maximum(1.0, t[:, :, 4])) * 0.1
    mfma = 4 * (2 if ci == 64 else 4) * terms * 32
    print(f"{co:3d}x{ci:<3d}   {sl:6d}  {med(blocks):6.0f}  {per_block:12.0f}  ({mfma:4d})   {100 * wait:11.1f}%   {100 * issue:10.1f}%   {med(t[:, :, 3]):15.0f}   {ghz:9.2f}   {e0.elapsed_time(e1) * 1e3:9.1f}", flush=True)
