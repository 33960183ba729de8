"""Where a workgroup of the rollout's actor launch (actor_sample_kernel, bg_ppo.hip) spends its time: shader-clock stamps of every wave (probe build
tools/build_stamps.sh bg_ppo; BG_LIB=tools/probe/bg_ppo_stamps.so python tools/actor_sample_stamps.py [rows=4096]).  Per phase the median over the
workgroups of the cycles of wave 0 (which also runs the 12-neuron output layer and the sampling tail) and of the slowest wave.  The MFMAs are
asynchronous: "MFMAs" is the time to ISSUE a tile's chain (each MFMA waits for the one before it, so all but the last 32 cycles), the wait for the last
result falls into the tile's epilogue; global loads likewise: "issue" columns are issue time, the wait for the data falls where it is first used."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from booster_gym_amd import _lib
from booster_gym_amd.utils.model import ActorCritic

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
lib = _lib.load()
lib.bg_probe_read_actor_stamps.restype = C.c_int; lib.bg_probe_read_actor_stamps.argtypes = [C.c_void_p, C.c_size_t]
torch.manual_seed(0)
model = ActorCritic(12, 47, 14).cuda()
obs, act = torch.randn(N, 47, device="cuda"), torch.empty(N, 12, device="cuda")
for k in range(5):
    model.sample_actions(obs, act, 1, k)
torch.cuda.synchronize()
buf = np.zeros(256 * 4 * 32, dtype=np.int64)
assert lib.bg_probe_read_actor_stamps(buf.ctypes.data, buf.nbytes) == 0
t = buf.reshape(256, 4, 32)[: min(256, -(-N // 16))]
# slots: 0 start, 1 first two layers' weight loads issued, 2 observation tile in LDS (every load so far has landed), 3 barrier, layer 0: 4 + 2 j tile j's
# MFMAs issued, 5 + 2 j its epilogue stored (4 tiles), 12 layer 2's loads issued, 13 barrier, layer 1: 14 .. 17 (2 tiles), 18 layer 3's loads issued, 19
# barrier, layer 2: 20 .. 23 (2 tiles), 24 = 23, 25 barrier, layer 3 (wave 0 only): 26 27, 28 barrier, 29 tail done, 30 / 31 the 100 MHz wall clock
phases = [("weight loads of layers 0, 1: issue", 0, 1), ("observation tile: wait for all loads + LDS store", 1, 2), ("barrier", 2, 3)]
for name, s, tiles, nxt in (("layer 0", 4, 4, "layer 2's weight loads: issue"), ("layer 1", 14, 2, "layer 3's weight loads: issue"), ("layer 2", 20, 2, None), ("layer 3", 26, 1, None)):
    prev = s - 1
    mf = [(prev if j == 0 else s + 2 * j - 1, s + 2 * j) for j in range(tiles)]
    ep = [(s + 2 * j, s + 2 * j + 1) for j in range(tiles)]
    phases += [(f"{name}: MFMAs of {tiles} tile(s)", mf), (f"{name}: epilogue (ELU + LDS stores) of {tiles} tile(s)", ep)]
    last = s + 2 * tiles - 1
    if nxt:
        phases += [(nxt, last, last + 1)]
        last += 1
    if name == "layer 2":
        last += 1
    phases += [(f"barrier behind {name}", last, last + 1)]
phases += [("sampling tail (Philox, exp, stores)", 28, 29)]


def cycles(w, p):
    """cycles of phase p on wave(s) w: [workgroups, waves]; a wave that has no tile in a layer stamps nothing there (zeros) and counts 0"""
    spans = [(p[1], p[2])] if len(p) == 3 else p[1]
    tot = np.zeros(t[:, w, 0].shape)
    for a, b in spans:
        ta, tb = t[:, w, a], t[:, w, b]
        tot += np.where((ta > 0) & (tb > 0), tb - ta, 0)
    return tot


whole = t[:, :, 29] - t[:, :, 0]
ghz = np.median(whole / np.maximum(1, t[:, :, 31] - t[:, :, 30])) * 0.1
print(f"actor_sample_kernel, {N} rows, {t.shape[0]} workgroups: a workgroup's wave takes {np.median(whole):.0f} cycles (median; min {whole.min()}, max {whole.max()}) = "
      f"{np.median(whole) / ghz / 1e3:.2f} us at {ghz:.2f} GHz; 992 MFMAs x 32 cycles / 4 waves = 7936 cycles")
print(f"{'phase':62s} {'wave 0':>8s} {'slowest wave':>13s}   (cycles, median over the workgroups)")
s0 = s1 = 0.0
for p in phases:
    a, b = np.median(cycles(0, p)), np.median(cycles(slice(None), p).max(axis=1))
    s0 += a; s1 += b
    print(f"{p[0]:62s} {a:8.0f} {b:13.0f}")
print(f"{'sum':62s} {s0:8.0f} {s1:13.0f}")
