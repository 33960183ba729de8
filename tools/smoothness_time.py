"""Timing of the action-smoothness loss (README "Smoothness loss"):

  python tools/smoothness_time.py kernel [num_envs=4096]
      bg_partner_rows alone in both modes (HIP events around 50 back-to-back launches, best of 5) on the 24 x num_envs rows of the default shape
      (64 columns) and of a frame stack of 3 with the actor's 9 x 5 scan (256 columns), about a fifth of the rows cut: us per launch, bytes moved,
      TB/s, and the fraction of the 6.29 TB/s a float4 copy reaches on this part (README "Mini-batches")
  python tools/smoothness_time.py loop [K=20] [W=5] [pairs=3] [num_envs=4096]
      the training loop (as tools/symmetry_time.py, no instrumentation) three ways -- the key off, algorithm.smoothness_loss on (pairs "next" and
      "interpolate"), algorithm.symmetry_loss on -- four runners on one GPU, timed in alternating runs of K iterations after W warm-up iterations each:
      ms per iteration, iterations per second, and every ratio against the key off per pair"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

COPY_TBS = 6.29  # a float4 copy on this part (profiles/mini_batch_time.txt)


def _best(fn, n, reps=5):
    best = float("inf")
    for _ in range(reps):
        fn(0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(n):
            fn(k)
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / n)
    return best


def kernel(N=4096, T=24):
    from booster_gym_amd.utils.utils import partner_rows

    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(0)
    for what, cols in (("default shape", 64), ("frame_stack 3 + 9 x 5 scan", 256)):
        # four sets of buffers in rotation, so that a launch does not find its rows in the caches because the launch before left them there
        sets = [(torch.randn(T, N, cols, generator=g).to(dev), torch.randn(N, cols, generator=g).to(dev), torch.empty(T, N, cols, device=dev)) for _ in range(4)]
        dones, time_outs = (torch.rand(T, N, generator=g) < 0.1).to(dev), (torch.rand(T, N, generator=g) < 0.11).to(dev)
        cut = (dones | time_outs).float().mean().item()
        for mode in ("next", "interpolate"):
            us = _best(lambda k: partner_rows(*sets[k % 4][:2], dones, time_outs, sets[k % 4][2], mode, 42, 0, k), 50)
            rows_moved = 2.0 if mode == "next" else 3.0 - cut  # per row: one row written; one read (next, or a cut row), two read (interpolate, uncut)
            nbytes = T * N * (cols * 4 * rows_moved + 2)
            tbs = nbytes / us / 1e6
            print(f"bg_partner_rows, {mode}, {what}, {T * N} rows x {cols} floats, {100 * cut:.1f} % cut: {us:.2f} us per launch, {nbytes / 1e6:.1f} MB moved, "
                  f"{tbs:.3f} TB/s = {100 * tbs / COPY_TBS:.1f} % of a float4 copy's {COPY_TBS} TB/s", flush=True)


def _runner(N, over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "plane", **over})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_smoothness_"), rank=0))
    return r


def loop(K=20, W=5, pairs=3, N=4096):
    smooth = {"algorithm.smoothness_loss": True, "algorithm.smoothness_coef": 10.0}
    sides = {"key off": {}, "smoothness next": smooth, "smoothness interpolate": {**smooth, "algorithm.smoothness_pairs": "interpolate"},
             "symmetry loss": {"algorithm.symmetry_loss": True}}
    runners = {k: _runner(N, o) for k, o in sides.items()}
    it = dict.fromkeys(sides, 0)

    def run(k, n):
        r = runners[k]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it[k]); it[k] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for k in sides:
        run(k, W)
    for p in range(pairs):
        order = list(sides) if p % 2 == 0 else list(sides)[::-1]
        ms = {k: run(k, K) for k in order}
        for k in sides:
            print(f"{k}, {N} envs: {ms[k]:.3f} ms per iteration = {1e3 / ms[k]:.2f} iterations/s", flush=True)
        print(f"pair {p}: " + ", ".join(f"{k} / key off = {ms[k] / ms['key off']:.3f}" for k in sides if k != "key off"), flush=True)
    for r in runners.values():
        r._flush_log()


if __name__ == "__main__":
    {"kernel": kernel, "loop": loop}[sys.argv[1]](*[int(a) for a in sys.argv[2:]])
