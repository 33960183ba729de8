"""Timing of the shuffled mini-batches (README "Mini-batches"):

  python tools/mini_batch_time.py [K=20] [W=5] [rounds=3] [num_envs=4096] [default_only=0]
      (1) bg_perm_fill and bg_gather_rows alone (HIP events around 50 back-to-back launches, best of 5) on the 24 x num_envs rows of the default
          shape (two inputs of 64 columns, actions, old mu, three scalars: 155 floats per row) and of env.frame_stack 3 with the height scan (inputs
          of 512 and 256 columns): us per launch, bytes moved (every row read once and written once, the permutation read once per stream),
          fraction of the 8 TB/s HBM peak and of the 6.29 TB/s a float4 copy reaches;
      (2) the training loop (no instrumentation) with runner.num_mini_batches absent, 2, 4 and 8: one runner at a time in turn, `rounds` runs of K
          iterations after W warm-up iterations each: ms per iteration, iterations per second, ratio to the absent key.
      default_only=1: (2) with the key absent only and one JSON line per round -- what an alternating comparison of two checkouts runs in each."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

DEV = "cuda:0"
HBM_PEAK, HBM_COPY = 8.0, 6.29  # TB/s: the part's peak, and what a float4 copy kernel reaches on it


def _best(fn, reps, rounds=5):
    b = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(reps):
            fn(k)
        e1.record(); torch.cuda.synchronize()
        b = min(b, e0.elapsed_time(e1) / reps * 1e3)
    return b


def kernels(N=4096, T=24):
    from booster_gym_amd import _lib

    lib, B = _lib.load(), T * N
    perm = torch.zeros(B, dtype=torch.int32, device=DEV)
    fill = lambda k: _lib.check(lib.bg_perm_fill(B, 42, 0, k, _lib.ptr(perm), _lib.current_stream_ptr()), "bg_perm_fill")
    us = _best(fill, 50)
    print(f"bg_perm_fill, {B} indices: {us:.2f} us per launch", flush=True)
    for widths, what in (((64, 64, 12, 12, 1, 1, 1), "default shape"), ((512, 256, 12, 12, 1, 1, 1), "frame_stack 3 + height scan")):
        srcs = [torch.randn(B, w, device=DEV) for w in widths]
        dsts = [torch.empty_like(s) for s in srcs]
        arr = (_lib.GatherStream * len(srcs))(*[_lib.GatherStream(s.data_ptr(), d.data_ptr(), w, 0) for s, d, w in zip(srcs, dsts, widths)])
        # (a fresh permutation per launch, as in the loop: filled outside the timed launches)
        perms = [torch.randperm(B, device=DEV).to(torch.int32) for _ in range(4)]
        us = _best(lambda k: _lib.check(lib.bg_gather_rows(B, B, _lib.ptr(perms[k % 4]), arr, len(srcs), _lib.current_stream_ptr()), "bg_gather_rows"), 50)
        for s, d in zip(srcs, dsts):
            assert torch.equal(d, s[perms[49 % 4].long()])
        nbytes = 4 * B * (2 * sum(widths) + len(widths))
        tbs = nbytes / us / 1e6
        print(f"bg_gather_rows, {what}, {B} rows x {sum(widths)} floats in {len(widths)} streams: {us:.2f} us per launch, {nbytes / 1e6:.1f} MB moved, "
              f"{tbs:.3f} TB/s = {tbs / HBM_PEAK * 100:.1f} % of {HBM_PEAK} TB/s peak, {tbs / HBM_COPY * 100:.1f} % of a float4 copy's {HBM_COPY} TB/s", flush=True)


def _runner(N, K):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "plane"})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    cfg["runner"].pop("num_mini_batches", None)
    if K is not None:
        cfg["runner"]["num_mini_batches"] = K
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_mini_batch_"), rank=0))
    return r


def loop(iters=20, W=5, rounds=3, N=4096, default_only=0):
    base = {}
    for K in ((None,) if default_only else (None, 2, 4, 8)):
        r, it = _runner(N, K), 0
        for p in range(rounds + 1):
            n = W if p == 0 else iters
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(n):
                r.train_iteration(it); it += 1
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / n * 1e3
            if p == 0:
                continue
            if default_only:
                print(json.dumps({"num_envs": N, "round": p - 1, "ms_per_iteration": round(ms, 4), "iterations_per_s": round(1e3 / ms, 3)}), flush=True)
                continue
            base.setdefault(p, ms)
            print(f"num_mini_batches {'absent' if K is None else K}, {N} envs, round {p - 1}: {ms:.3f} ms per iteration = {1e3 / ms:.2f} iterations/s = "
                  f"{1e3 / ms * r.cfg['runner']['mini_epochs'] * (K or 1):.0f} optimiser steps/s, {ms / base[p]:.4f} x the absent key", flush=True)
        r._flush_log()
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    N = a[3] if len(a) > 3 else 4096
    if not (len(a) > 4 and a[4]):
        kernels(N)
    loop(*a)
