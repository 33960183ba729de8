"""Timing of the mirror-symmetry loss (README "Symmetry loss"):

  python tools/symmetry_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      the training loop (as tools/width_time.py loop, no instrumentation) with algorithm.symmetry_loss off and on, two runners on one GPU, timed in
      alternating runs of K iterations after W warm-up iterations each: ms per iteration, iterations per second, and the ratio on / off per pair"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch


def _runner(N, on):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "plane", "algorithm.symmetry_loss": on})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_symmetry_"), rank=0))
    return r


def loop(K=20, W=5, pairs=3, N=4096):
    runners = {on: _runner(N, on) for on in (False, True)}
    it = {False: 0, True: 0}

    def run(on, n):
        r = runners[on]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it[on]); it[on] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for on in (False, True):
        run(on, W)
    for p in range(pairs):
        ms = {on: run(on, K) for on in ((False, True) if p % 2 == 0 else (True, False))}
        for on in (False, True):
            print(f"symmetry loss {'on ' if on else 'off'}, {N} envs: {ms[on]:.3f} ms per iteration = {1e3 / ms[on]:.2f} iterations/s", flush=True)
        print(f"pair {p}: on / off = {ms[True] / ms[False]:.3f}", flush=True)
    for r in runners.values():
        r._flush_log()


if __name__ == "__main__":
    loop(*[int(a) for a in sys.argv[1:]])
