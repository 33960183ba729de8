"""Timing of the critic's terrain height scan (README "Terrain height scan"):

  python tools/height_scan_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      (1) the env step alone (HIP events around 48 steps of fixed random actions, best of 5, as tools/terrain_curriculum_time.py) with
          terrain.measure_heights off and on (the default 17 x 11 grid), alternating: us per step;
      (2) the bg_height_scan launch alone: HIP events around 200 back-to-back T1.reset() calls (the reset-all launch: no physics) off and on,
          best of 5; the difference is the scan launch;
      (3) the training loop (as tools/terrain_curriculum_time.py, no instrumentation) off and on, two runners on one GPU, alternating runs of K
          iterations after W warm-up iterations each: ms per iteration, iterations per second, ratio on / off.  With the scan the critic runs the
          per-layer kernels instead of the chained ones (its input pads to 256) and the rollout's forward-ahead is off."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

P = 187


def _cfg(N, on):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "terrain.type": "trimesh", "terrain.measure_heights": on, "env.num_privileged_obs": 14 + (P if on else 0)}
    cfg = load_cfg("T1", ov)
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    return cfg


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


def env_step(pairs=3, N=4096):
    from booster_gym_amd.envs import T1

    envs = {on: T1(_cfg(N, on)) for on in (False, True)}
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand(N, 12, generator=g) * 0.6 - 0.3).to("cuda:0") for _ in range(8)]
    for env in envs.values():
        env.reset()
        for k in range(40):
            env.step(acts[k % 8])
    for p in range(pairs):
        order = (False, True) if p % 2 == 0 else (True, False)
        us = {on: _best(lambda k, e=envs[on]: e.step(acts[k % 8]), 48) for on in order}
        print(f"env step, {N} envs, trimesh: scan off {us[False]:.2f} us, on {us[True]:.2f} us, on / off = {us[True] / us[False]:.4f}", flush=True)
    for p in range(pairs):
        order = (False, True) if p % 2 == 0 else (True, False)
        us = {on: _best(lambda k, e=envs[on]: e.reset(), 200) for on in order}
        print(f"reset-all, {N} envs: scan off {us[False]:.2f} us, on {us[True]:.2f} us, difference (the bg_height_scan launch) "
              f"{us[True] - us[False]:.2f} us", flush=True)
    del envs


def _runner(N, on):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, on)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_height_scan_"), rank=0))
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
            print(f"height scan {'on ' if on else 'off'}, {N} envs: {ms[on]:.3f} ms per iteration = {1e3 / ms[on]:.2f} iterations/s", flush=True)
        print(f"pair {p}: on / off = {ms[True] / ms[False]:.4f}", flush=True)
    for r in runners.values():
        r._flush_log()
    del runners


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    env_step(a[2] if len(a) > 2 else 3, a[3] if len(a) > 3 else 4096)
    loop(*a)
