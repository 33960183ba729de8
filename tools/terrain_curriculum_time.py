"""Timing of the terrain curriculum (README "Terrain curriculum"):

  python tools/terrain_curriculum_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      (1) the training loop (as tools/symmetry_time.py, no instrumentation) on the trimesh terrain with terrain.curriculum off and on, two runners on
          one GPU, timed in alternating runs of K iterations after W warm-up iterations each: ms per iteration, iterations per second, ratio on / off;
      (2) the env step alone (HIP events around 48 steps of fixed random actions, best of 5, as tools/ab_sim.py) off and on, alternating: us per step.
  The curriculum's own work runs only at resets; what else differs is the height field, 5.5 x larger at 10 levels (1.98 MB of int16)."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch


def _cfg(N, on):
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "trimesh", "terrain.curriculum": on})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    return cfg


def _runner(N, on):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, on)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_terrain_curriculum_"), rank=0))
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
            print(f"terrain curriculum {'on ' if on else 'off'}, {N} envs: {ms[on]:.3f} ms per iteration = {1e3 / ms[on]:.2f} iterations/s", flush=True)
        print(f"pair {p}: on / off = {ms[True] / ms[False]:.4f}", flush=True)
    for r in runners.values():
        r._flush_log()
    lv = runners[True].env.terrain_levels.double().mean().item()
    print(f"mean terrain level after {it[True]} iterations: {lv:.3f}", flush=True)
    del runners


def env_step(pairs=3, N=4096):
    from booster_gym_amd.envs import T1

    envs = {on: T1(_cfg(N, on)) for on in (False, True)}
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand(N, 12, generator=g) * 0.6 - 0.3).to("cuda:0") for _ in range(8)]
    for env in envs.values():
        env.reset()
        for k in range(40):
            env.step(acts[k % 8])

    def best(env):
        b = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(48):
                env.step(acts[k % 8])
            e1.record(); torch.cuda.synchronize()
            b = min(b, e0.elapsed_time(e1) / 48 * 1e3)
        return b

    for p in range(pairs):
        us = {on: best(envs[on]) for on in ((False, True) if p % 2 == 0 else (True, False))}
        print(f"env step, {N} envs, trimesh: off {us[False]:.2f} us, on {us[True]:.2f} us, on / off = {us[True] / us[False]:.4f}", flush=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    loop(*a)
    env_step(a[2] if len(a) > 2 else 3, a[3] if len(a) > 3 else 4096)
