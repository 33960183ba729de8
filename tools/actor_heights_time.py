"""Timing of the actor's terrain height scan (README "Perceptive actor"):

  python tools/actor_heights_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      Configurations: "critic" = terrain.measure_heights alone (bg_height_scan, and bg_obs_stack with a frame stack), "actor" = the same with
      terrain.actor_heights (bg_obs_assemble in their place); H = 1 on the default 17 x 11 grid, H = 3 on a 9 x 5 grid (the critic's 512 inputs).
      (1) the env step alone (HIP events around 48 steps of fixed random actions, best of 5, as tools/height_scan_time.py), critic against actor,
          alternating: us per step;
      (2) the launches alone: HIP events around 200 back-to-back T1.reset() calls (the reset-all launch: no physics), best of 5, with the scan off
          altogether, critic and actor: the differences to "off" are bg_height_scan (+ bg_obs_stack) and bg_obs_assemble;
      (3) the rollout actor launch (HIP events around 200 sample_actions calls, best of 5) at K = 47 (bg_actor_sample) and K = 234;
      (4) the training loop (no instrumentation) critic against actor at H = 1, two runners on one GPU, alternating runs of K iterations after W
          warm-up iterations each: ms per iteration, iterations per second, ratio actor / critic."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

GRID_9x5 = {"terrain.measured_points_x": [round(-0.4 + 0.1 * i, 1) for i in range(9)], "terrain.measured_points_y": [-0.2, -0.1, 0.0, 0.1, 0.2]}
MODES = ("off", "critic", "actor")


def _cfg(N, mode, H=1):
    from booster_gym_amd.utils.config import load_cfg

    P = 0 if mode == "off" else (187 if H == 1 else 45)
    ov = {"env.num_envs": N, "terrain.type": "trimesh", "terrain.measure_heights": mode != "off", "terrain.actor_heights": mode == "actor",
          "env.frame_stack": H, "env.num_privileged_obs": 14 + P, "env.num_observations": 47 * H + (P if mode == "actor" else 0)}
    if H != 1:
        ov.update(GRID_9x5)
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


def _orders(p, keys):
    return keys if p % 2 == 0 else tuple(reversed(keys))


def env_step(pairs=3, N=4096):
    from booster_gym_amd.envs import T1

    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand(N, 12, generator=g) * 0.6 - 0.3).to("cuda:0") for _ in range(8)]
    for H in (1, 3):
        envs = {m: T1(_cfg(N, m, H)) for m in MODES}
        for env in envs.values():
            env.reset()
            for k in range(40):
                env.step(acts[k % 8])
        for p in range(pairs):
            us = {m: _best(lambda k, e=envs[m]: e.step(acts[k % 8]), 48) for m in _orders(p, ("critic", "actor"))}
            print(f"env step, {N} envs, trimesh, H = {H}: critic's scan {us['critic']:.2f} us, with the actor's {us['actor']:.2f} us, actor / critic = "
                  f"{us['actor'] / us['critic']:.4f}", flush=True)
        for p in range(pairs):
            us = {m: _best(lambda k, e=envs[m]: e.reset(), 200) for m in _orders(p, MODES)}
            print(f"reset-all, {N} envs, H = {H}: off {us['off']:.2f} us, critic {us['critic']:.2f} us, actor {us['actor']:.2f} us; bg_height_scan"
                  + (" + bg_obs_stack" if H > 1 else "") + f" {us['critic'] - us['off']:.2f} us, bg_obs_assemble {us['actor'] - us['off']:.2f} us"
                  + (" (off has its own bg_obs_stack launch: add it to both)" if H > 1 else ""), flush=True)
        del envs


def actor(pairs=3, N=4096):
    from booster_gym_amd.utils.model import ActorCritic

    nets = {47: ActorCritic(12, 47, 14).to("cuda:0"), 234: ActorCritic(12, 234, 201).to("cuda:0")}
    obs = {K: torch.randn(N, K, device="cuda:0") for K in nets}
    out = torch.empty(N, 12, device="cuda:0")
    for p in range(pairs):
        us = {K: _best(lambda k, K=K: nets[K].sample_actions(obs[K], out, 1, k, scan=187 if K == 234 else 0), 200) for K in _orders(p, (47, 234))}
        print(f"rollout actor, {N} rows, 256-128-128: K = 47 (bg_actor_sample) {us[47]:.2f} us, K = 234 (bg_actor_sample_mlp's kernel) {us[234]:.2f} us",
              flush=True)


def _runner(N, mode):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, mode)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_actor_heights_"), rank=0))
    return r


def loop(K=20, W=5, pairs=3, N=4096):
    runners = {m: _runner(N, m) for m in ("critic", "actor")}
    it = {m: 0 for m in runners}

    def run(m, n):
        r = runners[m]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it[m]); it[m] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for m in runners:
        run(m, W)
    for p in range(pairs):
        ms = {m: run(m, K) for m in _orders(p, ("critic", "actor"))}
        for m in ("critic", "actor"):
            print(f"{m:6s} scan, {N} envs: {ms[m]:.3f} ms per iteration = {1e3 / ms[m]:.2f} iterations/s", flush=True)
        print(f"pair {p}: actor / critic = {ms['actor'] / ms['critic']:.4f}", flush=True)
    for r in runners.values():
        r._flush_log()
    del runners


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    pairs, N = (a[2] if len(a) > 2 else 3), (a[3] if len(a) > 3 else 4096)
    env_step(pairs, N)
    actor(pairs, N)
    loop(*a)
