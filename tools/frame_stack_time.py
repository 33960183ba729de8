"""Timing of the actor's observation history (README "Frame stack"):

  python tools/frame_stack_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      (1) the env step alone (HIP events around 48 steps of fixed random actions, best of 5, as tools/height_scan_time.py) with env.frame_stack 1, 5
          and 10, in alternating order: us per step; and the bg_obs_stack launch alone: HIP events around 200 back-to-back T1.reset() calls (the
          reset-all launch: no physics), best of 5; the difference to frame_stack 1 is the stack launch;
      (2) the rollout actor launch (HIP events around 200 sample_actions calls, best of 5): bg_actor_sample at frame_stack 1, bg_actor_sample_mlp on
          47 H inputs at 5 and 10, the reference's widths;
      (3) the training loop (no instrumentation) at frame_stack 1, 5 and 10, three runners on one GPU, alternating runs of K iterations after W
          warm-up iterations each: ms per iteration, iterations per second, ratio to the frame_stack 1 runner of the same process.  With a stack
          the actor runs the per-layer kernels instead of the chained ones (its input pads to 256 / 512) and the rollout's forward-ahead is off."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

STACKS = (1, 5, 10)


def _cfg(N, H):
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "trimesh", "env.frame_stack": H, "env.num_observations": 47 * H})
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


def _orders(p):
    return STACKS if p % 2 == 0 else STACKS[::-1]


def env_step(pairs=3, N=4096):
    from booster_gym_amd.envs import T1

    envs = {H: T1(_cfg(N, H)) for H in STACKS}
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand(N, 12, generator=g) * 0.6 - 0.3).to("cuda:0") for _ in range(8)]
    for env in envs.values():
        env.reset()
        for k in range(40):
            env.step(acts[k % 8])
    for p in range(pairs):
        us = {H: _best(lambda k, e=envs[H]: e.step(acts[k % 8]), 48) for H in _orders(p)}
        print(f"env step, {N} envs, trimesh: " + ", ".join(f"frame_stack {H} {us[H]:.2f} us" for H in STACKS)
              + "; " + ", ".join(f"{H} / 1 = {us[H] / us[1]:.4f}" for H in STACKS[1:]), flush=True)
    for p in range(pairs):
        us = {H: _best(lambda k, e=envs[H]: e.reset(), 200) for H in _orders(p)}
        print(f"reset-all, {N} envs: " + ", ".join(f"frame_stack {H} {us[H]:.2f} us" for H in STACKS) + "; the bg_obs_stack launch "
              + ", ".join(f"H = {H}: {us[H] - us[1]:.2f} us" for H in STACKS[1:]), flush=True)
    del envs


def actor(pairs=3, N=4096):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(0)
    nets = {H: ActorCritic(12, 47 * H, 14).to("cuda:0") for H in STACKS}
    obs = {H: torch.randn(N, 47 * H, device="cuda:0") for H in STACKS}
    out = torch.empty(N, 12, device="cuda:0")
    for p in range(pairs):
        us = {H: _best(lambda k, H=H: nets[H].sample_actions(obs[H], out, 1, k), 200) for H in _orders(p)}
        print(f"rollout actor, {N} rows, 256-128-128: " + ", ".join(f"frame_stack {H} {us[H]:.2f} us" for H in STACKS)
              + " (1: bg_actor_sample; 5, 10: bg_actor_sample_mlp)", flush=True)


def _runner(N, H):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, H)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_frame_stack_"), rank=0))
    return r


def loop(K=20, W=5, pairs=3, N=4096):
    runners = {H: _runner(N, H) for H in STACKS}
    it = {H: 0 for H in STACKS}

    def run(H, n):
        r = runners[H]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it[H]); it[H] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for H in STACKS:
        run(H, W)
    for p in range(pairs):
        ms = {H: run(H, K) for H in _orders(p)}
        for H in STACKS:
            print(f"frame_stack {H:2d}, {N} envs: {ms[H]:.3f} ms per iteration = {1e3 / ms[H]:.2f} iterations/s", flush=True)
        print(f"round {p}: " + ", ".join(f"{H} / 1 = {ms[H] / ms[1]:.4f}" for H in STACKS[1:]), flush=True)
    for r in runners.values():
        r._flush_log()
    del runners


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    pairs, N = (a[2] if len(a) > 2 else 3), (a[3] if len(a) > 3 else 4096)
    env_step(pairs, N)
    actor(pairs, N)
    loop(*a)
