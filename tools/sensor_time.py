"""Timing of the sensor model (README "Sensor model"):

  python tools/sensor_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      (1) the launch alone: HIP events around 200 back-to-back T1.reset() calls (the reset-all launch sequence: no physics), best of 5, at
          env.frame_stack 1 and 5, section off against on (full bias, latency_steps [0, 1.5]), sides alternating: at H = 5 the difference is
          bg_obs_sensor against bg_obs_stack, at H = 1 off has no such launch and the difference is the added launch.  A reset-all draws every
          env's bias and latency, so this is the launch at its dearest; the same launch on steps without resets is inside (2);
      (2) the env step (HIP events around 48 steps of fixed random actions, best of 5), on against off, at both H: us per step;
      (3) the training loop (no instrumentation) at H = 1, two runners on one GPU, alternating runs of K iterations after W warm-up iterations
          each: ms per iteration, on / off.

  python tools/sensor_time.py bench PARENT_DIR [pairs=3]
      the default path: `python bench.py --gpus 1 --steps 20 --warmup 5` of this tree and of a built checkout of the parent commit at PARENT_DIR,
      in alternating fresh processes, and in each tree the SHA-256 over the parameters after two default iterations at 4096 envs."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the repository root
import torch

STACKS = (1, 5)
SIDES = ("off", "on")
GAUSS = lambda a, b: {"range": [a, b], "operation": "additive", "distribution": "gaussian"}
SENSORS = {"enabled": True, "latency_steps": [0.0, 1.5],
           "bias": {"gravity": GAUSS(0.0, 0.05), "ang_vel": GAUSS(0.0, 0.1), "dof_pos": GAUSS(0.0, 0.02), "dof_vel": GAUSS(0.0, 0.5)}}


def _cfg(N, H, side):
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "trimesh", "env.frame_stack": H, "env.num_observations": 47 * H})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    if side == "on":
        cfg["sensors"] = SENSORS
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
    return SIDES if p % 2 == 0 else SIDES[::-1]


def env_step(pairs=3, N=4096):
    from booster_gym_amd.envs import T1

    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand(N, 12, generator=g) * 0.6 - 0.3).to("cuda:0") for _ in range(8)]
    for H in STACKS:
        envs = {s: T1(_cfg(N, H, s)) for s in SIDES}
        for env in envs.values():
            env.reset()
            for k in range(40):
                env.step(acts[k % 8])
        for p in range(pairs):
            us = {s: _best(lambda k, e=envs[s]: e.reset(), 200) for s in _orders(p)}
            what = "bg_obs_sensor - bg_obs_stack" if H > 1 else "the added bg_obs_sensor launch"
            print(f"reset-all, {N} envs, frame_stack {H}: off {us['off']:.2f} us, on {us['on']:.2f} us; {what} {us['on'] - us['off']:.2f} us", flush=True)
        for p in range(pairs):
            us = {s: _best(lambda k, e=envs[s]: e.step(acts[k % 8]), 48) for s in _orders(p)}
            print(f"env step, {N} envs, trimesh, frame_stack {H}: off {us['off']:.2f} us, on {us['on']:.2f} us; on / off = {us['on'] / us['off']:.4f}", flush=True)
        assert envs["off"].sensor_launches == 0 and envs["on"].sensor_launches > 0
        del envs


def _runner(N, side):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, 1, side)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_sensor_time_"), rank=0))
    return r


def loop(K=20, W=5, pairs=3, N=4096):
    runners = {s: _runner(N, s) for s in SIDES}
    it = {s: 0 for s in SIDES}

    def run(s, n):
        r = runners[s]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it[s]); it[s] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for s in SIDES:
        run(s, W)
    for p in range(pairs):
        ms = {s: run(s, K) for s in _orders(p)}
        print(f"training loop, {N} envs, frame_stack 1: off {ms['off']:.3f} ms, on {ms['on']:.3f} ms per iteration; on / off = {ms['on'] / ms['off']:.4f}", flush=True)
    for r in runners.values():
        r._flush_log()
    del runners


# SHA-256 over the parameters and Adam moments after two default iterations, run with a tree's root as the working directory and first import path
SHA_CODE = """
import hashlib, os, sys, tempfile
sys.path.insert(0, os.getcwd())
import torch
import booster_gym_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(booster_gym_amd.__file__))) == os.getcwd()
from booster_gym_amd.utils.config import load_cfg
from booster_gym_amd.utils.recorder import Recorder
from booster_gym_amd.utils.runner import Runner
cfg = load_cfg("T1", {"env.num_envs": 4096})
cfg["runner"]["save_interval"] = 10 ** 9
r = Runner(cfg=cfg)
r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_sensor_time_"), rank=0))
for it in range(2):
    r.train_iteration(it)
r._flush_log()
torch.cuda.synchronize()
o, h = r.optimizer, hashlib.sha256()
for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr]:
    h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
print("SHA " + h.hexdigest())
"""


def bench(parent, pairs=3):
    trees = {"this": ROOT, "parent": os.path.abspath(parent)}
    for name, tree in trees.items():
        out = subprocess.run([sys.executable, "-c", SHA_CODE], cwd=tree, capture_output=True, text=True, timeout=600)
        got = [l[4:] for l in out.stdout.splitlines() if l.startswith("SHA ")]
        if out.returncode != 0 or not got:  # (nothing more is started on the GPU behind a child that failed)
            sys.exit(f"sha-256 after two default iterations, {name}: exit status {out.returncode}\n{out.stderr[-2000:]}")
        print(f"sha-256 after two default iterations, {name}: {got[-1]}", flush=True)
    for p in range(pairs):
        vals = {}
        for name in (("this", "parent") if p % 2 == 0 else ("parent", "this")):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=trees[name], capture_output=True, text=True, timeout=900)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode != 0 or not line:
                sys.exit(f"bench pair {p}, {name}: exit status {out.returncode}\n{out.stderr[-2000:]}")
            vals[name] = json.loads(line[-1])
            print(f"bench pair {p}, {name}: {vals[name]['value'] / 1e6:.4f} M env-steps/s, {vals[name]['ms_per_step']:.3f} ms per step", flush=True)
        print(f"bench pair {p}: this / parent = {vals['this']['value'] / vals['parent']['value']:.4f}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "bench":
        bench(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    else:
        a = [int(x) for x in sys.argv[1:]]
        pairs, N = (a[2] if len(a) > 2 else 3), (a[3] if len(a) > 3 else 4096)
        env_step(pairs, N)
        loop(*a)
