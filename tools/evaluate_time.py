"""Timing of evaluate.py (README "Evaluation", profiles/evaluate_time.txt):

  python tools/evaluate_time.py train OUT.pth [iterations=30] [num_envs=4096]
      a checkpoint from a short training run (plane, shipped config otherwise): what the loops below evaluate
  python tools/evaluate_time.py loop CHECKPOINT [num_envs=4096] [steps=1502]
      the evaluation loop (plane, shipped config): HIP events around the whole loop, ending in a synchronise (Evaluator.loop_s); one line
  python tools/evaluate_time.py launches [num_envs=4096] [steps=60]
      60 env steps with env.frame_stack: 2, each followed by bg_env_eval_step, and nothing else: the run to put under a kernel trace
      (rocprofv3 --kernel-trace --stats -- python tools/evaluate_time.py launches), where bg_eval_step stands beside bg_obs_stack, a launch of the
      same kind (one pass over a few hundred kB per step) at the same env count
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

PLANE = {"terrain.type": "plane"}


def train(out, iterations=30, N=4096):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    r = Runner(cfg=load_cfg("T1", dict(PLANE, **{"env.num_envs": N})))
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs)
    r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    for _ in range(iterations):
        r.iteration()
    torch.cuda.synchronize()
    torch.save(r.checkpoint_dict(), out)
    print(f"saved {out} after {iterations} iterations at {N} envs")


def loop(checkpoint, N=4096, steps=1502):
    from booster_gym_amd.utils.evaluate import Evaluator

    ev = Evaluator(checkpoint=checkpoint, overrides=dict(PLANE, **{"env.num_envs": N}))
    rep = ev.run(steps)
    a = rep["all"]
    print(f"evaluation loop, {N} envs, {steps} steps, plane: {ev.loop_s:.4f} s = {ev.loop_s / steps * 1e6:.1f} us per step = "
          f"{N * steps / ev.loop_s:,.0f} env-steps/s; fell {a['fell']}, timed out {a['timed_out']}, unfinished {a['unfinished']}", flush=True)


def launches(N=4096, steps=60):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    env = T1(load_cfg("T1", dict(PLANE, **{"env.num_envs": N, "env.frame_stack": 2, "env.num_observations": 94})))
    g = torch.Generator(device="cpu").manual_seed(0)
    act = (torch.rand(N, 12, generator=g) * 0.2 - 0.1).to(env.device)
    env.reset()
    record = env.eval_begin()
    for _ in range(steps):
        env.step(act)
        env.eval_step(record, 5)
    torch.cuda.synchronize()
    print(f"{steps} env steps with env.frame_stack 2 and bg_env_eval_step at {N} envs; still running: {int((record[0] == 0).sum())}")


if __name__ == "__main__":
    what, args = sys.argv[1], sys.argv[2:]
    if what == "train":
        train(args[0], *[int(a) for a in args[1:]])
    elif what == "loop":
        loop(args[0], *[int(a) for a in args[1:]])
    elif what == "launches":
        launches(*[int(a) for a in args])
    else:
        raise SystemExit(__doc__)
