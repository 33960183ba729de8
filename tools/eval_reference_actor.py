"""How well does a policy trained by the REFERENCE (PhysX TGS, Isaac Gym) survive and track in this build's simulator?

The reference ships one trained actor (deploy/models/T1.pt; its weights only are kept as tests/golden/t1_actor.npz).  Its weights encode the
PhysX dynamics it was trained on, so its behaviour here is the one quantitative statement about PhysX-versus-this-contact-model that can be made
offline (MuJoCo and Isaac Gym are absent).  The protocol is evaluate.py's (booster_gym_amd/utils/evaluate.py, README "Evaluation"): the actor's
mean action drives `num_envs` robots through their first episode under the SHIPPED envs/T1.yaml -- observation noise, domain randomisation,
actuation latency, kicks and pushes all on, commands resampled as in training -- and every scenario's report has that tool's keys.  This file
keeps the scenario list (terrain x asset.self_collisions, and one run without noise, kicks and pushes) and the contact-parameter sweep.

    python tools/eval_reference_actor.py [num_envs=4096] [steps=1502] [--sweep] [--gait] [--checkpoint logs/.../model.pth] -> logs/reference_actor_eval.json
(--checkpoint: the same scenarios for an actor trained by THIS build -> logs/own_actor_eval.json: the yardstick for the reference actor's numbers;
--gait: evaluation.gait: true in every scenario, whose gait table is printed and whose report carries the "gait" entries)

`evaluate()` below, with its own torch actor and accumulators, is the protocol of before evaluate.py existed (whole run instead of first episode,
tracking sampled every fifth step).  tests/test_gpu_env.py::test_trained_reference_policy_walks_on_the_gpu holds bounds on its figures, so it stays
for that test alone; main() no longer calls it.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from booster_gym_amd.envs import T1
from booster_gym_amd.utils.config import load_cfg
from booster_gym_amd.utils.evaluate import Evaluator, format_report


GAIT = False  # --gait: every scenario keeps the gait record too
ACTOR_CHECKPOINT = None  # --checkpoint <.pth of this build's Runner>: evaluate that actor instead (how a policy TRAINED HERE fares under the same protocol)


def load_actor(dev):
    if ACTOR_CHECKPOINT:
        sd = torch.load(ACTOR_CHECKPOINT, map_location=dev, weights_only=True)["model"]
        W = {k[len("actor."):]: v.float() for k, v in sd.items() if k.startswith("actor.")}
        layers = [(W[f"{i}.weight"].to(dev), W[f"{i}.bias"].to(dev)) for i in (0, 2, 4, 6)]
    else:
        W = np.load(os.path.join(ROOT, "tests", "golden", "t1_actor.npz"))
        layers = [(torch.tensor(W[f"{i}.weight"], device=dev), torch.tensor(W[f"{i}.bias"], device=dev)) for i in (0, 2, 4, 6)]

    def actor(x):
        for k, (w, b) in enumerate(layers):
            x = torch.addmm(b, x, w.T)
            if k < 3:
                x = torch.nn.functional.elu(x)
        return x

    return actor


def evaluate_first_episode(n, steps, overrides, seed=42):
    """One scenario under evaluate.py's protocol: its report, with the loop's time."""
    over = dict({"env.num_envs": n, "basic.seed": seed}, **overrides)
    if GAIT:
        over["evaluation.gait"] = True
    if ACTOR_CHECKPOINT:
        ev = Evaluator(checkpoint=ACTOR_CHECKPOINT, overrides=over)
    else:
        with np.load(os.path.join(ROOT, "tests", "golden", "t1_actor.npz")) as W:
            ev = Evaluator(actor={k: W[k] for k in W.files}, overrides=over)
    rep = ev.run(steps)
    rep["scenario_overrides"], rep["loop_s"] = overrides, ev.loop_s
    if GAIT:
        print(format_report(rep), flush=True)
    del ev
    return rep


def evaluate(n, steps, overrides, seed=42):
    cfg = load_cfg("T1", dict({"env.num_envs": n, "basic.seed": seed}, **overrides))
    env = T1(cfg)
    dev = env.device
    actor = load_actor(dev)
    obs, _ = env.reset()
    first_done = torch.zeros(n, dtype=torch.bool, device=dev)   # the first episode of this robot has ended
    first_fell = torch.zeros(n, dtype=torch.bool, device=dev)
    first_len = torch.zeros(n, dtype=torch.int32, device=dev)    # length of the first episode
    fall_cmd = torch.zeros(n, 3, device=dev)                     # the command a robot had when its first episode ended in a fall
    cmd_prev = env.commands
    falls = torch.zeros((), dtype=torch.float64, device=dev)
    sq = torch.zeros(3, dtype=torch.float64, device=dev); cnt = torch.zeros(3, dtype=torch.float64, device=dev)
    sq0 = torch.zeros(3, dtype=torch.float64, device=dev); cnt0 = torch.zeros(3, dtype=torch.float64, device=dev)
    terms = {k: torch.zeros((), dtype=torch.float64, device=dev) for k in env.reward_names}
    rew_sum = torch.zeros((), dtype=torch.float64, device=dev)
    t0 = time.perf_counter()
    with torch.no_grad():
        for s in range(steps):
            obs, rew, done, extras = env.step(actor(obs))
            fell = done & ~extras["time_outs"]
            falls += fell.sum()
            newly = fell & ~first_done
            first_fell |= newly
            fall_cmd[newly] = cmd_prev[newly]
            first_len += (~first_done).int()
            first_done |= done
            cmd_prev = env.commands  # (a reset env already holds its next command)
            rew_sum += rew.double().sum()
            for k in terms:
                terms[k] += extras["rew_terms"][k].double().sum()
            if s % 5 == 0:  # tracking error, every fifth step
                cmd = cmd_prev
                v = torch.cat((env.get_field("filtered_lin_vel")[:, :2], env.get_field("filtered_ang_vel")[:, 2:3]), dim=1)
                settled = (env.episode_length_buf > 50)[:, None]
                err2 = (cmd - v).double() ** 2
                moving = (cmd.abs() > 1e-6) & settled
                still = (cmd.abs() <= 1e-6) & settled
                sq += (err2 * moving).sum(0); cnt += moving.sum(0)
                sq0 += (err2 * still).sum(0); cnt0 += still.sum(0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st = env.episode_stats(reset=False).double().cpu().numpy()  # finished episodes, sum of lengths, sum of reward, 26 term sums, non-finite resets
    ax = ("lin_vel_x", "lin_vel_y", "ang_vel_yaw")
    out = {"overrides": overrides, "num_envs": n, "steps": steps, "wall_s": wall,
           "fall_rate_first_episode": float(first_fell.double().mean()),
           "fell_within_steps": {str(k): float((first_fell & (first_len <= k)).double().mean()) for k in (100, 300, 500, 1000, 1500)},
           "mean_first_episode_length": float(first_len.double().mean()),
           "falls_by_command": {"standing (cmd = 0)": int((first_fell & (fall_cmd.abs().sum(1) == 0)).sum()),
                                "|vx| > 0.5": int((first_fell & (fall_cmd[:, 0].abs() > 0.5)).sum()), "|vy| > 0.5": int((first_fell & (fall_cmd[:, 1].abs() > 0.5)).sum()),
                                "|yaw| > 0.5": int((first_fell & (fall_cmd[:, 2].abs() > 0.5)).sum()), "all": int(first_fell.sum())},
           "falls_total": float(falls), "falls_per_robot_minute": float(falls) / (n * steps * env.dt / 60.0),
           "finished_episodes": float(st[0]), "mean_episode_length": float(st[1] / max(st[0], 1.0)),
           "first_episode_ran_to_the_time_out": float((first_done & ~first_fell).double().mean()),
           "tracking_rmse": {a: float(torch.sqrt(sq[i] / cnt[i].clamp(min=1))) for i, a in enumerate(ax)},
           "tracking_rmse_still": {a: float(torch.sqrt(sq0[i] / cnt0[i].clamp(min=1))) for i, a in enumerate(ax)},
           "mean_reward_per_step": float(rew_sum) / (n * steps),
           "reward_terms": {k: float(v) / (n * steps) for k, v in terms.items()},
           "nonfinite_resets": float(st[-1])}
    del env
    return out


def main():
    global ACTOR_CHECKPOINT, GAIT
    GAIT = "--gait" in sys.argv
    if "--checkpoint" in sys.argv:
        k = sys.argv.index("--checkpoint")
        ACTOR_CHECKPOINT = sys.argv[k + 1]
        del sys.argv[k : k + 2]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 4096
    steps = int(args[1]) if len(args) > 1 else None  # None: the episode length + 2, every first episode ends
    res = {"what": __doc__.split("\n\n")[0],
           "actor": f"{ACTOR_CHECKPOINT} (an actor trained by this build)" if ACTOR_CHECKPOINT else "tests/golden/t1_actor.npz (weights of the reference's deploy/models/T1.pt)",
           "config": "envs/T1.yaml as shipped",
           "scenarios": {}}

    def brief(r):
        g = r["all"]
        return {"fall_rate": g["fall_rate"], "unfinished": g["unfinished"], "mean_episode_length": g["mean_episode_length"],
                "tracking_rmse": g["tracking_rmse"], "mean_reward_per_step": g["mean_reward_per_step"]}

    for terrain in ("plane", "trimesh"):
        for sc in (0, 1):
            key = f"{terrain}/self_collisions={sc}"
            res["scenarios"][key] = r = evaluate_first_episode(n, steps, {"terrain.type": terrain, "asset.self_collisions": sc})
            print(key, brief(r), flush=True)
    # the same actor without the perturbations, to separate "the contact model differs" from "kicks, pushes and noise are hard"
    quiet = {"terrain.type": "plane", "noise.gravity": None, "noise.ang_vel": None, "noise.dof_pos": None, "noise.dof_vel": None,
             "randomization.kick_lin_vel": None, "randomization.kick_ang_vel": None, "randomization.push_force": None, "randomization.push_torque": None}
    res["scenarios"]["plane/no_noise_no_kicks_no_pushes"] = r = evaluate_first_episode(n, steps, quiet)
    print("quiet", brief(r), flush=True)
    if "--sweep" in sys.argv:
        # which contact parameter moves the fall rate: one at a time around the defaults (contact.* of T1.yaml), plane, shipped perturbations
        sweep = {}
        for name, values in (("contact.stiffness", (1.0e4, 2.0e4, 8.0e4, 1.6e5)), ("contact.damping", (150.0, 300.0, 1200.0, 2400.0)),
                             ("contact.friction_viscosity", (2.5e3, 5.0e3, 2.0e4, 4.0e4))):
            for v in values:
                sweep[f"{name}={v:g}"] = b = brief(evaluate_first_episode(n, steps, {"terrain.type": "plane", name: v}))
                print(name, v, b["fall_rate"], flush=True)
        res["contact_parameter_sweep_plane"] = sweep
    os.makedirs(os.path.join(ROOT, "logs"), exist_ok=True)
    name = "own_actor_eval.json" if ACTOR_CHECKPOINT else "reference_actor_eval.json"
    with open(os.path.join(ROOT, "logs", name), "w") as f:
        json.dump(res, f, indent=1)
    print("written logs/" + name)


if __name__ == "__main__":
    main()
