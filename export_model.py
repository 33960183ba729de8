"""python export_model.py --task=T1 [--checkpoint path|-1]: TorchScript export of the actor (reference export_model.py:8-30) so that
the reference's deployment code (deploy/utils/policy.py:9) can load what this framework trains.  The actor's widths are read from the checkpoint's tensors (any supported architecture, with or without the terrain height
scan, a frame stack or the actor's own height scan, exports without editing the YAML); the TorchScript module is still a plain Sequential.  A checkpoint trained with
algorithm.empirical_normalization carries its observation statistics: they are folded into the actor's first layer, so the exported module takes raw observations.
A recurrent actor (algorithm.rnn_hidden_size, or a student of distillation.student_memory: the checkpoint carries "memory.*", from which the cell's
width is read) exports as a STATEFUL module, utils/model.py's RecurrentActor; the script prints its contract."""
import argparse
import glob
import os

import torch

from booster_gym_amd.utils.config import load_cfg
from booster_gym_amd.utils.model import ActorCritic, EstimatorActor, RecurrentActor, hidden_of

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", required=True, type=str)
    ap.add_argument("--checkpoint", type=str, default="-1")
    args = ap.parse_args()
    cfg = load_cfg(args.task)
    ck = args.checkpoint
    if ck in ("-1", None):
        ck = sorted(glob.glob(os.path.join("logs", "**/*.pth"), recursive=True), key=os.path.getmtime)[-1]
    print("Loading model from {}".format(ck))
    ckpt = torch.load(ck, map_location="cpu", weights_only=True)
    sd = ckpt["model"]
    # the actor's input from the checkpoint (47, or 47 H with env.frame_stack), and the critic's privileged inputs too (14, or 14 + P with
    # terrain.measure_heights); only the actor is exported
    num_obs = int(sd["actor.0.weight"].shape[1])
    # estimator.enabled: the actor's row ends with E estimates of a network the checkpoint carries ("estimator.*"); the exported module computes
    # actor(cat(x, estimator(x)[:, :E])), so the deploy contract stays "47 H floats in, 12 out"
    est_args = {}
    if any(k.startswith("estimator.") for k in sd):
        targets = [int(i) for i in ckpt["estimator"]["targets"]]
        est_args = {"estimator_hidden": hidden_of(sd, "estimator"), "estimator_cols": len(targets)}
        num_obs -= len(targets)
        print("Actor input of {} columns: 47 x {} observations, then {} estimates of the privileged columns {} from the checkpoint's estimator "
              "(hidden {}); the exported module takes the {} observations and computes the estimates itself".format(
                  num_obs + len(targets), num_obs // 47, len(targets), targets, list(est_args["estimator_hidden"]), num_obs))
    # distillation.student_memory: a GRU cell `memory` reads the observation and the actor reads the cell's state
    if "memory.weight_ih" in sd:
        est_args = {"memory_hidden": int(sd["memory.weight_hh"].shape[1])}
        num_obs = int(sd["memory.weight_ih"].shape[1])
    num_priv = int(sd["critic.0.weight"].shape[1]) - num_obs
    # algorithm.rnn_critic: a second cell `critic_memory` reads the critic's row and the critic its state; loaded with the rest, never exported
    if "critic_memory.weight_ih" in sd:
        est_args["critic_memory_hidden"] = int(sd["critic_memory.weight_hh"].shape[1])
        num_priv = int(sd["critic_memory.weight_ih"].shape[1]) - num_obs
    if num_obs % 47:
        # terrain.actor_heights: the actor's row ends with the height scan, whose grid the checkpoint carries
        pts = ckpt.get("height_points")
        P = int(pts.shape[0]) if pts is not None else 0
        if P == 0 or (num_obs - P) % 47 or num_obs <= P:
            raise ValueError(f"the checkpoint's actor takes {num_obs} inputs: neither 47 x env.frame_stack nor that plus the points of its "
                             f"\"height_points\" entry ({P}; terrain.actor_heights)")
        xs, ys = sorted(set(pts[:, 0].tolist())), sorted(set(pts[:, 1].tolist()))
        print("Actor input of {} columns: 47 x {} observations, then {} heights, grid x {:.3g} .. {:.3g} ({}) by y {:.3g} .. {:.3g} ({}), point p = i * {} + j "
              "at (x_i, y_j) in the robot's yaw frame".format(num_obs, (num_obs - P) // 47, P, xs[0], xs[-1], len(xs), ys[0], ys[-1], len(ys), len(ys)))
    model = ActorCritic(cfg["env"]["num_actions"], num_obs, num_priv, actor_hidden=hidden_of(sd, "actor"),
                        critic_hidden=hidden_of(sd, "critic"), **est_args)
    # rnd.enabled: the checkpoint's curiosity networks ("rnd_predictor.*", "rnd_target.*") belong to training and are not built here
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("rnd_predictor.", "rnd_target."))})
    if ckpt.get("obs_normalizer") is not None:
        # algorithm.empirical_normalization: the statistics go into the first Linear layer (W' = W diag(inv_std), b' = b - W' mean), so the exported
        # module still takes the raw observation deploy/utils/policy.py builds
        from booster_gym_amd.utils.obs_norm import ObsNormalizer

        st = ckpt["obs_normalizer"]
        norm = ObsNormalizer(int(st["mean"].numel()), float(st["eps"]))
        norm.load_state_dict(st)
        w, b = norm.fold_into_first_layer(model.actor[0].weight, model.actor[0].bias)
        with torch.no_grad():
            model.actor[0].weight.copy_(w)
            model.actor[0].bias.copy_(b)
        print("Folded the observation normaliser ({} columns, count {:.0f}) into the actor's first layer".format(norm.cols, norm.count))
    os.makedirs("deploy/models", exist_ok=True)
    out = os.path.join("deploy", "models", f"{args.task}.pt")
    if model.memory_hidden:
        module = RecurrentActor(model.memory, model.actor)
        print("Recurrent actor (GRU cell of width {}): the exported module is STATEFUL.  forward(obs [B][{}]) -> actions [B][12] advances its hidden state by "
              "one step: call it once per control step, on the newest observation only.  The state is a buffer of the module, zero at first and "
              "re-created zero whenever B changes; call reset() where an episode starts.".format(model.memory_hidden, num_obs))
    else:
        module = EstimatorActor(model.actor, model.estimator, model.estimator_cols) if model.has_estimator else model.actor
    torch.jit.script(module).save(out)
    print("Exported actor to {}".format(out))
