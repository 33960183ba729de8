"""Cross-simulator player (TEST-INFRASTRUCTURE TOOL, uses oracle/): headless equivalent of the reference's play_mujoco.py:717-764 step loop,
driving the float64 CPU oracle simulator with a trained actor, `x y yaw` commands and the gait-frequency rule of play_mujoco.py:692-714.

    python tools/play_oracle.py <checkpoint.pth | actor.npz> [--cmd 0.5 0 0] [--seconds 8]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_actor(path, memory=False):
    """The actor's layers.  memory: the caller runs the cell of a recurrent actor in front of them (load_memory); without it a checkpoint that
    carries memory.* is a ValueError, because its layers are the trunk behind the cell and read the cell's state, not the observation."""
    if path.endswith(".npz"):
        W = np.load(path)
        return [(W[f"{i}.weight"], W[f"{i}.bias"]) for i in (0, 2, 4, 6)]
    import torch

    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck["model"]
    if "memory.weight_ih" in sd and not memory:
        raise ValueError(f"{path} is a recurrent student or actor (distillation.student_memory, algorithm.rnn_hidden_size: it carries memory.*): its "
                         "layers read the cell's state; load them with load_actor(path, memory=True) and the cell with load_memory(path)")
    layers = [(sd[f"actor.{i}.weight"].numpy(), sd[f"actor.{i}.bias"].numpy()) for i in (0, 2, 4, 6)]
    if ck.get("obs_normalizer") is not None:
        # algorithm.empirical_normalization: the actor was trained on (x - mean) / (sqrt(var) + eps); the first layer takes the statistics in, so the
        # loop below feeds raw observations as the deployed policy does (export_model.py folds the same way)
        layers[0] = tuple(t.numpy() for t in normalizer_of(ck).fold_into_first_layer(*layers[0]))
    return layers


def load_estimator(path):
    """(layers, E) of the state estimator a checkpoint carries (estimator.enabled: "estimator.*" in its model, the targets under "estimator"), or
    None: the actor's row is then [observations | the first E outputs of the estimator on the observations]."""
    if path.endswith(".npz"):
        return None
    import torch

    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck["model"]
    idx = sorted(int(k.split(".")[1]) for k in sd if k.startswith("estimator.") and k.endswith(".weight"))
    if not idx:
        return None
    return [(sd[f"estimator.{i}.weight"].numpy(), sd[f"estimator.{i}.bias"].numpy()) for i in idx], len(ck["estimator"]["targets"])


def load_memory(path):
    """The GRU cell in front of a recurrent actor (algorithm.rnn_hidden_size, or a student of distillation.student_memory: "memory.*" in the
    checkpoint's model) as a GRUMemory, or None: the actor then reads the cell's state instead of the observation."""
    if path.endswith(".npz"):
        return None
    import torch

    sd = torch.load(path, map_location="cpu", weights_only=True)["model"]
    if "memory.weight_ih" not in sd:
        return None
    return GRUMemory(*[sd[f"memory.{k}"].numpy() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])


class GRUMemory:
    """The deploy side of a recurrent actor: torch.nn.GRUCell's equations (gate order r | z | n) in float64 on one row, the state zero at the start
    and after reset()."""

    def __init__(self, weight_ih, weight_hh, bias_ih, bias_hh):
        self.w_ih, self.w_hh, self.b_ih, self.b_hh = (np.asarray(t, dtype=np.float64) for t in (weight_ih, weight_hh, bias_ih, bias_hh))
        self.hidden = int(self.w_hh.shape[1])
        self.reset()

    def reset(self):
        self.h = np.zeros(self.hidden)

    def step(self, x):
        """One step on the newest single observation x; returns the new state [hidden] (kept: the next step starts from it)."""
        H, sig = self.hidden, lambda v: 1.0 / (1.0 + np.exp(-v))
        gi, gh = self.w_ih @ np.asarray(x, dtype=np.float64) + self.b_ih, self.w_hh @ self.h + self.b_hh
        r, z = sig(gi[:H] + gh[:H]), sig(gi[H : 2 * H] + gh[H : 2 * H])
        n = np.tanh(gi[2 * H :] + r * gh[2 * H :])
        self.h = (1.0 - z) * n + z * self.h
        return self.h


def mlp(layers, x):
    """An ELU MLP with a linear output layer on one row."""
    for k, (w, b) in enumerate(layers):
        x = w @ x + b
        if k + 1 < len(layers):
            x = np.where(x > 0, x, np.exp(np.minimum(x, 0)) - 1)
    return x


def normalizer_of(ck):
    """The ObsNormalizer (host only) a checkpoint carries under "obs_normalizer"."""
    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    st = ck["obs_normalizer"]
    norm = ObsNormalizer(int(st["mean"].numel()), float(st["eps"]))
    norm.load_state_dict(st)
    return norm


class FrameStack:
    """The deploy side of env.frame_stack (humanoid-gym's sim2sim deque): the last H single observations side by side, oldest first, newest last,
    all zeros before the first push and after reset()."""

    def __init__(self, frames, width=47):
        self.frames, self.width = int(frames), int(width)
        self.reset()

    def reset(self):
        self.row = np.zeros(self.frames * self.width)

    def push(self, obs):
        """Append the newest single observation, drop the oldest; returns the stacked row [frames * width] (a view: copy it to keep it)."""
        self.row = np.concatenate([self.row[self.width :], np.asarray(obs, dtype=np.float64).reshape(self.width)])
        return self.row


def load_height_points(path):
    """[P][2] grid of the actor's height scan (terrain.actor_heights: the checkpoint's "height_points"), or None."""
    if path.endswith(".npz"):
        W = np.load(path)
        return W["height_points"] if "height_points" in W.files else None
    import torch

    pts = torch.load(path, map_location="cpu", weights_only=True).get("height_points")
    return None if pts is None else pts.numpy()


def actor_frames(layers, width=47, scan=0):
    """Frames H of an actor whose first layer takes H * width inputs and then `scan` height-scan values (ValueError otherwise)."""
    k = int(layers[0][0].shape[1]) - int(scan)
    if k < width or k % width:
        raise ValueError(f"the actor takes {k + int(scan)} inputs, not a multiple of the {width} single observations (env.frame_stack)"
                         + (f" plus the {scan} points of the height scan (terrain.actor_heights)" if scan else ""))
    return k // width


def height_scan(root, height_points, cfg, terrain_height=None):
    """The noiseless actor scan the env computes (terrain.actor_heights): clip(base z - h_p - base_height_target, -1, 1) * S at the grid points turned
    by the base yaw.  terrain_height(x, y) -> h; None = the oracle's plane, h = 0."""
    pts = np.asarray(height_points, dtype=np.float64).reshape(-1, 2)
    x, y, z, w = root[3:7]
    yaw = np.arctan2(2.0 * (w * z + x * y), w * w + x * x - y * y - z * z)
    c, s = np.cos(yaw), np.sin(yaw)
    wx, wy = root[0] + c * pts[:, 0] - s * pts[:, 1], root[1] + s * pts[:, 0] + c * pts[:, 1]
    h = np.zeros(len(pts)) if terrain_height is None else np.array([terrain_height(a, b) for a, b in zip(wx, wy)])
    return np.clip(root[2] - h - cfg["rewards"]["base_height_target"], -1.0, 1.0) * cfg["normalization"].get("height_measurements", 5.0)


def gait_frequency(cmd, cfg_commands, max_lin=1.0, max_ang=1.0):
    """play_mujoco.py:692-714: stand still below 0.1 of command magnitude, else scale the frequency with the command."""
    mag = float(np.sqrt(np.sum(np.square(cmd))))
    if mag < 0.1:
        return 0.0
    lo, hi = min(cfg_commands["gait_frequency"]), max(cfg_commands["gait_frequency"])
    return lo + min(1.0, mag / max(max_lin, max_ang)) * (hi - lo)


def rollout(layers, cmd, seconds, cfg=None, dyn=None, model=None, height_points=None, estimator=None, memory=None):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.urdf import load_model
    from oracle import task_ref as tr
    from oracle.dyn_ref import DynRef

    cfg = cfg or load_cfg("T1")
    if (cfg.get("sensors") or {}).get("enabled"):
        print("play_oracle: sensors.enabled is not modelled here: the oracle feeds the policy the true, undelayed observation (noise, bias and latency are the env's)")
    model = model or load_model(cfg["asset"]["file"])
    dyn = dyn or DynRef(model, feet_edge_pos=cfg["asset"]["feet_edge_pos"])
    nz = cfg["normalization"]
    default = np.array([cfg["init_state"]["default_joint_angles"].get(k, 0.0) for k in ["Hip_Pitch", "default", "default", "Knee_Pitch", "Ankle_Pitch", "default"]] * 2)
    kp = np.array([200.0, 200, 200, 200, 50, 50] * 2); kd = np.array([5.0, 5, 5, 5, 1, 1] * 2)
    ctrl = np.array([45.0, 45, 30, 65, 24, 15] * 2)  # MJCF ctrlrange (T1_locomotion.xml:123-134), what play_mujoco.py:751-755 clips to
    root = np.zeros(13); root[:3] = cfg["init_state"]["pos"]; root[6] = 1.0
    q, qd = default.copy(), np.zeros(12)
    cmd = np.asarray(cmd, dtype=np.float64)
    gf, gp = gait_frequency(cmd, cfg["commands"]), 0.0
    actions, targets = np.zeros(12), default.copy()
    dec, dt = cfg["control"]["decimation"], cfg["sim"]["dt"]
    P = 0 if height_points is None else len(height_points)  # terrain.actor_heights: the row ends with the newest scan, not stacked
    est_layers, E = estimator if estimator is not None else (None, 0)  # estimator.enabled: E estimates behind the observations
    # a recurrent actor (memory: a GRUMemory): the cell reads the newest single observation and the trunk its state, zero at the start
    stack = FrameStack(1 if memory is not None else actor_frames(layers, scan=P + E))  # (H = 1: the single observation itself)
    if memory is not None:
        memory.reset()
    traj = []
    for it in range(int(round(seconds / dt))):
        if it % dec == 0:  # play_mujoco.py:733-748
            o = np.zeros(47)
            o[0:3] = tr.quat_rotate_inverse(root[3:7], np.array([0.0, 0.0, -1.0])) * nz["gravity"]
            o[3:6] = tr.quat_rotate_inverse(root[3:7], root[10:13]) * nz["ang_vel"]
            o[6], o[7], o[8] = cmd[0] * nz["lin_vel"], cmd[1] * nz["lin_vel"], cmd[2] * nz["ang_vel"]
            o[9], o[10] = np.cos(2 * np.pi * gp) * (gf > 1e-8), np.sin(2 * np.pi * gp) * (gf > 1e-8)
            o[11:23], o[23:35], o[35:47] = (q - default) * nz["dof_pos"], qd * nz["dof_vel"], actions
            x = stack.push(o)
            if P:
                x = np.concatenate([x, height_scan(root, height_points, cfg)])
            if E:
                x = np.concatenate([x, mlp(est_layers, x)[:E]])
            if memory is not None:
                x = memory.step(x)
            for k, (w, b) in enumerate(layers):
                x = w @ x + b
                if k < 3:
                    x = np.where(x > 0, x, np.exp(np.minimum(x, 0)) - 1)
            actions = np.clip(x, -nz["clip_actions"], nz["clip_actions"])
            targets = default + cfg["control"]["action_scale"] * actions
        dyn.step(root, q, qd, np.clip(kp * (targets - q) - kd * qd, -ctrl, ctrl))  # play_mujoco.py:751-756
        gp = np.fmod(gp + dt * gf, 1.0)
        traj.append(root.copy())
    return np.array(traj)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("policy")
    ap.add_argument("--cmd", type=float, nargs=3, default=[0.5, 0.0, 0.0])
    ap.add_argument("--seconds", type=float, default=8.0)
    a = ap.parse_args()
    tr_ = rollout(load_actor(a.policy, memory=True), a.cmd, a.seconds, height_points=load_height_points(a.policy), estimator=load_estimator(a.policy),
                  memory=load_memory(a.policy))
    up = 1 - 2 * (tr_[-1, 3] ** 2 + tr_[-1, 4] ** 2)
    print(f"cmd {a.cmd}: final pos {np.round(tr_[-1, :3], 3)}, mean velocity {np.round((tr_[-1, :2] - tr_[0, :2]) / a.seconds, 3)}, min height {tr_[:, 2].min():.3f}, upright {up:.3f}")
