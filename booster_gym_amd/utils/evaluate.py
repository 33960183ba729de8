"""How well does a checkpoint walk?  Per-robot metrics of every robot's FIRST episode, for every checkpoint kind this build produces.

    python evaluate.py --task=T1 --checkpoint=PATH [--num_envs N] [--seed S] [--steps K] [--out FILE] [--gait] [--record_out FILE.npz]

The policy's MEAN action drives N robots under the config as shipped (observation noise, domain randomisation, kicks and pushes stay on: that is the
protocol) until every first episode has ended.  Per env step the loop enqueues, without a host synchronisation: bg_obs_normalize when the checkpoint
has a normaliser, the rollout's own actor launch (ActorCritic.sample_actions; its mean is the action, its sample goes to a scratch tensor), the env
step, and ONE launch that keeps the per-robot record [23][N] (bg_env_eval_step; the rule is stated at the kernel in csrc/bg_sim.hip and in the README).
`evaluation_report` reduces the record on the host, once, in float64: for all robots, per terrain level and per terrain column.

The `evaluation:` section of a config (optional; read by this module alone): settle_s = the seconds at the start of an episode that give no
tracking sample (settle_steps = ceil(settle_s / dt)); spread_terrain_levels = with terrain.curriculum, robot i starts on level i mod num_levels, so
that every level gets the same number of robots (false: the checkpoint's levels stay); gait = keep the second per-robot record as well (default
false; `--gait`): one more launch per step (bg_env_gait_step, [60][N]: action rate, effort, wobble, duty factor, touchdowns, slip, swing clearance;
the rule is stated at that kernel and in the README), reduced by `gait_report` into the key "gait" of every group.  `--record_out FILE.npz` saves
the per-robot records themselves, so that two evaluations under one seed can be paired robot by robot.
"""
import argparse
import json
import math

import numpy as np

from .. import _lib

DEFAULTS = {"settle_s": 1.0, "spread_terrain_levels": True}
OPTIONAL = {"gait": False}  # accepted, not in the shipped mapping (and not in the key list of the two messages below, which stay as they were)
FELL_WITHIN_S = (2, 6, 10, 20)


def evaluation_cfg(cfg):
    """(settle_s, spread_terrain_levels) of a config's optional `evaluation` section (absent keys: DEFAULTS), or ValueError naming the key.  Pure."""
    sec = cfg.get("evaluation")
    if sec is None:
        sec = {}
    if not isinstance(sec, dict):
        raise ValueError(f"evaluation must be a mapping of its keys ({', '.join(DEFAULTS)}), got {sec!r}")
    unknown = sorted(set(sec) - set(DEFAULTS) - set(OPTIONAL))
    if unknown:
        raise ValueError(f"evaluation.{unknown[0]} is not a key of the section ({', '.join(DEFAULTS)})")
    v = {**DEFAULTS, **OPTIONAL, **sec}
    s = v["settle_s"]
    if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s < 0:
        raise ValueError(f"evaluation.settle_s must be a finite number >= 0, got {s!r}")
    if not isinstance(v["spread_terrain_levels"], bool):
        raise ValueError(f"evaluation.spread_terrain_levels must be true or false, got {v['spread_terrain_levels']!r}")
    if not isinstance(v["gait"], bool):
        raise ValueError(f"evaluation.gait must be true or false, got {v['gait']!r}")
    return float(s), v["spread_terrain_levels"]


def gait_of(cfg):
    """evaluation.gait of a config (absent: false), after every check of evaluation_cfg.  Pure."""
    evaluation_cfg(cfg)
    return bool((cfg.get("evaluation") or {}).get("gait", OPTIONAL["gait"]))


def settle_steps_of(settle_s, dt):
    return int(math.ceil(settle_s / dt - 1e-9))  # (1.0 / 0.02 is 50, not 51, whatever the division rounds to)


def _div(a, b):
    return float(a) / float(b) if b else None


def _group(rec, sel, dt):
    """The report of the robots `sel` (boolean [N]) of a float64 record."""
    L = _lib
    state, length = rec[L.EVAL_STATE][sel], rec[L.EVAL_LEN][sel]
    robots = int(sel.sum())
    fell_m = state == L.EVAL_FELL
    fell, timed_out, unfinished = int(fell_m.sum()), int((state == L.EVAL_TIMED_OUT).sum()), int((state == L.EVAL_RUNNING).sum())
    dist = np.hypot(rec[L.EVAL_X1][sel] - rec[L.EVAL_X0][sel], rec[L.EVAL_Y1][sel] - rec[L.EVAL_Y0][sel])
    cls = rec[L.EVAL_CLASS][sel]
    cnt = [rec[L.eval_track_plane(c, 0)][sel].sum() for c in range(L.EVAL_CLASSES)]
    out = {
        "robots": robots, "fell": fell, "timed_out": timed_out, "unfinished": unfinished,
        "fall_rate": _div(fell, fell + timed_out),
        "fell_within_s": {str(s): _div(int((fell_m & (length * dt <= s + 1e-9)).sum()), robots) for s in FELL_WITHIN_S},
        "mean_episode_length": _div(length.sum(), robots),
        "mean_reward_per_step": _div(rec[L.EVAL_REW][sel].sum(), length.sum()),
        "mean_distance_m": _div(dist.sum(), robots),
        # (the step that ended the episode gave no sample: LEN - 1 steps of a finished robot added to POWER)
        "mean_abs_joint_power_w": _div(rec[L.EVAL_POWER][sel].sum(), (length - (state != L.EVAL_RUNNING)).sum()),
        "tracking_rmse": {name: {ax: (math.sqrt(rec[L.eval_track_plane(c, 1 + a)][sel].sum() / cnt[c]) if cnt[c] else None)
                                 for a, ax in enumerate(L.EVAL_AXES)} for c, name in enumerate(L.EVAL_CLASS_NAMES)},
        "tracked_steps": {name: int(cnt[c]) for c, name in enumerate(L.EVAL_CLASS_NAMES)},
        "falls_by_class": {name: int((fell_m & (cls == c)).sum()) for c, name in enumerate(L.EVAL_CLASS_NAMES)},
    }
    return out


def evaluation_report(record, dt, num_levels, num_types):
    """The record [EVAL_PLANES][N] of bg_env_eval_step as a dict: "all", "by_level"[l], "by_type"[t], each with robots / fell / timed_out /
    unfinished, fall_rate = fell / (fell + timed_out), fell_within_s (the fraction of the group's robots that fell within 2, 6, 10, 20 s),
    mean_episode_length (steps), mean_reward_per_step, mean_distance_m (start to last position of the first episode, straight line),
    mean_abs_joint_power_w, tracking_rmse[class][axis] = sqrt(sum SQ / sum CNT), tracked_steps[class], falls_by_class (the class of the last
    command a fallen robot had).  A quotient without a denominator (an empty group, a class never tracked) is None.  numpy, float64, no device."""
    rec = np.asarray(record, dtype=np.float64)
    if rec.ndim != 2 or rec.shape[0] != _lib.EVAL_PLANES:
        raise ValueError(f"evaluation_report needs a record of shape [{_lib.EVAL_PLANES}][N], got {rec.shape}")
    n = rec.shape[1]
    level, typ = rec[_lib.EVAL_LEVEL].astype(np.int64), rec[_lib.EVAL_TYPE].astype(np.int64)
    return {"all": _group(rec, np.ones(n, dtype=bool), dt),
            "by_level": [_group(rec, level == l, dt) for l in range(int(num_levels))],
            "by_type": [_group(rec, typ == t, dt) for t in range(int(num_types))]}


def _gait_group(g, rec, sel, dt, mg):
    """The gait entries of the robots `sel` of the float64 gait record g and first record rec; mg[N] = mass * |gravity|."""
    L = _lib
    P = lambda p: g[p][sel]
    F = lambda k: [g[L.gait_foot_plane(k, f)][sel] for f in range(2)]
    live = P(L.GAIT_LEN) - (P(L.GAIT_STATE) != 0)  # L': the step that ended the episode gave no sample
    mov = P(L.GAIT_MOV).sum()
    stance, td, imp, peak, slip, clr, swt, swc = (F(k) for k in range(8))
    per_foot = lambda num, den: [_div(num[f].sum(), den[f].sum() if isinstance(den, list) else den) for f in range(2)]

    def asymmetry(a, b, who):
        den = np.abs(a) + np.abs(b)  # (a clearance can be negative on a height field: the quotient stays in [0, 1])
        who = who & (den > 0)
        return _div((np.abs(a[who] - b[who]) / den[who]).sum(), int(who.sum()))

    both = (swc[0] > 0) & (swc[1] > 0)
    one = np.ones_like(swc[0])
    mean_clr = [np.where(both, clr[f], 0.0) / np.where(both, swc[f], one) for f in range(2)]
    dist = np.hypot(rec[L.EVAL_X1][sel] - rec[L.EVAL_X0][sel], rec[L.EVAL_Y1][sel] - rec[L.EVAL_Y0][sel])
    robots = int(sel.sum())
    return {
        "moving_steps": int(mov),
        "mean_action_rate": _div(P(L.GAIT_D1).sum(), np.maximum(live - 1, 0).sum()),
        "mean_action_accel": _div(P(L.GAIT_D2).sum(), np.maximum(live - 2, 0).sum()),
        "mean_torque_sq": _div(P(L.GAIT_TAU2).sum(), live.sum()),
        "mean_tilt_sq": _div(P(L.GAIT_TILT).sum(), live.sum()),
        "mean_ang_vel_xy_sq": _div(P(L.GAIT_WOBBLE).sum(), live.sum()),
        "duty_factor": per_foot(stance, mov),
        "double_support": _div(P(L.GAIT_DS).sum(), mov),
        "flight": _div(P(L.GAIT_FL).sum(), mov),
        "step_frequency_hz": per_foot(td, mov * dt),
        "stance_asymmetry": asymmetry(stance[0], stance[1], np.ones(robots, dtype=bool)),
        "swing_asymmetry": asymmetry(mean_clr[0], mean_clr[1], both),
        "foot_slip_m_per_s": _div((slip[0] + slip[1]).sum(), mov * dt),
        "touchdown_force_n": per_foot(imp, td),
        "peak_force_bw": [_div((peak[f] / mg[sel]).sum(), robots) for f in range(2)],
        "swing_clearance_m": per_foot(clr, swc),
        "swing_time_s": [_div(dt * swt[f].sum(), swc[f].sum()) for f in range(2)],
        "cost_of_transport": _div(dt * rec[L.EVAL_POWER][sel].sum(), (mg[sel] * dist).sum()),
    }


def gait_report(gait_record, record, dt, mass, gravity, num_levels, num_types):
    """The gait record [GAIT_PLANES][N] of bg_env_gait_step, beside the first record [EVAL_PLANES][N] of the same run, as a dict with
    evaluation_report's groups: "all", "by_level"[l], "by_type"[t] (level and column are the first record's).  mass[N]: each robot's total mass, kg;
    gravity: its magnitude (or the vector).  With L' = LEN - (STATE != 0) a robot's live steps, sums over the group's robots, feet as [left, right]:
      mean_action_rate = sum D1 / sum max(L' - 1, 0), mean_action_accel = sum D2 / sum max(L' - 2, 0); mean_torque_sq, mean_tilt_sq,
      mean_ang_vel_xy_sq = sum TAU2, TILT, WOBBLE / sum L'; moving_steps = sum MOV; duty_factor[f] = sum STANCE_f / sum MOV; double_support, flight =
      sum DS, FL / sum MOV; step_frequency_hz[f] = sum TD_f / (sum MOV dt); stance_asymmetry = the mean over robots with STANCE_0 + STANCE_1 > 0 of
      |STANCE_0 - STANCE_1| / (STANCE_0 + STANCE_1); swing_asymmetry = the mean of |m_0 - m_1| / (|m_0| + |m_1|), m_f = CLR_f / SWC_f, over robots with
      both SWC_f > 0 and |m_0| + |m_1| > 0 (the same quotient where both clearances are positive; in [0, 1] where a foot's z lay below the ground); foot_slip_m_per_s = sum (SLIP_0 + SLIP_1) / (sum MOV dt); touchdown_force_n[f] = sum IMP_f / sum TD_f; peak_force_bw[f] = the mean over
      robots of PEAK_f / (mass g); swing_clearance_m[f] = sum CLR_f / sum SWC_f; swing_time_s[f] = dt sum SWT_f / sum SWC_f; cost_of_transport =
      dt sum POWER / sum (mass g distance), POWER and the start-to-end distance from the first record.
    A quotient without a denominator is None.  numpy, float64, no device."""
    g, rec = np.asarray(gait_record, dtype=np.float64), np.asarray(record, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] != _lib.GAIT_PLANES:
        raise ValueError(f"gait_report needs a gait record of shape [{_lib.GAIT_PLANES}][N], got {g.shape}")
    if rec.ndim != 2 or rec.shape != (_lib.EVAL_PLANES, g.shape[1]):
        raise ValueError(f"gait_report needs the first record of the same robots, [{_lib.EVAL_PLANES}][{g.shape[1]}], got {rec.shape}")
    n = g.shape[1]
    mass = np.asarray(mass, dtype=np.float64)
    if mass.shape != (n,) or not np.all(mass > 0):
        raise ValueError(f"gait_report needs mass as {n} positive numbers, got shape {mass.shape}")
    mg = mass * float(np.linalg.norm(np.asarray(gravity, dtype=np.float64)))
    level, typ = rec[_lib.EVAL_LEVEL].astype(np.int64), rec[_lib.EVAL_TYPE].astype(np.int64)
    return {"all": _gait_group(g, rec, np.ones(n, dtype=bool), dt, mg),
            "by_level": [_gait_group(g, rec, level == l, dt, mg) for l in range(int(num_levels))],
            "by_type": [_gait_group(g, rec, typ == t, dt, mg) for t in range(int(num_types))]}


def _set_dotted(cfg, dotted, value):
    node, keys = cfg, dotted.split(".")
    for k in keys[:-1]:
        node = node.setdefault(k, {})
    node[keys[-1]] = value


class Evaluator:
    """Runner(test=True) on the checkpoint (every check of Runner._load applies: widths, frame stack, scan, normaliser) plus the evaluation loop.
    checkpoint: a path; a student's (it has a "distillation" entry) first turns the config into the student's by distill.student_overrides, so it
    evaluates under the teacher's yaml.  actor: instead of a checkpoint, the state dict of an actor alone ("0.weight", "0.bias", "2.weight", ...:
    the reference's shipped weights), loaded into the config's actor.  One Evaluator = one run: the env's random streams go on with its step count."""

    def __init__(self, checkpoint=None, actor=None, task="T1", overrides=None, cfg=None):
        import torch

        from .config import load_cfg
        from .distill import checkpoint_student_overrides
        from .runner import Runner, checkpoint_memory_overrides

        if (checkpoint is None) == (actor is None):
            raise ValueError("Evaluator needs a checkpoint path or an actor state dict, one of the two")
        if cfg is None:
            cfg = load_cfg(task, overrides)
        self.settle_s, self.spread = evaluation_cfg(cfg)  # (ValueError before anything is built)
        self.gait = gait_of(cfg)
        self.applied = {}
        if checkpoint is not None:
            loaded = torch.load(checkpoint, map_location="cpu", weights_only=True)
            # a student's re-entry overrides, or the memory width of an actor trained under algorithm.rnn_hidden_size (a rule of its own)
            over = checkpoint_student_overrides(loaded) or checkpoint_memory_overrides(loaded)
            for k, v in (over or {}).items():
                _set_dotted(cfg, k, v)
                self.applied[k] = v
        cfg["basic"]["checkpoint"] = checkpoint
        self.checkpoint = checkpoint
        self.runner = r = Runner(test=True, cfg=cfg)
        self.cfg, self.env, self.model, self.obs_norm = cfg, r.env, r.model, r.obs_norm
        if actor is not None:
            if self.obs_norm is not None:
                raise ValueError("algorithm.empirical_normalization: true needs a checkpoint with its \"obs_normalizer\": an actor state dict has none")
            with torch.no_grad():
                r.model.actor.load_state_dict({k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in actor.items()})
            r.invalidate()
        env = self.env
        if env.terrain.curriculum and self.spread:
            env.terrain_levels = torch.arange(env.num_envs) % env.terrain.num_levels
            self.applied["env.terrain_levels"] = "arange(num_envs) % num_levels (evaluation.spread_terrain_levels)"
        self.settle_steps = settle_steps_of(self.settle_s, env.dt)
        self.max_episode_length = int(env._cfg_c.max_episode_length)
        N, A = env.num_envs, env.num_actions
        self._mu = torch.zeros(N, A, device=env.device)       # the action: the mean of the rollout's own launch
        self._sampled = torch.zeros(N, A, device=env.device)  # ... whose sample is not used
        self._obs_normed = torch.zeros(N, env.num_obs, device=env.device) if self.obs_norm is not None else None
        # estimator.enabled: the launch writes the estimator's 12 means somewhere; nobody here reads them
        self._est_scratch = torch.zeros(N, _lib.NUM_DOFS, device=env.device) if r.model.has_estimator else None
        self.record, self.gait_record, self.steps, self.loop_s, self._mass = None, None, 0, None, None

    def mass(self):
        """Every robot's total mass [N], float64, host: the model's link masses times the env's stored mass_scale.  Computed once."""
        if self._mass is None:
            self._mass = self.env.get_field("mass_scale").cpu().numpy().astype(np.float64) @ np.asarray(self.env.model.mass, dtype=np.float64)
        return self._mass

    def run(self, steps=None):
        """reset, eval_begin, K times (normalise, actor launch, env step, eval_step), nothing of it waiting for the host; then the report.
        evaluation.gait: gait_begin after eval_begin and one gait_step after every eval_step, the gait record in self.gait_record and gait_report's
        entries under "gait" of every group; without the key neither is called.
        K defaults to max_episode_length + 2: every first episode ends.  Leaves the record (device tensor) in self.record and the loop's time
        between two events around it in self.loop_s."""
        import torch

        env, model, norm = self.env, self.model, self.obs_norm
        K = int(steps) if steps is not None else self.max_episode_length + 2
        if K < 1:
            raise ValueError(f"steps must be at least 1, got {K}")
        seed = int(self.cfg["basic"]["seed"]) + 1000003  # (the sample is unused; the launch wants a seed)
        scan = getattr(env, "num_scan_obs", 0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            obs, _ = env.reset()
            model.reset_memory()  # (a recurrent student's hidden state; nothing for every other model)
            done = None
            record = env.eval_begin()
            gait_record = env.gait_begin() if self.gait else None
            packed = model.pack_actor()  # once: no parameter changes during the loop
            t0.record()
            for k in range(K):
                x = obs if norm is None else norm.normalize_into(obs, self._obs_normed)
                if model.memory_hidden:  # the env's done flags of the step just taken: the rows whose memory restarts
                    model.sample_actions(x, self._sampled, seed, k, mu_out=self._mu, reset=done)
                    obs, _, done, _ = env.step(self._mu)
                else:
                    model.sample_actions(x, self._sampled, seed, k, mu_out=self._mu, scan=scan, packed=packed, est_out=self._est_scratch)
                    obs = env.step(self._mu)[0]
                env.eval_step(record, self.settle_steps)
                if gait_record is not None:
                    env.gait_step(gait_record, self.settle_steps)
            t1.record()
        torch.cuda.synchronize()
        self.record, self.gait_record, self.steps, self.loop_s = record, gait_record, K, t0.elapsed_time(t1) * 1e-3
        terrain = env.terrain
        levels, types = (terrain.num_levels, int(self.cfg["terrain"]["num_terrains"])) if terrain.curriculum else (1, 1)
        host_record = record.cpu().numpy()
        rep = evaluation_report(host_record, env.dt, levels, types)
        if gait_record is not None:
            gr = gait_report(gait_record.cpu().numpy(), host_record, env.dt, self.mass(), self.cfg["sim"]["gravity"], levels, types)
            rep["all"]["gait"] = gr["all"]
            for key in ("by_level", "by_type"):
                for grp, gg in zip(rep[key], gr[key]):
                    grp["gait"] = gg
        rep.update({"checkpoint": self.checkpoint, "seed": int(self.cfg["basic"]["seed"]), "num_envs": env.num_envs, "steps": K,
                    "settle_s": self.settle_s, "overrides": dict(self.applied),
                    "nonfinite_resets": float(env.episode_stats(reset=False)[-1].item())})
        return rep

    def save_records(self, path):
        """The per-robot records of run() as an .npz: record [23][N] with record_planes, gait_record [60][N] with gait_planes (evaluation.gait only),
        dt, settle_steps, seed, mass [N].  Two files of equal seed and num_envs pair robot by robot."""
        if self.record is None:
            raise ValueError("save_records needs run() first")
        out = {"record": self.record.cpu().numpy(), "record_planes": np.array(_lib.eval_plane_names()), "dt": np.float64(self.env.dt),
               "settle_steps": np.int64(self.settle_steps), "seed": np.int64(self.cfg["basic"]["seed"]), "mass": self.mass()}
        if self.gait_record is not None:
            out.update({"gait_record": self.gait_record.cpu().numpy(), "gait_planes": np.array(_lib.gait_plane_names())})
        with open(path, "wb") as f:
            np.savez(f, **out)


def format_report(rep):
    """The short table evaluate.py prints: one line per group."""
    def f(x, spec):
        return format(x, spec) if x is not None else "-".rjust(len(format(0.0, spec)))

    lines = ["group      robots   fell  t/out  unfin  fall_rate  mean_len  rew/step   dist_m  power_w  rmse slow x/y/yaw     rmse fast x/y/yaw"]
    rows = [("all", rep["all"])] + [(f"level {l}", g) for l, g in enumerate(rep["by_level"])] + [(f"type {t}", g) for t, g in enumerate(rep["by_type"])]
    for name, g in rows:
        rm = g["tracking_rmse"]
        lines.append(f"{name:<10} {g['robots']:6d} {g['fell']:6d} {g['timed_out']:6d} {g['unfinished']:6d} {f(g['fall_rate'], '10.4f')} "
                     f"{f(g['mean_episode_length'], '9.1f')} {f(g['mean_reward_per_step'], '9.4f')} {f(g['mean_distance_m'], '8.2f')} "
                     f"{f(g['mean_abs_joint_power_w'], '8.1f')}  " + "  ".join(
                         "/".join(f(rm[c][ax], '.3f') for ax in _lib.EVAL_AXES) for c in ("slow", "fast")))
    if "gait" in rep["all"]:
        pair = lambda v, spec: "/".join(f(x, spec) for x in v)
        lines += ["", "gait (feet: left/right)",
                  "group      act_rate  act_acc  torque^2  tilt^2  wobble^2         duty  dbl_sup  flight      step_hz  st_asym  sw_asym  slip_m/s"
                  "   touchdown_n      peak_bw    clearance_m    swing_s     CoT"]
        for name, grp in rows:
            g = grp["gait"]
            lines.append(f"{name:<10} {f(g['mean_action_rate'], '8.4f')} {f(g['mean_action_accel'], '8.4f')} {f(g['mean_torque_sq'], '9.1f')} "
                         f"{f(g['mean_tilt_sq'], '7.4f')} {f(g['mean_ang_vel_xy_sq'], '9.4f')}  {pair(g['duty_factor'], '.3f'):>11} "
                         f"{f(g['double_support'], '8.3f')} {f(g['flight'], '7.3f')}  {pair(g['step_frequency_hz'], '.2f'):>11} "
                         f"{f(g['stance_asymmetry'], '8.3f')} {f(g['swing_asymmetry'], '8.3f')} {f(g['foot_slip_m_per_s'], '9.4f')}  "
                         f"{pair(g['touchdown_force_n'], '.0f'):>12} {pair(g['peak_force_bw'], '.2f'):>12} {pair(g['swing_clearance_m'], '.3f'):>14} "
                         f"{pair(g['swing_time_s'], '.3f'):>10} {f(g['cost_of_transport'], '7.3f')}")
    return "\n".join(lines)


def main(argv=None):
    p = argparse.ArgumentParser(description="Per-robot first-episode metrics of a checkpoint (README: evaluation).")
    p.add_argument("--task", required=True, type=str, help="Name of the task: its yaml is the config the checkpoint was trained under.")
    p.add_argument("--checkpoint", required=True, type=str, help="Path of the checkpoint (Runner's or Distiller's).")
    p.add_argument("--num_envs", type=int, help="Number of robots. Overrides config file if provided.")
    p.add_argument("--seed", type=int, help="Random seed. Overrides config file if provided.")
    p.add_argument("--steps", type=int, help="Env steps to run (default: the episode length + 2, so that every first episode ends).")
    p.add_argument("--out", type=str, default="evaluation.json", help="Where the JSON report goes.")
    p.add_argument("--gait", action="store_true", help="Keep the gait record as well (evaluation.gait: true): one more launch per step, a second table.")
    p.add_argument("--record_out", type=str, help="Save the per-robot records (.npz), for pairing two evaluations of one seed robot by robot.")
    a = p.parse_args(argv)
    over = {}
    if a.num_envs is not None:
        over["env.num_envs"] = a.num_envs
    if a.seed is not None:
        over["basic.seed"] = a.seed
    if a.gait:
        over["evaluation.gait"] = True
    ev = Evaluator(checkpoint=a.checkpoint, task=a.task, overrides=over)
    rep = ev.run(a.steps)
    rep["loop_s"], rep["env_steps_per_s"] = ev.loop_s, ev.env.num_envs * ev.steps / ev.loop_s
    print(format_report(rep))
    if rep["all"]["unfinished"] > 0:
        print(f"WARNING: {rep['all']['unfinished']} of {rep['num_envs']} first episodes had not ended after {rep['steps']} steps: their robots count as "
              f"neither fallen nor timed out (--steps {ev.max_episode_length + 2} ends every one)")
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1)
    print("written " + a.out)
    if a.record_out:
        ev.save_records(a.record_out)
        print("written " + a.record_out)
    return rep
