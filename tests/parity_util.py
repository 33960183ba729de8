"""Step-parity bookkeeping shared by the GPU env tests (test infrastructure).

One env step of the fused HIP kernel is compared with the float64 oracle from IDENTICAL inputs.  Two requirements:
  bulk   over the whole test at least 1 - `max_explained_frac` (99 %) of the env-steps are within the stated tolerance on EVERY compared
         field at once (measured: 100 % on flat ground, 99.9 % on the rough terrain, the same fractions as the oracle's own fp32 build
         against its float64 build: profiles/r02_parity_diag_*.json, tools/parity_diag.py);
  hard   every env outside a tolerance must be EXPLAINED, otherwise the test fails.  Accepted explanations, each verified per env:
           contact_flag    a discrete flag of the final state differs (foot-contact flag; fields derived from it: feet_slip, feet_swing)
           limit_crossing  a joint sits within the position tolerance of its limit (dof_pos_limits counts it on one side only)
           fp32_backward   backward-error criterion: the float64 oracle, run from this env's inputs perturbed at fp32-rounding size
                           (relative 2e-6, then 2e-5), produces outcomes whose envelope contains the GPU's post-physics state.  A stiff
                           penalty contact near a switching surface (corner touching down, height-field cell edge, friction regime)
                           turns rounding-level differences into visible ones; a kernel defect is not reproduced by such perturbations.
A tight bound on the number of explained envs keeps the explanations from becoming the rule.
"""
import math
import os

import numpy as np

FIELDS = ["root_states", "dof_pos", "dof_vel", "last_dof_targets", "actions", "last_actions", "last_dof_vel", "last_root_vel", "commands",
          "gait_frequency", "gait_process", "filtered_lin_vel", "filtered_ang_vel", "last_feet_pos", "pushing", "episode_length_buf",
          "cmd_resample_time", "delay_steps"]

# relative to max(1, |reference|) per element, worst element per env
STATE_TOL = {"root": 2e-3, "dof_pos": 2e-3, "dof_vel": 1e-2, "torques": 5e-3, "feet_pos": 2e-3, "obs": 5e-3, "priv": 5e-3}
# scaled reward terms (yaml scale x dt, magnitudes 1e-6 .. 1e-2): relative to max(|reference|, REW_FLOOR)
REW_FLOOR = 5e-5          # 1 % of the survival reward of one step (0.25 x 0.02)
REW_TOL = 2e-2
FLAG_TERMS = ("feet_slip", "feet_swing")          # functions of the foot-contact flags
COUNT_TERMS = ("dof_pos_limits", "collision")     # integer counts of threshold crossings


def gru_sequence_case(T, N, H, gi_scale=1.0, reset=0.2, h0=True, device="cpu"):
    """Inputs of bg_gru_sequence_forward / _backward at one shape, with the float64 restatement of the recurrence and an fp32 torch twin of the same
    loop (what torch's own fp32 arithmetic leaves of it: the yardstick a kernel's error is printed beside).
      gi_scale  multiplies the x-side pre-activations gi (8: a large share of the gates saturates)
      reset     a rate (each flag set with that probability), "step2" (every env at t = 2 and nowhere else), "t0" (the rate-0.2 flags of step 0,
                none later), "none" (an all-zero tensor) or None (no tensor: the launch's reset == NULL)
      h0        False: no tensor (h0 == NULL); the restatement then starts from a zero state
    The draws are made in one fixed order whatever the options, so two cases of one (T, N, H) share gi, h0, the rate-0.2 flags and dh_ext.
    Returns T, N, H, cell (torch.nn.GRUCell(47, H)), gi [T][N][3H], h0 [N][H] or None, reset uint8 [T][N] or None, dh_ext [T][N][H] on `device`, and
    ref / twin: dicts of h_prev, h [T][N][H], gates [T][N][4H] = r | z | n | gh_n, and autograd's dgi, dgh [T][N][3H], dh0 [N][H] of
    sum(h * dh_ext), in float64 / float32."""
    import torch

    g = torch.Generator(device="cpu").manual_seed(40 + H)
    torch.manual_seed(7)
    cell = torch.nn.GRUCell(47, H)
    gi = torch.randn(T, N, 3 * H, generator=g) * gi_scale
    h0_t = torch.randn(N, H, generator=g) * 0.5
    drawn = torch.rand(T, N, generator=g)
    dh_ext = torch.randn(T, N, H, generator=g)
    if reset is None:
        flags = None
    elif reset == "none":
        flags = torch.zeros(T, N, dtype=torch.uint8)
    elif reset == "step2":
        flags = torch.zeros(T, N, dtype=torch.uint8)
        flags[2] = 1
    elif reset == "t0":
        flags = (drawn < 0.2).to(torch.uint8)
        flags[1:] = 0
    else:
        flags = (drawn < float(reset)).to(torch.uint8)
    if not h0:
        h0_t = None

    def loop(dtype):
        W, b = cell.weight_hh.detach().to(dtype), cell.bias_hh.detach().to(dtype)
        gi_, h0_ = gi.to(dtype).requires_grad_(), (torch.zeros(N, H, dtype=dtype) if h0_t is None else h0_t.to(dtype)).requires_grad_()
        h, hp_l, h_l, gates_l, gh_l = h0_, [], [], [], []
        for t in range(T):
            hp = h if flags is None else h * (1 - flags[t].to(dtype)).view(N, 1)
            gh = hp @ W.t() + b
            gh.retain_grad()
            r, z = torch.sigmoid(gi_[t, :, :H] + gh[:, :H]), torch.sigmoid(gi_[t, :, H : 2 * H] + gh[:, H : 2 * H])
            n = torch.tanh(gi_[t, :, 2 * H :] + r * gh[:, 2 * H :])
            h = (1 - z) * n + z * hp
            hp_l.append(hp); h_l.append(h); gh_l.append(gh); gates_l.append(torch.cat((r, z, n, gh[:, 2 * H :]), 1))
        (torch.stack(h_l) * dh_ext.to(dtype)).sum().backward()
        out = dict(h_prev=torch.stack(hp_l).detach(), h=torch.stack(h_l).detach(), gates=torch.stack(gates_l).detach(), dgi=gi_.grad,
                   dgh=torch.stack([x.grad for x in gh_l]), dh0=h0_.grad)
        return {k: v.to(device) for k, v in out.items()}

    ref, twin = loop(torch.float64), loop(torch.float32)
    to = lambda x: None if x is None else x.to(device)
    return dict(T=T, N=N, H=H, cell=cell.to(device), gi=to(gi), h0=to(h0_t), reset=to(flags), dh_ext=to(dh_ext), ref=ref, twin=twin)


def rel_state(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.abs(a - b) / np.maximum(1.0, np.abs(b))).reshape(a.shape[0], -1).max(axis=1)


def rel_reward(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), REW_FLOOR)


def sync_oracle(env, ref):
    g = {k: env.get_field(k).cpu().numpy() for k in FIELDS}
    n = ref.n
    f = lambda k: g[k].astype(np.float64)
    ref.root, ref.q, ref.qd = f("root_states"), f("dof_pos"), f("dof_vel")
    ref.last_tgt, ref.actions, ref.last_actions = f("last_dof_targets"), f("actions"), f("last_actions")
    ref.last_qd, ref.last_rootvel = f("last_dof_vel"), f("last_root_vel")
    ref.cmd, ref.gait_f, ref.gait_p = f("commands"), f("gait_frequency")[:, 0], f("gait_process")[:, 0]
    ref.filt_lin, ref.filt_ang = f("filtered_lin_vel"), f("filtered_ang_vel")
    ref.last_feet, ref.push = f("last_feet_pos").reshape(n, 2, 3), f("pushing")
    ref.ep_len, ref.cmd_time, ref.delay = (g[k][:, 0].astype(np.int64) for k in ("episode_length_buf", "cmd_resample_time", "delay_steps"))
    ref.step_count = env.common_step_counter


class StepParity:
    def __init__(self, cfg, env, ref, max_explained_frac=0.01, state_tol=None, seed=1234):
        self.cfg, self.env, self.ref = cfg, env, ref
        self.max_explained_frac = max_explained_frac
        self.tol = dict(STATE_TOL)
        self.tol.update(state_tol or {})
        self.rng = np.random.default_rng(seed)
        self.log, self.checked, self.explained, self.flag_flips = [], 0, 0, 0

    # ---- before the step: identical inputs on both sides, and a copy of them for the backward-error probe
    def begin(self):
        sync_oracle(self.env, self.ref)
        r = self.ref
        self.pre = {k: getattr(r, k).copy() for k in ("root", "q", "qd", "last_tgt", "push", "delay")}
        self.pre_cmd_time = r.cmd_time.copy()

    # ---- float64 physics of one env from perturbed inputs: envelope of the post-physics state
    def _envelope(self, e, act, delta, P=48):
        r, cfg, pre = self.ref, self.cfg, self.pre
        rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[e:e + 1], P, axis=0).copy()
        root, q, qd, last_tgt = rep(pre["root"]), rep(pre["q"]), rep(pre["qd"]), rep(pre["last_tgt"])
        u = lambda shape: self.rng.uniform(-1.0, 1.0, shape)
        pert = lambda x: x + delta * np.maximum(1.0, np.abs(x)) * u(x.shape)
        root[1:], q[1:], qd[1:] = pert(root[1:]), pert(q[1:]), pert(qd[1:])  # copy 0 = the unperturbed inputs
        root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
        nz = cfg["normalization"]
        a = np.clip(np.asarray(act, dtype=np.float64)[e], -nz["clip_actions"], nz["clip_actions"])
        targets = np.repeat((r.default + cfg["control"]["action_scale"] * a)[None], P, axis=0)
        n = r.n
        com0 = np.array(r.dyn.model.com[0][:]) + r.p["com_off"].reshape(n, 13, 3)[e, 0]
        wrench = pre["push"][e].copy()
        wrench[3:] += np.cross(com0, pre["push"][e, :3])
        r.dyn.substeps_batch(cfg["control"]["decimation"], rep(r.p["mass_scale"]), rep(r.p["com_off"].reshape(n, 39)), rep(r.p["foot_mat"].reshape(n, 6)),
                             rep(r.p["kp"]), rep(r.p["kd"]), rep(r.p["fric"]), r.limits["torque_limits"], root, q, qd, targets, last_tgt,
                             np.repeat(pre["delay"][e:e + 1], P).astype(np.int32), np.repeat(wrench[None], P, axis=0))
        return root, q, qd

    def _inside(self, x, ys, tol):
        lo, hi = ys.min(axis=0), ys.max(axis=0)
        pad = tol * np.maximum(1.0, np.abs(ys[0]))
        return bool(np.all((x >= lo - pad) & (x <= hi + pad)))

    def _explain_physics(self, e, act, kicked):
        """fp32_backward: is the GPU's post-physics state inside the envelope of float64 outcomes for rounding-size input perturbations?"""
        g_root = self.env.root_states[e].cpu().numpy().astype(np.float64)
        g_q = self.env.dof_pos[e].cpu().numpy().astype(np.float64)
        g_qd = self.env.dof_vel[e].cpu().numpy().astype(np.float64)
        for delta in (2e-6, 2e-5):
            root, q, qd = self._envelope(e, act, delta)
            ok = self._inside(g_root[:7], root[:, :7], self.tol["root"]) and self._inside(g_q, q, self.tol["dof_pos"]) and \
                self._inside(g_qd, qd, self.tol["dof_vel"])
            if not kicked:  # a kick adds the same random velocity on both sides after the physics; the envelope has no kick
                ok = ok and self._inside(g_root[7:], root[:, 7:], self.tol["dof_vel"])
            if ok:
                return f"fp32_backward(delta={delta:g})"
        return None

    # ---- after the step
    def check(self, s, act, obs, rew, done, extras, ref_out, kicked=False, teleported=None):
        env, ref, tol = self.env, self.ref, self.tol
        o_ref, p_ref, r_ref, d_ref, t_ref, terms_ref, derived = ref_out
        n = ref.n
        d_gpu = done.cpu().numpy()
        keep = d_gpu == d_ref  # an env whose termination flag flipped (threshold crossing) is reset on one side only: counted by the caller
        if teleported is not None:
            keep = keep & ~teleported
        fc_gpu = env.get_field("feet_contact").cpu().numpy() > 0.5
        fc_ref = np.asarray(derived["feet_contact"]).astype(bool)
        flag_flip = (fc_gpu != fc_ref).any(axis=1)
        err = {"root": rel_state(env.root_states.cpu().numpy(), ref.root), "dof_pos": rel_state(env.dof_pos.cpu().numpy(), ref.q),
               "dof_vel": rel_state(env.dof_vel.cpu().numpy(), ref.qd), "torques": rel_state(env.get_field("torques").cpu().numpy(), derived["torques"]),
               "feet_pos": rel_state(env.get_field("feet_pos").cpu().numpy(), derived["feet_pos"].reshape(n, 6)),
               "obs": rel_state(obs.cpu().numpy(), o_ref), "priv": rel_state(extras["privileged_obs"].cpu().numpy(), p_ref)}
        bad = {k: err[k] > tol[k] for k in err}
        rerr = {"reward": rel_reward(rew.cpu().numpy(), r_ref)}
        for name, v in terms_ref.items():
            rerr[name] = rel_reward(extras["rew_terms"][name].cpu().numpy(), v)
        for k, v in rerr.items():
            bad["rew:" + k] = v > REW_TOL
        any_bad = np.zeros(n, dtype=bool)
        for k, b in bad.items():
            any_bad |= b
        any_bad &= keep
        nk = int(keep.sum())
        lo, hi = ref.limits["dof_pos_limits"][:, 0], ref.limits["dof_pos_limits"][:, 1]
        for e in np.nonzero(any_bad)[0]:
            fields = [k for k, b in bad.items() if b[e]]
            why = []
            state_fields = [k for k in fields if not k.startswith("rew:")]
            rew_fields = [k[4:] for k in fields if k.startswith("rew:")]
            # discrete flags of the final state
            pending = set(rew_fields)
            if flag_flip[e]:
                if pending & (set(FLAG_TERMS) | {"reward"}):
                    why.append("contact_flag")
                pending -= set(FLAG_TERMS) | {"reward"}
            near_limit = bool((np.minimum(np.abs(ref.q[e] - lo), np.abs(ref.q[e] - hi)) < tol["dof_pos"]).any())
            if "dof_pos_limits" in pending and near_limit:
                why.append("limit_crossing")
                pending -= {"dof_pos_limits", "reward"}
            if state_fields or pending:
                w = self._explain_physics(int(e), act, kicked)
                if w is None:
                    worst = {k: float(err[k][e]) for k in state_fields}
                    worst.update({k: float(rerr[k][e]) for k in pending})
                    raise AssertionError(f"step {s} env {e}: outside tolerance and NOT explained: {worst}")
                why.append(w)
            self.log.append((s, int(e), fields, why))
        self.checked += nk
        self.explained += int(any_bad.sum())
        self.flag_flips += int((flag_flip & keep).sum())
        return keep

    def finish(self):
        frac = self.explained / max(self.checked, 1)
        assert frac <= self.max_explained_frac, f"{self.explained} of {self.checked} env-steps needed an explanation ({frac:.4f}): {self.log[:10]}"
        out = {"env_steps": self.checked, "explained": self.explained, "foot_contact_flag_flips": self.flag_flips,
               "by_reason": {w: sum(1 for _, _, _, why in self.log if w in " ".join(why)) for w in ("contact_flag", "limit_crossing", "fp32_backward")}}
        # always in the test output (pytest -s / the captured log of a failure): a regression that starts leaning on the explanations shows here
        print("StepParity:", out, flush=True)
        return out


def assert_close(a, b, tol, frac=0.99, hard=None, what=""):
    """At least `frac` of the envs within `tol` (relative to max(1, |b|), worst element per env); `hard`: no env beyond it."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    per_env = err.reshape(err.shape[0], -1).max(axis=1)
    ok = (per_env < tol).mean()
    assert ok >= frac, f"{what}: only {ok:.3f} of envs within {tol}; worst {per_env.max():.3e}"
    if hard is not None:
        assert per_env.max() < hard, f"{what}: worst env error {per_env.max():.3e}"


# ================================================================== one constructor for the (env, oracle) pair
def phys_of(cfg):
    """Every physics key of the config as DynRef's `phys`, with the defaults T1._cfg_struct gives an absent key: an override of sim.dt, sim.gravity or
    contact.* reaches the oracle as it reaches bg_env_cfg."""
    ct = cfg.get("contact", {}) or {}
    t = cfg["terrain"]
    return {"dt": float(cfg["sim"]["dt"]), "g": tuple(float(v) for v in cfg["sim"]["gravity"]), "contact_k": float(ct.get("stiffness", 4.0e4)),
            "contact_d": float(ct.get("damping", 600.0)), "contact_ramp": float(ct.get("damping_ramp", 1.0e-3)),
            "friction_visc": float(ct.get("friction_viscosity", 1.0e4)), "limit_k": float(ct.get("joint_limit_stiffness", 2000.0)),
            "limit_d": float(ct.get("joint_limit_damping", 20.0)), "clamp_qd": int(bool(ct.get("clamp_dof_velocity", True))),
            "body_gate_height": float(ct.get("body_gate_height", 0.45)), "terrain_mu": 0.5 * (t["static_friction"] + t["dynamic_friction"]),
            "terrain_restitution": t["restitution"], "self_collisions": int(int(cfg["asset"].get("self_collisions", 0)) == 0),
            "self_k": float(ct.get("self_stiffness", 4.0e4)), "self_d": float(ct.get("self_damping", 150.0)), "self_mu": float(ct.get("self_friction", 1.0)),
            "self_visc": float(ct.get("self_friction_viscosity", 100.0))}


def make_oracle(cfg, model, params, tdict=None, real="f64"):
    """T1Ref over a DynRef whose physics constants are the config's (real="f32": the single-precision twin, task logic float64 either way)."""
    from oracle.dyn_ref import DynRef
    from oracle.task_ref import T1Ref

    dyn = DynRef(model, feet_edge_pos=cfg["asset"]["feet_edge_pos"], terrain=tdict, phys=phys_of(cfg), real=real)
    return T1Ref(cfg, model, dyn, params, terrain=tdict, seed=cfg["basic"]["seed"], rank=0)


def make_pair(terrain, n, overrides=None):
    """cfg, env (the HIP T1), ref (the float64 oracle on the env's model, terrain and per-env parameters)."""
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": n, "terrain.type": terrain}
    ov.update(overrides or {})
    cfg = load_cfg("T1", ov)
    env = T1(cfg)
    tdict = None
    if terrain != "plane":
        t = env.terrain
        tdict = dict(height_field_raw=t.height_field_raw, hscale=t.horizontal_scale, vscale=t.vertical_scale, border_px=t.border_pixels)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    params = dict(kp=f32(env._kp), kd=f32(env._kd), fric=f32(env._fric), mass_scale=f32(env._mass_scale), com_off=f32(env._com_off),
                  foot_mat=f32(env._foot_mat), bms=f32(env._bms), origins=f32(env._origins))
    return cfg, env, make_oracle(cfg, env.model, params, tdict)


def make_twin(cfg, model, ref):
    """The same oracle with its physics in single precision (oracle/dyn_ref.c built as libdynref32.so): how far fp32 rounding alone moves this
    algorithm on a given state.  Task logic stays the float64 numpy code; parameters and terrain are `ref`'s."""
    return make_oracle(cfg, model, ref.p, ref.terrain, real="f32")


def host_params(cfg, model, n):
    """Per-env parameters drawn in the yaml's randomization.* ranges on the host, for an oracle that has no env beside it (flat ground).  Its own
    seeded draws, not T1._create_envs': two configs that differ in control.stiffness / damping alone get the same scaling draws."""
    rng = np.random.default_rng(int(cfg["basic"]["seed"]))
    rnd = cfg["randomization"]

    def draw(x, spec):
        if spec is None:
            return x, np.zeros_like(x)
        a, b = spec["range"]
        raw = rng.standard_normal(x.shape) if spec["distribution"] == "gaussian" else rng.random(x.shape)
        val = a + b * raw if spec["distribution"] == "gaussian" else a + (b - a) * raw
        return (x + val if spec["operation"] == "additive" else x * val), raw

    kp, kd = np.zeros((n, 12)), np.zeros((n, 12))
    for i, name in enumerate(model.dof_names):
        for key in cfg["control"]["stiffness"]:
            if key in name:
                kp[:, i], kd[:, i] = cfg["control"]["stiffness"][key], cfg["control"]["damping"][key]
    kp, kd, fric = draw(kp, rnd.get("dof_stiffness"))[0], draw(kd, rnd.get("dof_damping"))[0], draw(np.zeros((n, 12)), rnd.get("dof_friction"))[0]
    mass_scale, com_off, bms = np.ones((n, 13)), np.zeros((n, 13, 3)), np.zeros((n, 4))
    for b in range(13):
        ck, mk = ("base_com", "base_mass") if b == 0 else ("other_com", "other_mass")
        com_off[:, b], craw = draw(np.zeros((n, 3)), rnd.get(ck))
        mass_scale[:, b], sraw = draw(np.ones(n), rnd.get(mk))
        if b == 0:
            bms[:, :3], bms[:, 3] = craw, sraw
    fm = np.zeros((n, 2, 3))
    for k, key in enumerate(("friction", "compliance", "restitution")):
        fm[:, :, k] = draw(np.zeros((n, 2)), rnd.get(key))[0]
    fm[:, :, 1] = np.maximum(fm[:, :, 1], 1e-3)
    origins = np.zeros((n, 3))
    cols = np.floor(np.sqrt(n))
    xx, yy = np.meshgrid(np.arange(np.ceil(n / cols)), np.arange(cols), indexing="ij")
    origins[:, 0], origins[:, 1] = cfg["env"]["env_spacing"] * xx.flatten()[:n], cfg["env"]["env_spacing"] * yy.flatten()[:n]
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return dict(kp=f32(kp), kd=f32(kd), fric=f32(fric), mass_scale=f32(mass_scale), com_off=f32(com_off), foot_mat=f32(fm), bms=f32(bms), origins=f32(origins))


_ATTR = {"root_states": "root", "dof_pos": "q", "dof_vel": "qd", "last_dof_targets": "last_tgt", "actions": "actions", "last_actions": "last_actions",
         "last_dof_vel": "last_qd", "last_root_vel": "last_rootvel", "commands": "cmd", "gait_frequency": "gait_f", "gait_process": "gait_p",
         "filtered_lin_vel": "filt_lin", "filtered_ang_vel": "filt_ang", "last_feet_pos": "last_feet", "pushing": "push",
         "episode_length_buf": "ep_len", "cmd_resample_time": "cmd_time", "delay_steps": "delay"}
_INT_ATTR = ("ep_len", "cmd_time", "delay")


def snapshot(ref):
    """The oracle's whole mutable state (to start a second oracle from the same inputs)."""
    s = {a: np.array(getattr(ref, a), copy=True) for a in _ATTR.values()}
    s["step_count"] = ref.step_count
    return s


def restore(ref, snap):
    for a in _ATTR.values():
        setattr(ref, a, snap[a].copy())
    ref.step_count = snap["step_count"]


class OracleEnv:
    """The oracle's fp32 twin behind the part of T1's interface that StepParity and run_case use, so that the twin is held to the float64 oracle by the
    very code that holds the HIP env to it.  Like the kernel it keeps its state in fp32 between steps: both sides of a step start from identical inputs."""

    def __init__(self, cfg, twin):
        import torch

        self._t, self.cfg, self.r, self.device, self.dt = torch, cfg, twin, "cpu", twin.dt
        self.reward_names, self._derived, self._finished = list(twin.scales), None, 0

    def _round(self):
        for a in _ATTR.values():
            if a not in _INT_ATTR:
                setattr(self.r, a, np.asarray(getattr(self.r, a), dtype=np.float32).astype(np.float64))

    def get_field(self, name):
        n = self.r.n
        if name in ("feet_contact", "torques", "feet_pos"):
            return self._t.as_tensor(np.asarray(self._derived[name], dtype=np.float32).reshape(n, -1).copy())
        a = _ATTR[name]
        return self._t.as_tensor(np.asarray(getattr(self.r, a)).astype(np.int32 if a in _INT_ATTR else np.float32).reshape(n, -1).copy())

    def set_field(self, name, value):
        a = _ATTR[name]
        old = np.asarray(getattr(self.r, a))
        setattr(self.r, a, np.asarray(self._t.as_tensor(value).cpu().numpy(), dtype=np.float32).astype(old.dtype).reshape(old.shape))

    root_states = property(lambda self: self.get_field("root_states"))
    dof_pos = property(lambda self: self.get_field("dof_pos"))
    dof_vel = property(lambda self: self.get_field("dof_vel"))
    commands = property(lambda self: self.get_field("commands"))

    @property
    def common_step_counter(self):
        return self.r.step_count

    @common_step_counter.setter
    def common_step_counter(self, v):
        self.r.step_count = int(v)

    def _pack(self, obs, priv):
        f = lambda a: self._t.as_tensor(np.asarray(a, dtype=np.float32))
        return f(obs), {"privileged_obs": f(priv)}

    def reset(self):
        obs, priv = self.r.reset()
        self._round()
        return self._pack(obs, priv)

    def step(self, actions):
        obs, priv, rew, done, tout, scaled, derived = self.r.step(self._t.as_tensor(actions).cpu().numpy().astype(np.float64))
        self._derived = derived
        self._round()
        self._finished += int(np.sum(done))
        f = lambda a: self._t.as_tensor(np.asarray(a, dtype=np.float32))
        o, extras = self._pack(obs, priv)
        extras.update(time_outs=self._t.as_tensor(np.asarray(tout)), rew_terms={k: f(v) for k, v in scaled.items()})
        return o, f(rew), self._t.as_tensor(np.asarray(done)), extras

    def episode_stats(self, reset=False):
        return self._t.tensor([float(self._finished)] + [0.0] * 29)


def make_oracle_pair(n, overrides=None):
    """cfg, OracleEnv(fp32 twin), float64 oracle on flat ground, without a GPU.  The model is the config's asset.file, resolved as T1 resolves it."""
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.urdf import load_model

    ov = {"env.num_envs": n, "terrain.type": "plane"}
    ov.update(overrides or {})
    cfg = load_cfg("T1", ov)
    model = load_model(cfg["asset"]["file"], cfg["asset"].get("collapse_fixed_joints", True))
    ref = make_oracle(cfg, model, host_params(cfg, model, n))
    return cfg, OracleEnv(cfg, make_twin(cfg, model, ref)), ref


# ================================================================== the config surface away from the shipped values
# One table for tests/test_config_surface_ref.py (the cases are well-posed on the oracle alone) and tests/test_gpu_config_surface.py (the kernel matches
# the oracle under them).  Per key: the value, the outputs the key governs, and the steps of the window at which it can show ("any", or the step of a
# kick, a push start, a push end, a step with a push in force, "limit": the first step, over the envs arranged past a joint limit, or "reset":
# T1.reset()).  Outputs, each with the tolerance StepParity holds it to:
#   ("obs", a, b) / ("priv", a, b)   columns [a, b) of the observation / privileged observation           STATE_TOL["obs"] / ["priv"]
#   ("term", name) / ("total",)      a scaled reward term / the total reward                               REW_TOL (relative to max(|.|, REW_FLOOR))
#   ("state",)                       the post-physics state: root, dof_pos, dof_vel, mean torques          STATE_TOL of each
#   ("root_vel",) / ("push",)        the root's velocities after the kick / the stored push wrench         STATE_TOL["root"] / 1e-4 (the step test's bound)
#   ("reset", attr)                  the oracle attribute after reset()                                    1e-5 (the reset test's bound on the root)
# The values started from the issue's list; where one moved, the reason stands beside it.  The thresholds (SENS_FACTOR x tolerance in SENS_SHARE of
# the envs; ACTIVE_SHARE of the env-steps above REW_FLOOR) never moved.
SENS_FACTOR, SENS_SHARE, ACTIVE_SHARE, SWING_SHARE = 10.0, 0.5, 0.5, 0.10
TOTAL_POS_SHARE, TOTAL_CLIP_SHARE, TOTAL_NONZERO_SHARE = 0.25, 0.25, 0.90
TRACKING = [("term", "tracking_lin_vel_x"), ("term", "tracking_lin_vel_y"), ("term", "tracking_ang_vel")]


def _rs(dist, op, a, b):
    return {"range": [a, b], "operation": op, "distribution": dist}


REWARD_KEYS = {
    "rewards.scales.dof_vel_limits": (-0.05, [("term", "dof_vel_limits")], "any"),
    "rewards.scales.torque_limits": (-0.01, [("term", "torque_limits")], "any"),
    "rewards.scales.feet_vel_z": (-0.5, [("term", "feet_vel_z")], "any"),
    # 4.0, not the issue's 5.0: the unclipped total is then negative in clearly more than half of the env-steps, which only_positive_rewards: false needs
    "rewards.scales.survival": (4.0, [("term", "survival")], "any"),
    "rewards.scales.torques": (-1.0e-4, [("term", "torques")], "any"),
    "rewards.scales.base_height": (-5.0, [("term", "base_height")], "any"),
    "rewards.scales.action_rate": (-0.3, [("term", "action_rate")], "any"),
    "rewards.soft_dof_pos_limit": (0.6, [("term", "dof_pos_limits")], "any"),
    "rewards.soft_dof_vel_limit": (0.1, [("term", "dof_vel_limits")], "any"),
    "rewards.soft_torque_limit": (0.3, [("term", "torque_limits")], "any"),
    "rewards.tracking_sigma": (0.5, TRACKING, "any"),
    "rewards.base_height_target": (0.62, [("term", "base_height")], "any"),
    "rewards.swing_period": (0.3, [("swing",)], "any"),
    "rewards.feet_distance_ref": (0.25, [("term", "feet_distance")], "any"),
    "control.action_scale": (0.5, [("state",)], "any"),
    "normalization.clip_actions": (0.4, [("obs", 35, 47)], "any"),
    "normalization.filter_weight": (0.3, [("term", "lin_vel_z")] + TRACKING, "any"),
    "normalization.gravity": (0.5, [("obs", 0, 3)], "any"),
    "normalization.lin_vel": (2.0, [("priv", 4, 7), ("obs", 6, 8)], "any"),
    # 2.0, not the issue's 0.25: with the combined case's noise.ang_vel: null, a factor below 1 shrinks the shipped noise that the null entry removes
    # under 10 x the observation tolerance
    "normalization.ang_vel": (2.0, [("obs", 3, 6), ("obs", 8, 9)], "any"),
    "normalization.dof_pos": (2.0, [("obs", 11, 23)], "any"),
    "normalization.dof_vel": (0.05, [("obs", 23, 35)], "any"),
    "normalization.push_force": (0.05, [("priv", 8, 11)], "pushed"),
    "normalization.push_torque": (0.25, [("priv", 11, 14)], "pushed"),
}
# the reward terms the group activates or re-parameterises (feet_swing has its own condition, SWING_SHARE)
REWARD_TERMS = ["dof_vel_limits", "torque_limits", "feet_vel_z", "survival", "torques", "base_height", "action_rate", "dof_pos_limits",
                "tracking_lin_vel_x", "tracking_lin_vel_y", "tracking_ang_vel", "feet_distance"]
NEW_TERMS = ["dof_vel_limits", "torque_limits", "feet_vel_z"]

# Modes of apply_rand (0 null, 1 gaussian additive, 2 gaussian scaling, 3 uniform additive, 4 uniform scaling): observation sites 3 2 0 4 1 2, state
# sites 3 2 3 3 4 1 0.  Moved from the issue's list, all for the 10 x tolerance rule (0.05 in observation units): the null entry sits on ang_vel, whose
# shipped noise (0.1) is large enough to be missed, not on dof_pos (0.01); dof_pos takes the uniform scaling; gravity, height and kick_ang_vel got wider
# ranges; dof_vel is gaussian ADDITIVE with a non-zero mean, which no shipped entry has; init_dof_pos takes a scaling (the shipped default pose is
# non-zero on the pitch joints), so that mode 4 occurs at a state site where it is not degenerate (a scaled zero push is a zero push); the null state
# entry sits on init_base_lin_vel_xy and not on push_torque, so that normalization.push_torque still has a torque to scale in the combined case.
# The intervals are no multiples of either step length (0.05 / 0.02 and 0.05 / 0.021 both round up to 3), so the step counts do not hang on one
# rounding of a quotient.  friction_viscosity 200 and damping_ramp 5e-3 (below): 5000 and 2e-3 moved the post-physics state in too few envs.
NOISE_KEYS = {
    "noise.gravity": (_rs("uniform", "additive", -0.2, 0.2), [("obs", 0, 3)], "any"),
    "noise.lin_vel": (_rs("gaussian", "scaling", 1.0, 0.02), [("priv", 4, 7)], "any"),
    "noise.ang_vel": (None, [("obs", 3, 6)], "any"),
    "noise.dof_pos": (_rs("uniform", "scaling", 0.5, 1.5), [("obs", 11, 23)], "any"),
    "noise.dof_vel": (_rs("gaussian", "additive", 0.5, 2.0), [("obs", 23, 35)], "any"),
    "noise.height": (_rs("gaussian", "scaling", 1.0, 0.3), [("priv", 7, 8)], "any"),
    "randomization.kick_lin_vel": (_rs("uniform", "additive", -0.2, 0.2), [("root_vel",)], "kick"),
    "randomization.kick_ang_vel": (_rs("gaussian", "scaling", 0.5, 0.3), [("root_vel",)], "kick"),
    "randomization.push_force": (_rs("uniform", "additive", -20.0, 20.0), [("push",)], "push_start"),
    "randomization.push_torque": (_rs("uniform", "additive", -3.0, 3.0), [("push",)], "push_start"),
    "randomization.init_dof_pos": (_rs("uniform", "scaling", 0.8, 1.2), [("reset", "q")], "reset"),
    "randomization.init_base_pos_xy": (_rs("gaussian", "additive", 0.0, 0.3), [("reset", "root")], "reset"),
    "randomization.init_base_lin_vel_xy": (None, [("reset", "root")], "reset"),
    "randomization.kick_interval_s": (0.05, [("root_vel",)], "kick"),
    "randomization.push_interval_s": (0.09, [("push",)], "push_start"),
    "randomization.push_duration_s": (0.03, [("push",)], "push_end"),
}

PHYSICS_KEYS = {
    "control.decimation": (7, [("state",)], "any"),
    "sim.dt": (0.003, [("state",)], "any"),
    "sim.gravity": ([0.0, 0.0, -8.0], [("state",)], "any"),
    "contact.stiffness": (30000.0, [("state",)], "any"),
    "contact.damping": (400.0, [("state",)], "any"),
    "contact.joint_limit_stiffness": (1000.0, [("state",)], "limit"),
    "contact.joint_limit_damping": (10.0, [("state",)], "limit"),
    "contact.friction_viscosity": (200.0, [("state",)], "any"),
    "contact.damping_ramp": (5.0e-3, [("state",)], "any"),
    "control.stiffness": ({"Hip": 150.0, "Knee": 180.0, "Ankle": 40.0}, [("state",)], "any"),
    "control.damping": ({"Hip": 4.0, "Knee": 6.0, "Ankle": 1.5}, [("state",)], "any"),
}
# terms whose value hangs on the policy-step length beyond their scale x dt, and the mean torque's divisor
PHYSICS_TERMS = ["survival", "dof_acc", "root_acc", "torques"]
SIGNED = {"rewards.only_positive_rewards": (False, [("total",)], "any")}


def _case(start_count, terms, total, *groups):
    keys = {}
    for g in groups:
        keys.update(g)
    return {"keys": keys, "overrides": {k: v[0] for k, v in keys.items()}, "terms": terms, "total": total, "start_count": start_count,
            "new_terms": [t for t in NEW_TERMS if "rewards.scales." + t in keys], "swing": "rewards.swing_period" in keys,
            "limits": "contact.joint_limit_stiffness" in keys}


# start_count places the window's steps (counter values start_count + 1 .. + 6) over a kick, a push start and a push end where the case has them:
# rewards: the shipped 250-step push schedule, start at 250; noise and combined: kicks every 3 steps, pushes every 5, for 2; physics: at 21 ms the shipped
# schedule is 96 / 239 / 48 steps, push start at 239, kick at 240.  The noise and physics groups run with only_positive_rewards: false so that their
# total reward is compared as a number and not as 0 against 0 (the shipped scales give a negative total throughout).
CONFIG_CASES = {
    "rewards_positive": _case(246, REWARD_TERMS, "clipped", REWARD_KEYS),
    "rewards_signed": _case(246, REWARD_TERMS, "signed", REWARD_KEYS, SIGNED),
    "noise": _case(4, [], "signed", NOISE_KEYS, SIGNED),
    "physics": _case(236, PHYSICS_TERMS, "signed", PHYSICS_KEYS, SIGNED),
    "combined": _case(4, REWARD_TERMS + ["dof_acc", "root_acc"], "clipped", REWARD_KEYS, NOISE_KEYS, PHYSICS_KEYS),
}
N_CASE = 96
AIRBORNE = slice(12, 28)  # the envs with an arranged state (arrange_for)


def schedule(cfg, dt):
    r = cfg["randomization"]
    return tuple(int(math.ceil(r[k] / dt)) for k in ("kick_interval_s", "push_interval_s", "push_duration_s"))


def kick_step(cfg, env):
    """Does the env step that is about to run apply a kick (t1.py:501: global counter, all envs at once)?"""
    return (env.common_step_counter + 1) % schedule(cfg, env.dt)[0] == 0


def arrange_for(case, lift=0.15, phase=0.12, freq=0.1, past=0.03, spread=0.3):
    """The window's arranged states of a case, all on the envs of AIRBORNE, which are lifted clear of the ground for the whole window (both feet out
    of contact, no stiff contact near them).
      rewards.swing_period    a slow gait clock at a phase inside the left foot's swing window of width 0.3 (|phase - 0.25| < 0.15) and outside the
                              shipped one (< 0.1): feet_swing is 1 under the case and 0 under the shipped period
      contact.joint_limit_*   the limit spring acts on a joint past its limit only, and the window's actions leave none there: the left hip yaw starts
                              `past` rad beyond its limit of 1 rad, toes out, with that leg abducted by `spread` rad so that its heel stays
                              clear of the right foot (no leg-against-leg contact), held by the actuators until the env's delayed target
                              arrives; spring and actuator bring it back within the first compared step, at which the two keys are judged
                              ("limit": over these envs)"""
    if not (case["swing"] or case["limits"]):
        return None

    def arrange(env):
        import torch

        put = lambda k, v: env.set_field(k, torch.as_tensor(v).float())
        root, feet = env.get_field("root_states"), env.get_field("last_feet_pos")
        root[AIRBORNE, 2] += lift
        feet[AIRBORNE, 2] += lift; feet[AIRBORNE, 5] += lift
        put("root_states", root); put("last_feet_pos", feet)
        if case["swing"]:
            gf, gp = env.get_field("gait_frequency"), env.get_field("gait_process")
            gf[AIRBORNE, 0] = freq; gp[AIRBORNE, 0] = phase
            put("gait_frequency", gf); put("gait_process", gp)
        if case["limits"]:
            q, tgt = env.get_field("dof_pos"), env.get_field("last_dof_targets")
            q[AIRBORNE, 2] = tgt[AIRBORNE, 2] = 1.0 + past
            q[AIRBORNE, 1] = tgt[AIRBORNE, 1] = spread
            put("dof_pos", q); put("last_dof_targets", tgt)
    return arrange


def run_case(cfg, env, ref, start_count, settle=15, steps=6, arrange=None, before_step=None, after_step=None, fp16=False, state_tol=None):
    """test_step_matches_oracle's procedure as a function of (cfg, env, ref): settle, forced time-outs and command resamples, `steps` compared env
    steps through StepParity from identical inputs.  Returns the StepParity summary and, per compared step, the oracle's and the env's total and
    scaled terms with the mask of compared envs (for the non-vacuity shares).  fp16: the oracle's stored state is rounded as the kernel's is."""
    import torch

    n = ref.n
    env.reset(); ref.reset()
    rng = np.random.default_rng(11)
    for _ in range(settle):  # feet on the ground; then seed episode ends / resamples for some envs
        env.step(torch.tensor(rng.uniform(-0.3, 0.3, (n, 12)), dtype=torch.float32, device=env.device))
    max_ep = int(math.ceil(cfg["rewards"]["episode_length_s"] / env.dt))
    ep = env.get_field("episode_length_buf")
    ep[:6, 0] = max_ep - 2  # time-out within the window
    env.set_field("episode_length_buf", ep)
    ct = env.get_field("cmd_resample_time")
    ct[6:12, 0] = ep[6:12, 0] + 2  # command resample within the window
    ct[:6, 0] = 5000
    env.set_field("cmd_resample_time", ct)
    env.common_step_counter = start_count
    if arrange is not None:
        arrange(env)
    sp = StepParity(cfg, env, ref, state_tol=state_tol)
    flags_bad, rec = 0, {"ref_total": [], "env_total": [], "ref_terms": [], "env_terms": [], "keep": []}
    ptol, ctol = (2e-3, 2e-3) if fp16 else (1e-4, 1e-5)  # fp16 state: one fp16 ulp where the two sides round a near-tie differently
    for s in range(steps):
        sp.begin()
        if before_step is not None:
            before_step(s)
        kicked = kick_step(cfg, env)
        act = rng.uniform(-0.6, 0.6, (n, 12)).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        out = ref.step(act.astype(np.float64))
        if fp16:
            ref.quantize_state_fp16()
        keep = sp.check(s, act, obs, rew, done, extras, out, kicked=kicked)
        flags_bad += int((~keep).sum()) + int((extras["time_outs"].cpu().numpy() != out[4]).sum())
        assert (env.get_field("cmd_resample_time").cpu().numpy()[:, 0][keep] == ref.cmd_time[keep]).all()
        assert (env.get_field("episode_length_buf").cpu().numpy()[:, 0][keep] == ref.ep_len[keep]).all()
        assert rel_state(env.get_field("pushing").cpu().numpy(), ref.push).max() < ptol, f"step {s} push"
        assert rel_state(env.commands.cpu().numpy()[keep], ref.cmd[keep]).max() < ctol, f"step {s} commands"
        rec["ref_total"].append(np.asarray(out[2], dtype=np.float64)); rec["env_total"].append(rew.cpu().numpy().astype(np.float64))
        rec["ref_terms"].append({k: np.asarray(v, dtype=np.float64) for k, v in out[5].items()})
        rec["env_terms"].append({k: extras["rew_terms"][k].cpu().numpy().astype(np.float64) for k in out[5]})
        rec["keep"].append(keep)
        if after_step is not None:
            after_step(s, sp, act, out, keep)
    summary = sp.finish()
    print("step parity:", summary, sp.log)
    assert flags_bad <= 2, f"{flags_bad} termination / time-out flags differ"
    st = env.episode_stats(reset=False).cpu().numpy()
    assert st[-1] == 0, "non-finite resets during a benign rollout"
    assert st[0] >= 6  # the forced time-outs were counted as finished episodes
    return summary, rec


def shares(case, rec, side):
    """The non-vacuity shares of one side ("ref": the oracle's outputs, "env": the env's own) over the compared env-steps: per term of the case the
    share above REW_FLOOR, the shares of the total above the floor / exactly zero / beyond the floor in magnitude, and feet_swing's share."""
    keep = np.concatenate(rec["keep"])
    tot = np.concatenate(rec[side + "_total"])[keep]
    cat = lambda name: np.concatenate([t[name] for t in rec[side + "_terms"]])[keep]
    out = {"terms": {name: float((np.abs(cat(name)) > REW_FLOOR).mean()) for name in case["terms"]},
           "total_positive": float((tot > REW_FLOOR).mean()), "total_zero": float((tot == 0.0).mean()), "total_nonzero": float((np.abs(tot) > REW_FLOOR).mean())}
    if case["swing"]:
        out["feet_swing"] = float((np.abs(cat("feet_swing")) > REW_FLOOR).mean())
    return out


def assert_not_vacuous(case, sh, what):
    for name, v in sh["terms"].items():
        assert v >= ACTIVE_SHARE, f"{what}: reward term {name} above the floor in {v:.3f} of the env-steps only"
    if case["total"] == "clipped":
        assert sh["total_positive"] >= TOTAL_POS_SHARE and sh["total_zero"] >= TOTAL_CLIP_SHARE, f"{what}: total reward positive in {sh['total_positive']:.3f}, clipped in {sh['total_zero']:.3f}"
    else:
        assert sh["total_nonzero"] >= TOTAL_NONZERO_SHARE, f"{what}: total reward non-zero in {sh['total_nonzero']:.3f} of the env-steps only"
    if case["swing"]:
        assert sh["feet_swing"] >= SWING_SHARE, f"{what}: feet_swing non-zero in {sh['feet_swing']:.3f} of the env-steps only"


# ================================================================== stages that couple envs, or walk them with a grid smaller than the work
# One table for tests/test_env_scale_ref.py (the sizes and placements cross the thresholds they claim to cross, the references satisfy the
# conditions on their own) and tests/test_gpu_env_scale.py (the kernels).  A large run whose env e carries the state and per-env parameters of env
# src[e] of a 256-env run must reproduce that env's outputs bit for bit, whichever kernel, trip or list position served it.
SCALE_N, SCALE_SRC = 33000, 256        # 1,032 blocks of 32 envs, the last one of 8
RESAMPLE_NS = (70000, 600)             # 274 resample blocks (two per thread of the offsets scan, threads 137.. empty) / three with a ragged tail
SPARSE_ONE = (0, 255, 256, 511, 512, 1023, 1024, 1031)   # forward dynamics, sparse batch: blocks with one listed env ...
SPARSE_FULL = (300, 1031)                                # ... blocks listed whole (1031 is the ragged last block), plus 3 % of all others
LOW_BASES = (0, 3, 7)                  # gated simulate / env step: low envs in blocks b, b + BODY_GRID, b + 2 BODY_GRID
PER_ENV_PARAMS = ("dof_stiffness", "dof_damping", "dof_friction", "mass_scale", "com_offset", "foot_material", "base_mass_scaled", "delay_steps")
# The stated tolerance per contact family of tests/test_gpu_dynamics.py and tests/test_gpu_sim_calls.py, the one table those files'
# parametrisations and the scale cases read: relative 1e-4 on the accelerations without a contact, 5e-4 with stiff sole or leg-against-leg contacts, 1e-3
# with the trunk box and the hip-yaw / shank cylinders on the ground.
FAMILY_TOL = {False: 1e-4, True: 5e-4, "low": 1e-3, "crossed": 5e-4, "sparse_crossed": 5e-4, "crossed_gated": 5e-4}


def kernel_constants(text=None):
    """The constants the sizes of the scale cases rest on, read from the source text of csrc/bg_sim.hip."""
    import re

    if text is None:
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "booster_gym_amd", "csrc", "bg_sim.hip")) as f:
            text = f.read()
    one = lambda pat: int(re.search(pat, text, re.S).group(1))
    return {"ENVS_PER_BLOCK": one(r"constexpr int ENVS_PER_BLOCK = (\d+);"), "BODY_GRID": one(r"constexpr int BODY_GRID = (\d+);"),
            "RS_BLOCK": one(r"constexpr int RS_BLOCK = (\d+);"),
            "FD_GRID": one(r"forward_dynamics_body_kernel<true>, dim3\(nb < (\d+) \? nb : \1\)"),
            "COMPACT_BLOCK": one(r"__launch_bounds__\((\d+)\) void aba_compact_kernel"),
            "COMPACT_GRID_DIV": one(r"aba_compact_kernel, dim3\(\(nb \+ \d+\) / (\d+)\)")}


def sparse_listed(n=SCALE_N, epb=32, seed=5):
    """The sparse forward-dynamics batch: which envs are to be listed for kernel B."""
    rng = np.random.default_rng(seed)
    listed = rng.random(n) < 0.03
    for b in SPARSE_ONE + SPARSE_FULL:
        listed[b * epb:(b + 1) * epb] = False
    for b in SPARSE_ONE:
        rows = min(epb, n - b * epb)
        listed[b * epb + int(rng.integers(0, rows))] = True
    for b in SPARSE_FULL:
        listed[b * epb:(b + 1) * epb] = True
    return listed


def low_placement(n=SCALE_N, epb=32, grid=512, seed=6):
    """Gated simulate / env step: which envs lie low.  Blocks b, b + grid, b + 2 grid for b in LOW_BASES hold some; block 3 + grid is low whole, block 7
    holds a single one, the ragged last block (7 + 2 grid at the shipped constants) holds low envs too."""
    rng = np.random.default_rng(seed)
    low = np.zeros(n, dtype=bool)
    for base in LOW_BASES:
        for trip in range(3):
            b = base + trip * grid
            rows = min(epb, n - b * epb)
            if rows <= 0:
                continue
            k = rows if (base, trip) == (3, 1) else 1 if (base, trip) == (7, 0) else min(rows, 5)
            low[b * epb + rng.choice(rows, size=k, replace=False)] = True
    return low


def block_masks(flags, epb=32):
    """Per block of `epb` envs the number of flagged envs and the block's size."""
    n = len(flags)
    nb = (n + epb - 1) // epb
    pad = np.zeros(nb * epb, dtype=bool); pad[:n] = flags
    return pad.reshape(nb, epb).sum(axis=1), np.minimum(epb, n - np.arange(nb) * epb)


def shuffled_src(member, classes, seed=7):
    """src [N] onto the source envs: env e of class member[e] (an int) takes a source env of classes[member[e]] (an index array), every source env
    occurring at least once, in a fixed-seed random arrangement."""
    rng = np.random.default_rng(seed)
    member = np.asarray(member)
    src = np.empty(len(member), dtype=np.int64)
    for c, pool in enumerate(classes):
        where = np.nonzero(member == c)[0]
        assert len(where) >= len(pool), f"class {c}: {len(where)} envs cannot hold {len(pool)} source envs"
        pick = np.concatenate([pool, rng.choice(pool, size=len(where) - len(pool))])
        rng.shuffle(pick)
        src[where] = pick
    return src


def spot_positions(n, must=(), count=64, epb=32, seed=8):
    """`count` env positions for the oracle's spot check: the first and the last env, both sides of the boundaries at 16,384 and 32,768 envs, the
    ragged last block, the positions of `must`, the rest at random."""
    fixed = [0, n - 1] + [e for e in (16383, 16384, 32767, 32768) if e < n] + list(range((n - 1) // epb * epb, n))
    pos = list(dict.fromkeys([int(e) for e in fixed] + [int(e) for e in must]))[:count]
    rng = np.random.default_rng(seed)
    rest = [int(e) for e in rng.permutation(n) if int(e) not in set(pos)]
    return np.array(sorted(pos + rest[:count - len(pos)]))


def leg_clearance(dyn, flat_model, root, q):
    """self_clearance of csrc/bg_dyn.h in float64: the lateral gap between the capsules of the two legs along the trunk's y axis; kernel A of the
    gated forward dynamics leaves an env to kernel B when it is negative."""
    from oracle.dyn_ref import self_capsules

    pos, rot = dyn.body_poses(np.asarray(root, dtype=np.float64), np.asarray(q, dtype=np.float64))
    ey = rot[0][:, 1]
    inner = []
    for leg, fb in enumerate((6, 12)):
        ext = []
        for body, a, b, r in self_capsules(flat_model, [fb]):
            ys = [float(ey @ (pos[body] + rot[body] @ np.asarray(p) - pos[0])) for p in (a, b)]
            ext.append(min(ys) - r if leg == 0 else -(max(ys) + r))
        inner.append(min(ext))
    return inner[0] + inner[1]


def fd_listed(dyn, flat_model, root, q, gate=0.45):
    """(listed, margin): does kernel A of the gated forward dynamics leave this state to kernel B (trunk lower than the gate above the terrain, or the
    legs can meet), and by how much the nearer of the two tests is decided."""
    h = float(root[2]) - dyn.terrain_height(float(root[0]), float(root[1])) - gate
    c = leg_clearance(dyn, flat_model, root, q)
    return (h < 0 or c < 0), (max(-h, -c) if (h < 0 or c < 0) else min(h, c))


def fd_tables(dyn, flat_model, states_of, terrain_shift=None, margin=1e-4):
    """Source states of the forward-dynamics scale cases from test_gpu_dynamics._states at that file's seed (3) and size (256), whose excused list is
    empty: source env i carries state i of one family, chosen per i as the first family whose state is listed / not listed by more than `margin`
    (metres; fp32 rounding of the two tests is 1e-7).  Returns {"all": every source env listed, "sparse": even source envs listed and odd ones not,
    "crossed": the crossed family (ungated env)}, each a dict of root, q, qd, tau, w [256, .], family [256], listed [256] and ok [256]: by the
    kernel's rule not every "crossed_gated" or "low" state is left to kernel B (218 and 224 of the 256 are), so a source env with no such state in
    either family is not ok, and pool = the source envs that are ok in "all" and in "sparse" (the only ones a large batch may point to)."""
    fams = {}
    for fam in (False, True, "low", "crossed", "crossed_gated"):
        root, q, qd, tau, w = states_of(np.random.default_rng(3), flat_model, SCALE_SRC, fam)
        if terrain_shift is not None:
            terrain_shift(root)
        fams[fam] = (root, q, qd, tau, w)

    def table(want, order):
        out = {k: [] for k in ("root", "q", "qd", "tau", "w", "family", "listed", "ok")}
        for i in range(SCALE_SRC):
            ok = False
            for fam in order(i):
                listed, m = fd_listed(dyn, flat_model, fams[fam][0][i], fams[fam][1][i])
                if listed == want(i) and m > margin:
                    ok = True
                    break
            for k, a in zip(("root", "q", "qd", "tau", "w"), fams[fam]):
                out[k].append(a[i])
            out["family"].append(fam); out["listed"].append(listed); out["ok"].append(ok)
        return {k: (np.array(v) if k != "family" else v) for k, v in out.items()}

    lst = lambda i: ("crossed_gated", "low") if i % 4 < 2 else ("low", "crossed_gated")
    tabs = {"all": table(lambda i: True, lst), "sparse": table(lambda i: i % 2 == 0, lambda i: lst(i) if i % 2 == 0 else (True, False)),
            "crossed": dict(zip(("root", "q", "qd", "tau", "w"), fams["crossed"]), family=["crossed"] * SCALE_SRC, listed=np.zeros(SCALE_SRC, bool),
                            ok=np.ones(SCALE_SRC, bool))}
    tabs["pool"] = np.nonzero(tabs["all"]["ok"] & tabs["sparse"]["ok"])[0]
    return tabs


def fd_spot_check(dyn, tab, src, spots, qacc, cf, params, twin=None):
    """The float64 oracle on the envs `spots` of a large forward-dynamics run (qacc [N,18], cf [N,2,3]; the state of env e is row src[e] of `tab`,
    its parameters are params[.][e] as the kernel holds them), at the tolerance of its source's contact family in tests/test_gpu_dynamics.py: 5e-4
    at least with an active contact, nothing excused.  twin: hold the oracle's fp32 build to the same bounds instead of a kernel.  Returns the worst
    error over its bound and the number of states with a contact."""
    worst, ncontact = 0.0, 0
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    for e in spots:
        i = int(src[e])
        args = tuple(f32(tab[k][i]) for k in ("root", "q", "qd", "tau"))
        kw = dict(base_wrench=f32(tab["w"][i]), mass_scale=f32(params["mass_scale"][e]), com_off=f32(params["com_offset"][e]).reshape(13, 3),
                  foot_mat=f32(params["foot_material"][e]).reshape(6))
        qa, cfr = dyn.forward(*args, **kw)
        got, gcf = (twin.forward(*args, **kw)[0], None) if twin is not None else (np.asarray(qacc[e], dtype=np.float64), cf[e])
        touching = np.abs(cfr).max() > 0
        tol = max(FAMILY_TOL[tab["family"][i]], 5e-4) if touching else FAMILY_TOL[tab["family"][i]]
        raw = np.abs(got - qa).max() / max(1.0, np.abs(qa).max())
        assert raw < tol, f"env {e} (source {i}, {tab['family'][i]}): relative qacc error {raw:.2e}, tolerance {tol:g}"
        worst = max(worst, raw / tol)
        if touching:
            ncontact += 1
            if gcf is not None:
                assert np.abs(np.asarray(gcf, dtype=np.float64) - cfr[[6, 12]]).max() <= 2e-3 * max(1.0, np.abs(cfr).max()), f"env {e}: foot forces"
    return worst, ncontact


def copy_params(small, big, src):
    """The per-env parameters of the small env, through src, into the large one (set_field); returns them as numpy for the oracle."""
    import torch

    idx = torch.as_tensor(src, device=small.device)
    for k in PER_ENV_PARAMS:
        big.set_field(k, small.get_field(k)[idx])
    return {k: big.get_field(k).cpu().numpy() for k in PER_ENV_PARAMS}


def sim_sources(flat_model, states_of, gate, n=SCALE_SRC):
    """Source states of the gated-simulate scale case from test_gpu_dynamics._states at the seed (11) and families of tests/test_gpu_sim_calls.py:
    every fourth source env a "low" state whose trunk is more than 5 cm under the gate (it stays low through ten calls), the others standing states;
    the body wrench of that file.  Returns root, q, qd, tau, bf, bt and is_low [n]."""
    lo = states_of(np.random.default_rng(11), flat_model, n, "low")
    rng = np.random.default_rng(11)
    st = states_of(rng, flat_model, n, True)
    is_low = (np.arange(n) % 4 == 0) & (lo[0][:, 2] < gate - 0.05)
    root, q, qd, tau = (np.where(is_low[:, None], a, b) for a, b in zip(lo[:4], st[:4]))
    assert is_low.sum() >= 32 and (root[~is_low, 2] > gate + 0.05).all()
    bf, bt = rng.normal(size=(n, 13, 3)) * 10.0, rng.normal(size=(n, 13, 3)) * 2.0
    return root, q, qd, tau, bf, bt, is_low


def sim_implied_error(dyn, root, q, qd, tau, bf, bt, par, vel_after):
    """The velocity part of tests/test_gpu_sim_calls.simulate_parity for one env and one gym.simulate: the accelerations implied by the velocities
    `vel_after` [18] (root lin / ang, dof) against the float64 oracle's step from (root, q, qd), relative to max(1, |qacc|), less the fp32 rounding
    of the stored velocities themselves.  bf / bt: the pending body wrench or None."""
    r, qq, qv = np.array(root, dtype=np.float64), np.array(q, dtype=np.float64), np.array(qd, dtype=np.float64)
    qa, _ = dyn.forward_bw(r, qq, qv, tau, bf, bt, **par)
    dyn.step_bw(r, qq, qv, tau, bf, bt, **par)
    vel_r = np.concatenate([r[7:13], qv])
    dt = dyn.phys.dt
    return (np.abs(np.asarray(vel_after, dtype=np.float64) - vel_r).max() / dt - 2e-7 * max(1.0, np.abs(vel_r).max()) / dt) / max(1.0, np.abs(qa).max())
