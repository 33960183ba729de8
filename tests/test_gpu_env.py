"""Parity of the fused HIP env step (through the C ABI) with the oracle (oracle/task_ref.py + oracle/dyn_ref.c) on the same seeded
inputs: every step starts from the HIP state copied into the oracle, so each comparison is one env-step from identical inputs
(10 physics substeps + post-physics task logic + noise).  Tolerances: fp32 kernel vs float64 oracle, contact-rich dynamics.
"""
import numpy as np
import pytest
import torch

import parity_util as PU
from parity_util import FIELDS, StepParity

pytestmark = pytest.mark.gpu


def _make(terrain, n, overrides=None):
    return PU.make_pair(terrain, n, overrides)


def _twin32(cfg, env, ref):
    return PU.make_twin(cfg, env.model, ref)


def _sync_oracle(env, ref):
    PU.sync_oracle(env, ref)


_close = PU.assert_close


@pytest.mark.parametrize("terrain,overrides", [("plane", None), ("trimesh", None), ("plane", {"parallel.exact_still_count": True})])
def test_reset_matches_oracle(terrain, overrides):
    cfg, env, ref = _make(terrain, 64, overrides)
    obs, extras = env.reset()
    o_ref, p_ref = ref.reset()
    if overrides:  # t1.py:381-383: exactly int(still_proportion * K) of the K = 64 envs resampled by reset() stand still
        cmd = env.commands.cpu().numpy()
        still = (cmd == 0).all(axis=1) & (env.get_field("gait_frequency").cpu().numpy()[:, 0] == 0)
        assert int(still.sum()) == int(cfg["commands"]["still_proportion"] * 64) == 6
        assert np.array_equal(still, (ref.cmd == 0).all(axis=1))
    _close(obs.cpu().numpy(), o_ref, 2e-5, frac=1.0, what="reset obs")
    _close(extras["privileged_obs"].cpu().numpy(), p_ref, 2e-5, frac=1.0, what="reset privileged obs")
    _close(env.root_states.cpu().numpy(), ref.root, 1e-5, frac=1.0, what="reset root")
    assert (env.get_field("delay_steps").cpu().numpy()[:, 0] == ref.delay).all()
    assert (env.get_field("cmd_resample_time").cpu().numpy()[:, 0] == ref.cmd_time).all()


_kick_step = PU.kick_step


def _settle(env, n, rng, steps=15):
    for _ in range(steps):
        env.step(torch.tensor(rng.uniform(-0.3, 0.3, (n, 12)), dtype=torch.float32, device=env.device))


EXACT = {"parallel.exact_still_count": True, "parallel.same_step_curriculum": True}


@pytest.mark.parametrize("terrain,start_count,overrides", [("plane", 0, None), ("plane", 96, None), ("trimesh", 246, None), ("trimesh", 297, None),
                                                           ("trimesh", 246, {"commands.curriculum": True}),
                                                           ("plane", 96, {"parallel.exact_still_count": True}),
                                                           ("trimesh", 246, dict(EXACT, **{"commands.curriculum": True}))])
def test_step_matches_oracle(terrain, start_count, overrides):
    """start_count places the global step counter so that the window covers a kick (cnt % 100 == 0), a push start (cnt % 250 == 0)
    and a push end (cnt % 250 == 50).  The last case is BASELINE configs[2] as SURVEY 8(d) words it: the shipped rough terrain WITH the command
    curriculum.  Every env outside a tolerance has to be explained (parity_util.StepParity); the 23 reward terms with a non-zero shipped scale
    (every name of oracle.task_ref.REWARD_NAMES but dof_vel_limits, torque_limits and feet_vel_z, which ship at -0.0 and are dropped from
    extras["rew_terms"]) are compared one by one, relative to their own magnitude.  The other three, the soft_* factors, and the total reward
    away from the clip of only_positive_rewards (here it is 0 against 0 throughout) are held to the oracle by tests/test_gpu_config_surface.py."""
    n = 96
    cfg, env, ref = _make(terrain, n, overrides)
    env.reset(); ref.reset()
    rng = np.random.default_rng(11)
    _settle(env, n, rng)  # feet on the ground; then seed episode ends / resamples for some envs
    ep = env.get_field("episode_length_buf")
    ep[:6, 0] = 1498  # time-out within the window (max_episode_length = 1500)
    env.set_field("episode_length_buf", ep)
    ct = env.get_field("cmd_resample_time")
    exact = bool(cfg["parallel"].get("exact_still_count", False))
    n_rs = 46 if exact else 12  # exact-count mode: 40 envs resample in one step, so that int(0.1 * K) = 4 of them must stand still
    ct[6:n_rs, 0] = ep[6:n_rs, 0] + 2  # command resample within the window
    ct[:6, 0] = 5000
    env.set_field("cmd_resample_time", ct)
    env.common_step_counter = start_count
    still_seen = 0
    if cfg["commands"].get("curriculum", False):
        prob0 = rng.uniform(0.0, 0.8, (21, 21)).astype(np.float32); prob0[10, 10] = 1.0
        env.curriculum_prob = torch.tensor(prob0)
        ref.curr_prob = prob0.astype(np.float64); ref.curr_prob_read = ref.curr_prob.copy()
    sp = StepParity(cfg, env, ref)
    flags_bad = 0
    for s in range(6):
        sp.begin()
        if ref.curriculum:
            ref.curr_levels[:, 0] = env.get_field("env_curriculum_level_lin").cpu().numpy()[:, 0]
            ref.curr_levels[:, 1] = env.get_field("env_curriculum_level_ang").cpu().numpy()[:, 0]
        kicked = _kick_step(cfg, env)
        act = rng.uniform(-0.6, 0.6, (n, 12)).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        out = ref.step(act.astype(np.float64))
        keep = sp.check(s, act, obs, rew, done, extras, out, kicked=kicked)
        flags_bad += int((~keep).sum()) + int((extras["time_outs"].cpu().numpy() != out[4]).sum())
        assert (env.get_field("cmd_resample_time").cpu().numpy()[:, 0][keep] == ref.cmd_time[keep]).all()
        assert (env.get_field("episode_length_buf").cpu().numpy()[:, 0][keep] == ref.ep_len[keep]).all()
        assert PU.rel_state(env.get_field("pushing").cpu().numpy(), ref.push).max() < 1e-4, f"step {s} push"
        assert PU.rel_state(env.commands.cpu().numpy()[keep], ref.cmd[keep]).max() < 1e-5, f"step {s} commands"
        if exact:
            rs_now = env.get_field("cmd_resample_time").cpu().numpy()[:, 0] != sp.pre_cmd_time  # envs that resampled in this step
            st_now = rs_now & (env.commands.cpu().numpy() == 0).all(axis=1) & (env.get_field("gait_frequency").cpu().numpy()[:, 0] == 0)
            assert int(st_now.sum()) == int(float(np.float32(cfg["commands"]["still_proportion"])) * int(rs_now.sum())), (int(st_now.sum()), int(rs_now.sum()))
            still_seen += int(st_now.sum())
        if ref.curriculum:
            assert np.allclose(env.curriculum_prob.cpu().numpy(), np.minimum(ref.curr_prob, 1.0), atol=1e-5), f"step {s}: curriculum grid differs"
            assert (env.get_field("env_curriculum_level_lin").cpu().numpy()[:, 0][keep] == ref.curr_levels[keep, 0]).all()
    assert not exact or still_seen >= 4, "the exact-count path never selected a still env"
    summary = sp.finish()
    print("step parity:", summary, sp.log)
    assert flags_bad <= 2, f"{flags_bad} termination / time-out flags differ"
    st = env.episode_stats(reset=False).cpu().numpy()
    assert st[-1] == 0, "non-finite resets during a benign rollout"
    assert st[0] >= 6  # the forced time-outs were counted as finished episodes


def test_teleport_matches_oracle():
    """_teleport_robot (t1.py:343-360): robots that walked past +-0.75 x border of the rough-terrain field re-enter on the opposite side, root
    and feet shifted by (field size + border).  Four robots are placed past each of the four bounds; one step; root, the stored feet positions
    (last_feet_pos, t1.py:495) and the observations must equal the oracle's within the plain tolerances, no explanation accepted."""
    n = 64
    cfg, env, ref = _make("trimesh", n)
    env.reset(); ref.reset()
    rng = np.random.default_rng(17)
    _settle(env, n, rng)
    t = cfg["terrain"]
    ew, el, b = t["num_terrains"] * t["terrain_width"], t["terrain_length"], t["border_size"]
    root = env.root_states.cpu().numpy().astype(np.float64)
    feet = env.get_field("last_feet_pos").cpu().numpy().astype(np.float64).reshape(n, 2, 3)
    h0 = np.array([ref.dyn.terrain_height(x, y) for x, y in root[:, :2]])
    where = {0: (-0.84 * b, None), 1: (ew + 0.84 * b, None), 2: (None, -0.84 * b), 3: (None, el + 0.84 * b)}
    moved = np.zeros(n, dtype=bool)
    for e in range(16):
        x, y = where[e % 4]
        nx, ny = (root[e, 0] if x is None else x + 0.01 * e), (root[e, 1] if y is None else y + 0.01 * e)
        d = np.array([nx - root[e, 0], ny - root[e, 1]])
        root[e, :2] += d; feet[e, :, :2] += d
        dz = ref.dyn.terrain_height(root[e, 0], root[e, 1]) - h0[e]  # keep the height above the ground (the border strip is flat)
        root[e, 2] += dz; feet[e, :, 2] += dz
        moved[e] = True
    env.set_field("root_states", torch.tensor(root, dtype=torch.float32))
    env.set_field("last_feet_pos", torch.tensor(feet.reshape(n, 6), dtype=torch.float32))
    env.common_step_counter = 7
    sp = StepParity(cfg, env, ref)
    sp.begin()
    x0 = ref.root[:, :2].copy()
    act = rng.uniform(-0.3, 0.3, (n, 12)).astype(np.float32)
    obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
    out = ref.step(act.astype(np.float64))
    shift = ref.root[:, :2] - x0
    big = np.abs(shift).max(axis=1) > 1.0
    assert (big == moved).all(), "the oracle teleported a different set of robots than the test placed"
    expect = {0: (ew + b, 0.0), 1: (-(ew + b), 0.0), 2: (0.0, el + b), 3: (0.0, -(el + b))}
    g_root = env.root_states.cpu().numpy()
    for e in range(16):
        assert np.allclose(g_root[e, :2] - x0[e], expect[e % 4], atol=0.05), (e, g_root[e, :2] - x0[e])
    keep = done.cpu().numpy() == out[3]
    assert keep[:16].all()
    for name, g, r in (("root", g_root, ref.root), ("last_feet_pos", env.get_field("last_feet_pos").cpu().numpy(), ref.last_feet.reshape(n, 6)),
                       ("obs", obs.cpu().numpy(), out[0]), ("privileged obs", extras["privileged_obs"].cpu().numpy(), out[1])):
        err = PU.rel_state(g[:16], r[:16])
        assert err.max() < (5e-3 if "obs" in name else 2e-3), f"teleported robots, {name}: {err}"
    sp.check(0, act, obs, rew, done, extras, out, teleported=moved)  # the other robots: the usual step parity


def test_body_contacts_collision_reward_and_contact_termination_match_oracle():
    """Non-foot collision shapes (trunk box, hip-yaw / shank cylinders): robots are dropped lying at random orientations with the height
    termination switched off, so that those shapes carry the load.  The `collision` reward term (number of penalised bodies with more than
    1 N, t1.py:627-629) and termination on contact (`terminate_contacts_on: [Trunk]`, t1.py:553) must agree with the oracle."""
    n = 128
    cfg, env, ref = _make("plane", n, {"rewards.terminate_height": -1.0, "rewards.terminate_contacts_on": ["Trunk"], "rewards.terminate_vel": 1.0e9})
    env.reset()
    rng = np.random.default_rng(21)
    root = env.root_states.cpu().numpy().astype(np.float64)
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0.5, 3.0, n)
    root[:, 2] = rng.uniform(0.08, 0.35, n)
    root[:, 3:6], root[:, 6] = ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)
    root[:, 7:] = 0.0
    env.set_field("root_states", torch.tensor(root, dtype=torch.float32))
    env.common_step_counter = 7
    # lying robots on explicit (non-implicit) sphere contacts are the stiffest states this build simulates: the same tolerances as for a walking
    # robot, the same rule (whatever is outside has to be explained), a little more room for explained cases
    sp = StepParity(cfg, env, ref, max_explained_frac=0.03)
    coll_seen, term_seen, flags_bad, coll_diff = 0, 0, 0, 0
    for s in range(4):
        sp.begin()
        act = rng.uniform(-0.3, 0.3, (n, 12)).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        out = ref.step(act.astype(np.float64))
        d_ref, terms_ref = out[3], out[5]
        keep = sp.check(s, act, obs, rew, done, extras, out)
        flags_bad += int((~keep).sum())
        coll_gpu, coll_ref = extras["rew_terms"]["collision"].cpu().numpy(), terms_ref["collision"]
        coll_diff += int((np.abs(coll_gpu - coll_ref)[keep] > 1e-6).sum())  # every one of these went through sp.check's explanation
        coll_seen += int((coll_ref < 0).sum()); term_seen += int(d_ref.sum())
    print("body-contact parity:", sp.finish(), "collision counts differing:", coll_diff, "termination flags differing:", flags_bad)
    assert coll_seen > n // 4 and term_seen > n // 10, (coll_seen, term_seen)  # the shapes were exercised
    assert flags_bad <= n * 4 * 2 // 100, flags_bad
    assert env.episode_stats(reset=False).cpu().numpy()[-1] == 0


def _cross_legs(env, n, rng):
    """Joint positions with the hip rolls turned inwards on both legs (ankle rolls compensating).  First half of the envs by 0.08 .. 0.16 rad:
    the feet between just apart and a few centimetres inside each other; second half by 0.22 .. 0.32 rad: legs crossed so far that the shanks
    meet as well.  Returns the action that asks the PD actuators for 0.12 rad MORE on each side, so that the legs keep pressing together."""
    q = env.dof_pos.cpu().numpy().astype(np.float64)
    roll = np.where(np.arange(n) < n // 2, rng.uniform(0.08, 0.16, n), rng.uniform(0.22, 0.32, n))
    yaw = rng.uniform(-0.2, 0.2, (n, 2))
    q[:, 1], q[:, 7] = -roll, roll
    q[:, 5], q[:, 11] = roll, -roll
    q[:, 2], q[:, 8] = yaw[:, 0], yaw[:, 1]
    env.set_field("dof_pos", torch.tensor(q, dtype=torch.float32))
    env.set_field("last_dof_targets", torch.tensor(q, dtype=torch.float32))
    act = np.zeros((n, 12), dtype=np.float32)
    act[:, 1], act[:, 7], act[:, 5], act[:, 11] = -(roll + 0.12), roll + 0.12, roll, -roll
    return act


@pytest.mark.parametrize("terrain", ["plane", "trimesh"])
def test_self_collision_step_matches_oracle(terrain):
    """Leg against leg (reference: PhysX self-collision enabled, envs/T1.yaml:69, envs/t1.py:128).  Standing robots get their legs crossed:
    hip rolls inwards until feet / shanks of the two legs overlap, and the actuators keep pulling them together.  One env step at a time from
    identical inputs against the float64 oracle, walking tolerances, every env outside them explained; the shank-against-shank contacts show
    up in the `collision` reward term (Shank is a penalised body, t1.py:627-629) exactly as in the oracle."""
    n = 96
    cfg, env, ref = _make(terrain, n)
    assert env._cfg_c.self_collisions == 1 and ref.dyn.phys.self_collisions == 1
    env.reset(); ref.reset()
    rng = np.random.default_rng(23)
    _settle(env, n, rng)
    act0 = _cross_legs(env, n, rng)
    env.common_step_counter = 7
    sp = StepParity(cfg, env, ref, max_explained_frac=0.03)
    contact_seen, coll_seen, coll_diff, flags_bad = 0, 0, 0, 0
    for s in range(5):
        sp.begin()
        act = (act0 + rng.uniform(-0.1, 0.1, (n, 12))).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        out = ref.step(act.astype(np.float64))
        keep = sp.check(s, act, obs, rew, done, extras, out)
        flags_bad += int((~keep).sum())
        for e in range(n):  # leg-against-leg forces in the state the step ended in
            contact_seen += int(np.abs(ref.dyn.self_contact_forces(ref.root[e], ref.q[e], ref.qd[e])).max() > 1.0)
        coll_gpu, coll_ref = extras["rew_terms"]["collision"].cpu().numpy(), out[5]["collision"]
        coll_seen += int((coll_ref < 0).sum())
        coll_diff += int((np.abs(coll_gpu - coll_ref)[keep] > 1e-6).sum())
    print("self-collision step parity:", sp.finish(), sp.log, "collision counts differing:", coll_diff, "flags differing:", flags_bad)
    assert contact_seen > n and coll_seen > 10, (contact_seen, coll_seen)  # leg-against-leg forces at the end of > 20 % of the env-steps; shank contacts penalised
    assert flags_bad <= 4, flags_bad
    assert env.episode_stats(reset=False).cpu().numpy()[-1] == 0


def test_self_collisions_off_lets_the_legs_pass_through_each_other():
    """asset.self_collisions != 0 (Isaac Gym's filter mask: the actor's shapes do not collide with each other) switches the contacts off on both
    sides: same crossed-leg start, still parity with the oracle, and the legs end up deeper inside each other than with the contacts on."""
    n = 64
    depth = {}
    for mask in (0, 1):
        cfg, env, ref = _make("plane", n, {"asset.self_collisions": mask})
        assert env._cfg_c.self_collisions == 1 - mask
        env.reset(); ref.reset()
        rng = np.random.default_rng(29)
        _settle(env, n, rng)
        act0 = _cross_legs(env, n, rng)
        env.common_step_counter = 7
        sp = StepParity(cfg, env, ref, max_explained_frac=0.03)
        for s in range(4):
            sp.begin()
            obs, rew, done, extras = env.step(torch.tensor(act0, device=env.device))
            out = ref.step(act0.astype(np.float64))
            sp.check(s, act0, obs, rew, done, extras, out)
        sp.finish()
        fp = env.get_field("feet_pos").cpu().numpy().reshape(n, 2, 3)
        depth[mask] = 0.1 - np.linalg.norm(fp[:, 0, :2] - fp[:, 1, :2], axis=1)  # overlap of the two foot capsules (radius 0.05) in plan view
    assert np.median(depth[1]) > np.median(depth[0]) + 0.02, (np.median(depth[0]), np.median(depth[1]))
    assert np.percentile(depth[0], 90) < 0.03, np.percentile(depth[0], 90)


@pytest.mark.parametrize("terrain", ["plane", "trimesh"])
def test_hip_step_deviates_from_the_float64_oracle_like_its_fp32_twin(terrain):
    """The product kernels are built with value-changing FP relaxations (-fassociative-math -freciprocal-math -ffinite-math-only, hardware rcp /
    sqrt).  Evidence that this is harmless, as an assertion: over 256 envs x 6 steps the HIP step's deviation from the float64 oracle is of
    the SAME SIZE as the deviation of the oracle's own single-precision build (libdynref32.so: the dense 6x6 algorithm with every double a
    float, IEEE arithmetic, no relaxations) from the same float64 result -- median and 99th percentile of the post-physics state within
    2.5 x the twin's, and no more envs beyond the tolerances than the twin has plus 0.5 %.  (The tool form of this, with the full
    distributions, is tools/parity_diag.py -> profiles/r02_parity_diag_*.json.)"""
    n = 256
    cfg, env, ref = _make(terrain, n)
    ref32 = _twin32(cfg, env, ref)
    env.reset()
    rng = np.random.default_rng(11)
    _settle(env, n, rng)
    env.common_step_counter = 7
    acc = {k: {"gpu": [], "twin": []} for k in ("root", "dof_pos", "dof_vel")}
    for s in range(6):
        PU.sync_oracle(env, ref); PU.sync_oracle(env, ref32)
        act = rng.uniform(-0.6, 0.6, (n, 12)).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        d = ref.step(act.astype(np.float64))[3]
        d2 = ref32.step(act.astype(np.float64))[3]
        keep = (done.cpu().numpy() == d) & (d2 == d)
        for k, (g, w, f) in {"root": (env.root_states.cpu().numpy(), ref32.root, ref.root), "dof_pos": (env.dof_pos.cpu().numpy(), ref32.q, ref.q),
                             "dof_vel": (env.dof_vel.cpu().numpy(), ref32.qd, ref.qd)}.items():
            acc[k]["gpu"].append(PU.rel_state(g, f)[keep]); acc[k]["twin"].append(PU.rel_state(w, f)[keep])
    for k, v in acc.items():
        g, w = np.concatenate(v["gpu"]), np.concatenate(v["twin"])
        tol = PU.STATE_TOL[k]
        print(f"{terrain} {k}: HIP p50 {np.median(g):.2e} p99 {np.quantile(g, 0.99):.2e} >tol {(g > tol).mean():.4f} | fp32 twin p50 {np.median(w):.2e} "
              f"p99 {np.quantile(w, 0.99):.2e} >tol {(w > tol).mean():.4f}")
        assert np.median(g) <= 2.5 * np.median(w) + 1e-7, (k, np.median(g), np.median(w))
        assert np.quantile(g, 0.99) <= 2.5 * np.quantile(w, 0.99) + 1e-6, (k, np.quantile(g, 0.99), np.quantile(w, 0.99))
        assert (g > tol).mean() <= (w > tol).mean() + 0.005, (k, (g > tol).mean(), (w > tol).mean())


FP16_FIELDS = ["dof_pos", "dof_vel", "last_dof_targets", "actions", "last_actions", "last_dof_vel", "last_root_vel", "commands", "gait_frequency",
               "gait_process", "filtered_lin_vel", "filtered_ang_vel", "pushing"]


def test_fp16_state_step_matches_oracle():
    """sim.state_dtype: fp16 (BASELINE configs[4]): the state the env keeps between steps is fp16-representable (root position and feet
    positions stay fp32), one env step from identical (fp16) inputs matches the float64 oracle whose stored state is rounded the same way,
    observations (computed before the state is rounded for storage) keep the fp32 tolerance."""
    n = 96
    cfg, env, ref = _make("trimesh", n, {"sim.state_dtype": "fp16"})
    env.reset()
    rng = np.random.default_rng(5)
    for _ in range(15):
        env.step(torch.tensor(rng.uniform(-0.3, 0.3, (n, 12)), dtype=torch.float32, device=env.device))
    env.common_step_counter = 246  # push drawn inside the window
    is_h = lambda a: np.array_equal(a, a.astype(np.float16).astype(np.float32))
    # stored state: dynamics tolerance + one fp16 ulp (2^-10 relative) where the two sides round a near-tie differently
    sp = StepParity(cfg, env, ref, state_tol={"root": 3e-3, "dof_pos": 3e-3, "dof_vel": 1e-2})
    for s in range(6):
        sp.begin()
        for k in FP16_FIELDS:
            assert is_h(env.get_field(k).cpu().numpy()), k
        root = env.root_states.cpu().numpy()
        assert is_h(root[:, 3:]) and not is_h(root[:, :3])
        assert not is_h(env.get_field("last_feet_pos").cpu().numpy()) and not is_h(env.get_field("dof_stiffness").cpu().numpy())
        kicked = _kick_step(cfg, env)
        act = rng.uniform(-0.6, 0.6, (n, 12)).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        out = ref.step(act.astype(np.float64))
        ref.quantize_state_fp16()
        keep = sp.check(s, act, obs, rew, done, extras, out, kicked=kicked)
        assert keep.mean() > 0.97
        assert PU.rel_state(env.get_field("last_dof_targets").cpu().numpy()[keep], ref.last_tgt[keep]).max() < 2e-3, f"step {s} targets"
        assert PU.rel_state(env.get_field("pushing").cpu().numpy(), ref.push).max() < 2e-3, f"step {s} push"
    print("fp16-state parity:", sp.finish())
    assert env.episode_stats(reset=False).cpu().numpy()[-1] == 0


def test_command_curriculum_matches_oracle():
    """commands.curriculum = true (t1.py:391-435): grid update on successful episodes, multinomial resampling, level bookkeeping."""
    n = 96
    cfg, env, ref = _make("plane", n, {"commands.curriculum": True})
    env.reset(); ref.reset()
    rng = np.random.default_rng(3)
    for _ in range(12):
        env.step(torch.tensor(rng.uniform(-0.3, 0.3, (n, 12)), dtype=torch.float32, device=env.device))
    # a non-trivial grid, levels for every env, and a batch of envs that end a SUCCESSFUL long episode in the window
    prob0 = rng.uniform(0.0, 0.8, (21, 21)).astype(np.float32); prob0[10, 10] = 1.0
    env.curriculum_prob = torch.tensor(prob0)
    ref.curr_prob = prob0.astype(np.float64); ref.curr_prob_read = ref.curr_prob.copy()
    lin0, ang0 = rng.integers(-10, 11, n), rng.integers(-10, 11, n)
    env.set_field("env_curriculum_level_lin", torch.tensor(lin0, dtype=torch.int32)); env.set_field("env_curriculum_level_ang", torch.tensor(ang0, dtype=torch.int32))
    ep = env.get_field("episode_length_buf"); ep[:24, 0] = 1499; env.set_field("episode_length_buf", ep)
    ct = env.get_field("cmd_resample_time"); ct[:24, 0] = 9000; ct[24:40, 0] = ep[24:40, 0] + 2; env.set_field("cmd_resample_time", ct)
    cmd = env.get_field("commands"); filt_l = env.get_field("filtered_lin_vel"); filt_a = env.get_field("filtered_ang_vel")
    cmd[:24] = 0.0; filt_l[:12] = 0.0; filt_a[:12] = 0.0  # 12 successes (tracking error 0), 12 probable failures
    filt_l[12:24, 0] = 1.0
    env.set_field("commands", cmd); env.set_field("filtered_lin_vel", filt_l); env.set_field("filtered_ang_vel", filt_a)
    changed = False
    for s in range(4):
        _sync_oracle(env, ref)
        ref.curr_levels[:, 0] = env.get_field("env_curriculum_level_lin").cpu().numpy()[:, 0]
        ref.curr_levels[:, 1] = env.get_field("env_curriculum_level_ang").cpu().numpy()[:, 0]
        act = rng.uniform(-0.3, 0.3, (n, 12)).astype(np.float32)
        obs, rew, done, extras = env.step(torch.tensor(act, device=env.device))
        o_ref, p_ref, r_ref, d_ref, t_ref, terms_ref, derived = ref.step(act.astype(np.float64))
        keep = done.cpu().numpy() == d_ref
        assert keep.mean() > 0.97
        got = env.curriculum_prob.cpu().numpy()
        assert np.allclose(got, np.minimum(ref.curr_prob, 1.0), atol=1e-5), f"step {s}: grid differs"
        changed = changed or np.abs(got - prob0).max() > 0.05
        assert (env.get_field("env_curriculum_level_lin").cpu().numpy()[:, 0][keep] == ref.curr_levels[keep, 0]).all()
        assert (env.get_field("env_curriculum_level_ang").cpu().numpy()[:, 0][keep] == ref.curr_levels[keep, 1]).all()
        assert PU.rel_state(env.commands.cpu().numpy()[keep], ref.cmd[keep]).max() < 1e-5, f"step {s} curriculum commands"
    assert changed, "no successful episode updated the grid"
    env.refresh_curriculum_levels()
    assert env.max_lin_vel_level >= 1.0 and 0.0 < env.mean_ang_vel_level <= 10.0


def test_trained_reference_policy_walks_on_the_gpu():
    """Closed loop on the GPU with the one artefact of the reference that embeds its physics: the actor it trained in PhysX (deploy/models/T1.pt,
    weights only) drives 1,024 robots for 500 env steps (10 s) under the SHIPPED T1.yaml -- observation noise, domain randomisation, latency, kicks,
    pushes, resampled commands.  The bounds are the values measured at 4,096 robots over a full episode (profiles/r04_reference_actor_eval.json,
    tools/eval_reference_actor.py) with a stated margin: 2.0 % of the robots fall within 500 steps there (1.1 % in the first 100, then 0.2 % per 100
    steps), tracking RMSE 0.205 / 0.241 m/s and 0.193 rad/s against moving commands, 0.11 / 0.08 / 0.12 against a standing command.  Margins: fall rate
    + 4.5 sigma of a 1,024-robot sample, RMSE + 25 %."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from eval_reference_actor import evaluate

    r = evaluate(1024, 500, {"terrain.type": "plane"})
    assert r["fell_within_steps"]["500"] < 0.04, r["fell_within_steps"]
    assert r["fell_within_steps"]["100"] < 0.03, r["fell_within_steps"]
    t, t0 = r["tracking_rmse"], r["tracking_rmse_still"]
    assert t["lin_vel_x"] < 0.26 and t["lin_vel_y"] < 0.30 and t["ang_vel_yaw"] < 0.245, t
    assert t0["lin_vel_x"] < 0.15 and t0["lin_vel_y"] < 0.11 and t0["ang_vel_yaw"] < 0.16, t0
    # the tracking rewards the reference's own reward function pays this policy here: 0.9 of their maximum (scale x dt = 0.02 / 0.02 / 0.01 per step)
    rt = r["reward_terms"]
    assert rt["tracking_lin_vel_x"] > 0.8 * 0.02 and rt["tracking_lin_vel_y"] > 0.8 * 0.02 and rt["tracking_ang_vel"] > 0.8 * 0.01, rt
    assert r["nonfinite_resets"] == 0


def test_stale_time_outs_flag_reproduces_the_reference_binding():
    """parallel.stale_time_outs (SURVEY Q3, t1.py:317 vs :556-558): on a step without any reset the reference's runner reads the time-out flags of
    the LAST step that had a reset.  Two envs with the same seed, flag off / on, stepped with the same actions: same flags whenever an env was
    reset in the step, the remembered ones otherwise."""
    n = 64
    cfg0, env0, _ = _make("plane", n)
    cfg1, env1, _ = _make("plane", n, {"parallel.stale_time_outs": True})
    env0.reset(); env1.reset()
    ct = env0.get_field("cmd_resample_time"); ct[:, 0] = 5000; ct[3, 0] = 4; ct[9, 0] = 7  # resample steps: time_outs without a reset
    env0.set_field("cmd_resample_time", ct); env1.set_field("cmd_resample_time", ct.clone())
    ep = env0.get_field("episode_length_buf"); ep[20, 0] = 1495
    env0.set_field("episode_length_buf", ep); env1.set_field("episode_length_buf", ep.clone())
    rng = np.random.default_rng(2)
    remembered = torch.zeros(n, dtype=torch.bool, device=env0.device)  # reset(): _reset_idx(all) bound the initial buffer
    seen_stale, seen_fresh = 0, 0
    for s in range(10):
        a = torch.tensor(rng.uniform(-0.2, 0.2, (n, 12)), dtype=torch.float32, device=env0.device)
        _, _, d0, x0 = env0.step(a)
        _, _, d1, x1 = env1.step(a)
        assert torch.equal(d0, d1)
        fresh = x0["time_outs"].clone()
        if bool(d0.any()):
            remembered = fresh
            assert torch.equal(x1["time_outs"], fresh); seen_fresh += 1
        else:
            assert torch.equal(x1["time_outs"], remembered)
            seen_stale += int(not torch.equal(fresh, remembered))
    assert seen_fresh >= 1 and seen_stale >= 1, (seen_fresh, seen_stale)  # both branches exercised, and the stale value really differed


def test_mirrored_rollout_stays_mirrored(flat_model, tmp_path):
    """The fused env-step kernel (10 substeps of dynamics + PD actuators + task logic per launch) on a SYMMETRISED copy of the model (conftest.symmetrised),
    every randomisation, noise, kick and push off: mirrored standing states driven by mirrored actions stay mirrored over a rollout -- root on the sagittal
    plane, no roll / yaw, right-leg joints = MIRROR_SIGN x left, mirrored foot forces, mirrored observation and torque rows.  (SURVEY section 8c KAT (5),
    applied to the shipping kernel through bg_env_step: an independent physical identity, not a comparison with this build's own oracle.)  fp32 sums in
    mirrored order differ in the last bits and stiff sole contacts amplify that from step to step: measured <= 5e-6 after 4 control steps (40 substeps),
    bound 1e-4."""
    from conftest import MIRROR_SIGN, mirrored_states, symmetrised

    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    n = 128
    path = tmp_path / "T1_symmetrised.flat.json"
    symmetrised(flat_model).save(str(path))
    off = {f"randomization.{k}": None for k in ("init_dof_pos", "init_base_pos_xy", "init_base_lin_vel_xy", "kick_lin_vel", "kick_ang_vel", "push_force", "push_torque",
                                                "dof_stiffness", "dof_damping", "dof_friction", "friction", "compliance", "restitution", "base_com", "base_mass",
                                                "other_com", "other_mass")}
    off.update({f"noise.{k}": None for k in ("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel", "height")})
    cfg = load_cfg("T1", dict({"env.num_envs": n, "terrain.type": "plane", "asset.file": str(path)}, **off))
    env = T1(cfg)
    env.reset()
    rng = np.random.default_rng(21)
    root, q, qd, _ = mirrored_states(rng, n, True, z_range=(0.695, 0.72))  # (soles up to 2.5 cm into the ground: deeper starts launch the robot)
    root[:, :2] = env.get_field("root_states").cpu().numpy()[:, :2]  # keep every robot on its own origin
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=env.device)
    env.set_field("root_states", f(root)); env.set_field("dof_pos", f(q)); env.set_field("dof_vel", f(qd))
    env.set_field("last_dof_vel", f(qd))
    cmd = env.get_field("commands"); cmd[:, 1:] = 0.0  # no lateral / yaw command (it only enters observations and rewards)
    env.set_field("commands", cmd)
    S, my = np.array(MIRROR_SIGN), np.array([1.0, -1.0, 1.0])
    y0 = root[:, 1].copy()
    worst, keep = {}, np.ones(n, dtype=bool)
    for step in range(4):
        aL = rng.uniform(-0.2, 0.2, (n, 6))  # (gentle: +-0.5 rad of random target jumps throws some robots over within two steps)
        obs, rew, done, extras = env.step(f(np.concatenate([aL, S * aL], axis=1)))
        keep &= ~done.cpu().numpy().astype(bool)  # a robot that was reset has left its mirrored state
        r = env.get_field("root_states").cpu().numpy().astype(np.float64)[keep]
        qn, qdn = env.get_field("dof_pos").cpu().numpy().astype(np.float64)[keep], env.get_field("dof_vel").cpu().numpy().astype(np.float64)[keep]
        cf = env.get_field("feet_contact_forces").cpu().numpy().reshape(n, 2, 3).astype(np.float64)[keep]
        tq = env.get_field("torques").cpu().numpy().astype(np.float64)[keep]
        o = obs.cpu().numpy().astype(np.float64)[keep]
        m = {"root_y": np.abs(r[:, 1] - y0[keep]).max(), "quat_xz": np.abs(r[:, [3, 5]]).max(), "vel_y": np.abs(r[:, 8]).max(), "ang_vel_xz": np.abs(r[:, [10, 12]]).max(),
             "dof_pos": np.abs(qn[:, 6:] - S * qn[:, :6]).max(), "dof_vel": np.abs(qdn[:, 6:] - S * qdn[:, :6]).max() / max(1.0, np.abs(qdn).max()),
             "torques": np.abs(tq[:, 6:] - S * tq[:, :6]).max() / max(1.0, np.abs(tq).max()),
             "feet_forces": np.abs(cf[:, 1] - cf[:, 0] * my).max() / max(1.0, np.abs(cf).max()),
             # observation row (envs/t1.py:574-603): the 12 joint positions / velocities / last actions sit in the last 36 entries
             "obs_joints": max(np.abs(o[:, 11 + 12 * k + 6 : 11 + 12 * k + 12] - S * o[:, 11 + 12 * k : 11 + 12 * k + 6]).max() for k in range(3))}
        for k, v in m.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    assert keep.sum() >= 0.9 * n, f"only {int(keep.sum())} of {n} robots stayed up"
    print("mirrored rollout, worst asymmetry over 4 control steps:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert float(np.abs(cf).max()) > 50.0, "the robots are not standing on their soles"
    for k, v in worst.items():
        assert v < 1e-4, (k, v)
