"""CPU tests of the mirror-symmetry loss (algorithm.symmetry_loss): the mirror maps against the task logic, the config key, the plan."""
import types

import numpy as np
import pytest
import torch

from conftest import MIRROR_SIGN


def _default_pose(cfg, names):
    dja = cfg["init_state"]["default_joint_angles"]
    return np.array([([v for k, v in dja.items() if k != "default" and k in n] or [dja["default"]])[-1] for n in names], dtype=np.float32)


def _maps(flat_model):
    from booster_gym_amd.envs.mirror import mirror_maps
    from booster_gym_amd.utils.config import load_cfg

    axes = [int(a) for a in flat_model.joint_axis if int(a) != 0]
    return mirror_maps(flat_model.dof_names, axes, _default_pose(load_cfg("T1", {}), flat_model.dof_names), 47)


def test_mirror_maps_are_signed_permutation_involutions_with_the_expected_entries(flat_model):
    from booster_gym_amd.envs.mirror import signed_permutation

    obs_src, obs_sign, act_src, act_sign = _maps(flat_model)
    Mo, Ma = signed_permutation(obs_src, obs_sign), signed_permutation(act_src, act_sign)
    for M, n in ((Mo, 47), (Ma, 12)):
        assert M.shape == (n, n)
        assert np.array_equal(np.abs(M).sum(0), np.ones(n)) and np.array_equal(np.abs(M).sum(1), np.ones(n))  # a signed permutation
        assert np.array_equal(M @ M, np.eye(n))  # an involution
        assert np.array_equal(M, M.T)  # symmetric
    # gravity (x, -y, z), angular velocity (-x, y, -z), commands (vx, -vy, -yaw), gait clock (-cos, -sin)
    assert np.array_equal(np.diag(Mo)[:11], [1, -1, 1, -1, 1, -1, 1, -1, -1, -1, -1])
    names = flat_model.dof_names
    for j, n in enumerate(names):
        other = n.replace("Left", "Right") if n.startswith("Left") else n.replace("Right", "Left")
        assert names[act_src[j]] == other
    assert tuple(act_sign[:6]) == MIRROR_SIGN and tuple(act_sign[6:]) == MIRROR_SIGN
    for blk in (11, 23, 35):  # dof_pos - default, dof_vel, last actions
        assert np.array_equal(Mo[blk : blk + 12, blk : blk + 12], Ma)


def _mirror_state(s):
    """The mirror image of a state in the sagittal plane (y -> -y): root position, quaternion, velocities, joints left <-> right with
    MIRROR_SIGN, gait phase + 0.5, commands (vx, -vy, -yaw), last actions."""
    S = np.array(MIRROR_SIGN * 2)
    perm = np.r_[6:12, 0:6]
    m = {k: v.copy() for k, v in s.items()}
    m["root_pos"] = s["root_pos"] * [1, -1, 1]
    m["quat"] = s["quat"] * [-1, 1, -1, 1]  # (x, y, z, w): a rotation about axis (ax, ay, az) by th becomes one about (-ax, ay, -az) by -th
    m["lin_vel"] = s["lin_vel"] * [1, -1, 1]
    m["ang_vel"] = s["ang_vel"] * [-1, 1, -1]  # a pseudo-vector
    for k in ("dof_pos", "dof_vel", "actions"):
        m[k] = s[k][:, perm] * S
    m["gait_process"] = np.fmod(s["gait_process"] + 0.5, 1.0)
    m["commands"] = s["commands"] * [1, -1, -1]
    return m


def _observations(s, cfg, default):
    import oracle.task_ref as tr

    nz = cfg["normalization"]
    norm = dict(gravity=nz["gravity"], lin_vel=nz["lin_vel"], ang_vel=nz["ang_vel"], dof_pos=nz["dof_pos"], dof_vel=nz["dof_vel"], push_force=0.1, push_torque=0.5)
    K = len(s["quat"])
    st = dict(projected_gravity=tr.quat_rotate_inverse(s["quat"], np.tile([0.0, 0.0, -1.0], (K, 1))), base_ang_vel=tr.quat_rotate_inverse(s["quat"], s["ang_vel"]),
              commands=s["commands"], gait_frequency=s["gait_frequency"], gait_process=s["gait_process"], dof_pos=s["dof_pos"], dof_vel=s["dof_vel"],
              actions=s["actions"], root_states=np.concatenate([s["root_pos"], s["quat"], s["lin_vel"], s["ang_vel"]], axis=1),
              base_mass_scaled=np.zeros((K, 4)), base_lin_vel=tr.quat_rotate_inverse(s["quat"], s["lin_vel"]), push_force=np.zeros((K, 3)),
              push_torque=np.zeros((K, 3)))
    return tr.compute_observations(st, norm, default, None)[0]


def test_mirror_maps_agree_with_the_task_logic(flat_model):
    """oracle.task_ref.compute_observations(mirror(s)) == M_o compute_observations(s) on random states, to float64 rounding."""
    from booster_gym_amd.envs.mirror import signed_permutation
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", {})
    default = _default_pose(cfg, flat_model.dof_names).astype(np.float64)
    rng = np.random.default_rng(5)
    K = 500
    q = rng.normal(size=(K, 4))
    S = np.array(MIRROR_SIGN * 2)
    s = dict(root_pos=rng.normal(size=(K, 3)), quat=q / np.linalg.norm(q, axis=1, keepdims=True), lin_vel=rng.normal(size=(K, 3)), ang_vel=rng.normal(size=(K, 3)),
             dof_pos=default + rng.normal(size=(K, 12)) * 0.3, dof_vel=rng.normal(size=(K, 12)) * 3, actions=rng.normal(size=(K, 12)),
             gait_process=rng.uniform(0, 1, K), gait_frequency=np.where(rng.uniform(size=K) < 0.2, 0.0, rng.uniform(1, 2, K)), commands=rng.normal(size=(K, 3)))
    assert np.array_equal(default[np.r_[6:12, 0:6]] * S, default)  # the default pose is its own mirror image
    obs_src, obs_sign, _, _ = _maps(flat_model)
    Mo = signed_permutation(obs_src, obs_sign)
    o, om = _observations(s, cfg, default), _observations(_mirror_state(s), cfg, default)
    np.testing.assert_allclose(om, o @ Mo.T, rtol=0, atol=1e-12)
    assert np.abs(om - o).max() > 0.1  # (the states are not their own mirror images)


def test_models_without_a_mirror_pairing_are_rejected(flat_model):
    from booster_gym_amd.envs.mirror import mirror_maps

    axes = [int(a) for a in flat_model.joint_axis if int(a) != 0]
    pose = np.array([-0.2, 0, 0, 0.4, -0.25, 0] * 2)
    with pytest.raises(ValueError, match="no Left_"):
        mirror_maps([f"Joint_{k}" for k in range(12)], axes, np.zeros(12), 47)
    with pytest.raises(ValueError, match="no mirror partner"):
        mirror_maps(flat_model.dof_names[:6] + [n.replace("Right", "Rear") for n in flat_model.dof_names[6:]], axes, pose, 47)
    with pytest.raises(ValueError, match="same x / y / z axis"):
        mirror_maps(flat_model.dof_names, axes[:6] + [2] * 6, pose, 47)
    with pytest.raises(ValueError, match="default joint pose"):
        mirror_maps(flat_model.dof_names, axes, np.r_[pose[:6], pose[:6] + 0.1], 47)
    with pytest.raises(ValueError, match="layout"):
        mirror_maps(flat_model.dof_names, axes, pose, 48)


def test_config_key_default_and_absent_mean_off():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import symmetry_loss

    cfg = load_cfg("T1", {})
    assert cfg["algorithm"]["symmetry_loss"] is False and cfg["algorithm"]["symmetric_coef"] == 10.0
    assert symmetry_loss(cfg) == (False, 0.0)
    del cfg["algorithm"]["symmetry_loss"]
    assert symmetry_loss(cfg) == (False, 0.0)
    assert symmetry_loss(load_cfg("T1", {"algorithm.symmetry_loss": True})) == (True, 10.0)
    assert symmetry_loss(load_cfg("T1", {"algorithm.symmetry_loss": True, "algorithm.symmetric_coef": 0})) == (True, 0.0)
    for bad in ({"algorithm.symmetry_loss": "yes"}, {"algorithm.symmetry_loss": 1}, {"algorithm.symmetry_loss": True, "algorithm.symmetric_coef": -1.0},
                {"algorithm.symmetry_loss": True, "algorithm.symmetric_coef": float("nan")}):
        with pytest.raises(ValueError):
            symmetry_loss(load_cfg("T1", bad))


SW = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
          defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
CRITIC, ACTOR = ((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64)


def test_plan_reflects_the_doubled_actor_rows_and_turns_the_forward_ahead_off():
    from booster_gym_amd.utils.runner import plan_update

    off = plan_update(CRITIC, ACTOR, 24 * 4096, **SW)
    on = plan_update(CRITIC, ACTOR, 24 * 4096, symmetry=True, **SW)
    assert plan_update(CRITIC, ACTOR, 24 * 4096, symmetry=False, **SW) == off and not off.symmetry  # the default plan is unchanged
    assert off.ahead and not on.ahead and on.symmetry
    assert on._replace(ahead=True, symmetry=False) == off  # every kernel form stays the default's
    assert plan_update(CRITIC, ACTOR, 24 * 4096, symmetry=True, **SW) == on  # pure
    # the actor's passes differentiate 2B rows: at B = 40 the grouped weight-gradient launch takes the actor's layers (80 >= 64 rows), not the critic's
    small = plan_update(CRITIC, ACTOR, 40, symmetry=True, **SW)
    assert all(small.actor.grouped[:-1]) and not any(small.critic.grouped)  # (the 12-wide output layer is never in the grouped launch)
    assert not any(plan_update(CRITIC, ACTOR, 40, **SW).actor.grouped)
    with pytest.raises(ValueError, match="fused output layers"):
        plan_update(CRITIC, ACTOR, 24 * 4096, symmetry=True, **dict(SW, fused_head=False))


def test_cu_shares_follow_the_doubled_actor_slabs(monkeypatch):
    """Runner._plan_chain_split with the actor's 2B input rows: the forward launch splits 800 critic slabs against 1,536 actor slabs, the backward launch
    768 critic slabs (the batch) against 1,536."""
    from booster_gym_amd.utils.model import ActorCritic, MLPTrainer
    from booster_gym_amd.utils.runner import Runner, plan_chain_split, plan_update

    for k in ("BG_FWD_CHAIN_CUS", "BG_BWD_CHAIN_CUS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=256))
    m = ActorCritic(12, 47, 14)
    r = Runner.__new__(Runner)
    r._critic_tr, r._actor_tr, r.device = MLPTrainer(m.critic), MLPTrainer(m.actor), "cpu"
    r._split_chain_cus = r._split_bwd_chain_cus = True
    plan = plan_update(CRITIC, ACTOR, 24 * 4096, symmetry=True, **SW)
    r._plan_chain_split(torch.empty(25 * 4096, 64, device="meta"), torch.empty(2 * 24 * 4096, 64, device="meta"), plan)
    fc, fa = 64 * 256 + 256 * 256 + 256 * 128, 64 * 256 + 256 * 128 + 128 * 128
    bc, ba = 256 * 256 + 128 * 256, 128 * 256 + 128 * 128
    fwd = (r._critic_tr.chain_workgroups, r._actor_tr.chain_workgroups)
    assert fwd == plan_chain_split(800, 1536, fc, fa, 256) and fwd != plan_chain_split(800, 768, fc, fa, 256)
    assert fwd[1] > 96  # the actor's share grows with its slabs (96 of 256 CUs without the loss)
    assert (r._critic_tr.chain_bwd_workgroups, r._actor_tr.chain_bwd_workgroups) == plan_chain_split(768, 1536, bc, ba, 256)
