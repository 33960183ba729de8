"""The actor's terrain height scan (terrain.actor_heights) without a GPU: the config rules, the key-absent behaviour, the scan block of the mirror map
against a numpy restatement of the scan at mirrored poses on a mirrored field, the update plan of a 234-input actor, the C ABI's argument check, and
the host-side row of tools/play_oracle.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 187
GRID_9x5 = {"terrain.measured_points_x": [round(-0.4 + 0.1 * i, 1) for i in range(9)], "terrain.measured_points_y": [-0.2, -0.1, 0.0, 0.1, 0.2]}


def _cfg(H=1, points=P, num_obs=None, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.frame_stack": H, "env.num_privileged_obs": 14 + points,
          "env.num_observations": 47 * H + points if num_obs is None else num_obs}
    ov.update(over)
    return load_cfg("T1", ov)


def test_config_rules_name_their_keys():
    from booster_gym_amd.envs.t1 import check_env_sizes
    from booster_gym_amd.utils.terrain import Terrain, actor_heights_of, height_scan_points

    cfg = _cfg()
    assert actor_heights_of(cfg["terrain"]) and len(height_scan_points(cfg["terrain"])[1]) == P
    check_env_sizes(cfg, P)  # 234 observations, 201 privileged: the critic takes 435
    check_env_sizes(_cfg(3, 45, **GRID_9x5), 45)  # 141 + 45 = 186; critic 186 + 59 = 245
    # the key on without the critic's scan: both keys named, before anything is built
    bad = _cfg(**{"terrain.measure_heights": False})
    with pytest.raises(ValueError, match=r"terrain\.actor_heights.*terrain\.measure_heights"):
        actor_heights_of(bad["terrain"])
    with pytest.raises(ValueError, match=r"terrain\.actor_heights.*terrain\.measure_heights"):
        Terrain("cpu", bad["terrain"])
    # num_observations: the number it should be
    with pytest.raises(ValueError, match=r"env\.num_observations = 47.*terrain\.actor_heights.*env\.num_observations to 234"):
        check_env_sizes(_cfg(num_obs=47), P)
    with pytest.raises(ValueError, match=r"env\.num_observations to 328"):
        check_env_sizes(_cfg(3, num_obs=141), P)
    with pytest.raises(ValueError, match=r"env\.num_privileged_obs to 201"):
        check_env_sizes(_cfg(**{"env.num_privileged_obs": 14}), P)
    # the critic's input 47 H + P + 14 + P above 512: H = 3 with the default grid is 141 + 187 + 14 + 187 = 529
    with pytest.raises(ValueError, match=r"env\.frame_stack.*measured_points_x.*measured_points_y.* = 529 exceeds 512"):
        check_env_sizes(_cfg(3), P)
    check_env_sizes(_cfg(2), P)  # 94 + 187 + 201 = 482


def test_key_absent_or_false_is_todays_config():
    from booster_gym_amd.envs.t1 import check_env_sizes
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.terrain import Terrain, actor_heights_of

    cfg = load_cfg("T1")
    assert cfg["terrain"]["actor_heights"] is False  # (the shipped yaml names the key, at its default)
    assert cfg["noise"]["height_measurements"] == {"range": [-0.1, 0.1], "operation": "additive", "distribution": "uniform"}
    assert cfg["noise"]["height"] == {"range": [0.0, 0.02], "operation": "additive", "distribution": "gaussian"}
    assert (cfg["env"]["num_observations"], cfg["env"]["num_privileged_obs"]) == (47, 14)
    for absent in (False, True):
        cfg = load_cfg("T1")
        if absent:
            del cfg["terrain"]["actor_heights"], cfg["noise"]["height_measurements"]
        assert not actor_heights_of(cfg["terrain"])
        check_env_sizes(cfg, 0)
        with pytest.raises(ValueError, match="47 observations"):
            check_env_sizes(load_cfg("T1", {"env.num_observations": 234}), 0)
        scan = load_cfg("T1", {"terrain.measure_heights": True, "env.num_privileged_obs": 201})
        if absent:
            del scan["terrain"]["actor_heights"]
        check_env_sizes(scan, P)  # the critic-only scan keeps the actor's 47
        assert not Terrain("cpu", scan["terrain"]).actor_heights


# ------------------------------------------------------------------ the mirror map
def _scan_f64(pose, pts, hf, border_px, hscale, vscale, target, S):
    """tests/test_gpu_height_scan.py's _scan_ref for one pose (x, y, z, yaw) on a height field, float64."""
    x, y, z, yaw = pose
    c, s = np.cos(yaw), np.sin(yaw)
    wx = x + c * pts[:, 0] - s * pts[:, 1]
    wy = y + s * pts[:, 0] + c * pts[:, 1]
    px, py = border_px + wx / hscale, border_px + wy / hscale
    x1 = np.clip(np.floor(px).astype(np.int64), 0, hf.shape[0] - 2)
    y1 = np.clip(np.floor(py).astype(np.int64), 0, hf.shape[1] - 2)
    fx, fy = px - x1, py - y1
    h = ((1 - fx) * (1 - fy) * hf[x1, y1] + fx * (1 - fy) * hf[x1 + 1, y1] + (1 - fx) * fy * hf[x1, y1 + 1] + fx * fy * hf[x1 + 1, y1 + 1]) * vscale
    return np.clip(z - h - target, -1.0, 1.0) * S


@pytest.mark.parametrize("H", [1, 3])
def test_mirror_map_is_a_signed_permutation_an_involution_and_mirrors_the_scan(flat_model, H):
    from booster_gym_amd.envs.mirror import mirror_maps, signed_permutation
    from booster_gym_amd.utils.terrain import height_scan_points

    cfg = _cfg()
    pts = height_scan_points(cfg["terrain"])[1]
    axes = [int(a) for a in flat_model.joint_axis if int(a) != 0]
    q0 = np.zeros(12)
    F, W = 47 * H, 47 * H + P
    src, sign, act_src, act_sign = mirror_maps(flat_model.dof_names, axes, q0, W, H, pts)
    src0, sign0, a0, s0 = mirror_maps(flat_model.dof_names, axes, q0, F, H)
    assert src.shape == sign.shape == (W,) and src.dtype == np.int32
    assert np.array_equal(act_src, a0) and np.array_equal(act_sign, s0)
    assert np.array_equal(src[:F], src0) and np.array_equal(sign[:F], sign0)  # the frame blocks tile as without the scan
    M = signed_permutation(src, sign)
    assert np.array_equal(np.abs(M).sum(0), np.ones(W)) and np.array_equal(np.abs(M).sum(1), np.ones(W)) and set(np.unique(M)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(M @ M, np.eye(W))
    assert np.all(sign[F:] == 1.0) and src[F:].min() >= F
    # point (x_i, y_j) takes the value of (x_i, -y_j)
    p64 = pts.astype(np.float64)
    assert np.array_equal(p64[src[F:] - F, 0], p64[:, 0]) and np.array_equal(p64[src[F:] - F, 1], -p64[:, 1])
    # the scan at a pose on a field, mirrored by the map's scan block, is the scan at the y-mirrored pose on the y-mirrored field.  The field is
    # mirrored about the world line y = 0: pixel column j holds y = (j - border) * hscale, so the mirrored field has column j' = 2 border - j
    rng = np.random.default_rng(5)
    border, hscale, vscale = 40, 0.1, 0.005
    hf = rng.integers(-60, 60, size=(120, 81)).astype(np.float64)  # columns 0 .. 80 = y in [-4, 4]: symmetric about column 40
    hf_m = hf[:, ::-1].copy()
    Ms = M[F:, F:]
    for _ in range(20):
        pose = (rng.uniform(1.0, 6.0), rng.uniform(-1.5, 1.5), rng.uniform(0.3, 1.2), rng.uniform(-np.pi, np.pi))
        a = _scan_f64(pose, p64, hf, border, hscale, vscale, 0.68, 5.0)
        b = _scan_f64((pose[0], -pose[1], pose[2], -pose[3]), p64, hf_m, border, hscale, vscale, 0.68, 5.0)
        assert np.ptp(a) > 0.1  # (the field is seen: not a constant row)
        assert np.abs(Ms @ a - b).max() < 1e-12


def test_asymmetric_y_grid_with_the_symmetry_loss_is_a_value_error(flat_model):
    from booster_gym_amd.envs.mirror import mirror_maps
    from booster_gym_amd.utils.terrain import height_scan_points

    cfg = _cfg(points=3 * 4, **{"terrain.measured_points_x": [-0.1, 0.0, 0.1], "terrain.measured_points_y": [-0.2, -0.1, 0.0, 0.1]})
    pts = height_scan_points(cfg["terrain"])[1]
    axes = [int(a) for a in flat_model.joint_axis if int(a) != 0]
    with pytest.raises(ValueError, match=r"algorithm\.symmetry_loss.*terrain\.actor_heights.*terrain\.measured_points_y"):
        mirror_maps(flat_model.dof_names, axes, np.zeros(12), 47 + 12, 1, pts)


def test_plan_of_a_perceptive_actor_is_the_per_layer_plan():
    """234 inputs pad to 256 columns: per-layer forward and backward kernels, the grouped weight gradients, the fused heads, no forward-ahead -- as
    with a frame stack (tests/test_frame_stack.py); the critic's 435 pad to 512."""
    from booster_gym_amd.utils.runner import pad_input, plan_update

    assert pad_input(234) == 256 and pad_input(234 + 201) == 512 and pad_input(141 + 45) == 256
    sw = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
              defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
    plan = plan_update(((435, 256, 256, 128, 1), 512), ((234, 256, 128, 128, 12), 256), 24 * 4096, **sw)
    assert plan.actor.fwd == "layer" and plan.actor.bwd == "layer" and all(plan.actor.grouped[:-1])
    assert plan.critic.fwd == "layer" and plan.critic.bwd == "layer" and all(plan.critic.grouped[:-1])
    assert not plan.ahead and plan.fused_head and not plan.chain_values


def test_env_create_rejects_actor_heights_without_scan_points_without_gpu(flat_model):
    """bg_env_create checks cfg.actor_heights before it touches the device; the two new fields lie behind frame_stack, so every older offset stays."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    assert _lib.EnvCfg.actor_heights.offset == _lib.EnvCfg.frame_stack.offset + 4
    assert _lib.EnvCfg.noise_height_measurements.offset == _lib.EnvCfg.actor_heights.offset + 4
    assert _lib.EnvCfg.noise_height_measurements.offset + C.sizeof(_lib.Rand) <= C.sizeof(_lib.EnvCfg)
    m = flat_model
    desc = _lib.ModelDesc(); desc.num_bodies, desc.num_dofs = 13, 12
    for b in range(13):
        desc.parent[b], desc.joint_axis[b], desc.mass[b] = int(m.parent[b]), int(m.joint_axis[b]), float(m.mass[b])
    model = C.c_void_p()
    assert lib.bg_model_create(C.byref(desc), C.byref(model)) == 0
    try:
        cfg = _lib.EnvCfg(); cfg.num_envs, cfg.decimation, cfg.sim_dt, cfg.actor_heights = 4, 10, 0.002, 1
        env = C.c_void_p()
        assert lib.bg_env_create(C.byref(cfg), model, C.byref(env)) == -1 and b"actor_heights" in lib.bg_last_error()
    finally:
        lib.bg_model_destroy(model)


def test_play_oracle_builds_the_row_with_the_noiseless_scan():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import play_oracle as po
    finally:
        sys.path.pop(0)
    from booster_gym_amd.utils.terrain import height_scan_points

    cfg = _cfg()
    pts = height_scan_points(cfg["terrain"])[1]
    layers = [(np.zeros((256, 47 * 3 + P)), np.zeros(256))]
    assert po.actor_frames(layers, scan=P) == 3 and po.actor_frames([(np.zeros((8, 94)), None)]) == 2
    with pytest.raises(ValueError, match=r"terrain\.actor_heights"):
        po.actor_frames(layers, scan=P - 1)
    root = np.zeros(13); root[2], root[6] = 0.7, 1.0
    row = po.height_scan(root, pts, cfg)
    S, target = cfg["normalization"]["height_measurements"], cfg["rewards"]["base_height_target"]
    assert row.shape == (P,) and np.allclose(row, (0.7 - target) * S, atol=1e-12)  # on the oracle's plane h = 0
    bumps = po.height_scan(root, pts, cfg, terrain_height=lambda x, y: 0.1 * x)
    assert np.allclose(bumps, np.clip(0.7 - 0.1 * pts[:, 0].astype(np.float64) - target, -1, 1) * S, atol=1e-12)
    root[2] = 5.0
    assert np.array_equal(po.height_scan(root, pts, cfg), np.full(P, S))  # the clip at +1
