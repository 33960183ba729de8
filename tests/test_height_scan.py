"""Terrain height scan of the critic (terrain.measure_heights, an addition of this build): the point grid, the config checks, the critic's input pad
and the update plan it leads to.  CPU only; the scan values on the device and the training run are tests/test_gpu_height_scan.py."""
import numpy as np
import pytest

from booster_gym_amd.utils.config import load_cfg
from booster_gym_amd.utils.terrain import height_scan_points

P = 187  # legged_gym's default grid: 17 x 11


def _scan_cfg(n=4, **over):
    ov = {"env.num_envs": n, "terrain.measure_heights": True, "env.num_privileged_obs": 14 + P}
    ov.update(over)
    return load_cfg("T1", ov)


def test_default_grid_is_legged_gyms_in_ij_order():
    on, pts = height_scan_points(load_cfg("T1", {"terrain.measure_heights": True})["terrain"])
    assert on and pts.shape == (P, 2) and pts.dtype == np.float32
    xs = np.round(np.arange(-0.8, 0.8 + 1e-9, 0.1), 1)
    ys = np.round(np.arange(-0.5, 0.5 + 1e-9, 0.1), 1)
    assert len(xs) == 17 and len(ys) == 11
    for i in range(17):
        for j in range(11):
            p = i * 11 + j
            assert pts[p, 0] == np.float32(xs[i]) and pts[p, 1] == np.float32(ys[j])
    # the keys absent: the same default grid
    t = {k: v for k, v in load_cfg("T1")["terrain"].items() if k not in ("measured_points_x", "measured_points_y")}
    t["measure_heights"] = True
    assert np.array_equal(height_scan_points(t)[1], pts)


def test_custom_grid_order():
    t = dict(load_cfg("T1")["terrain"], measure_heights=True, measured_points_x=[0.5, -0.5], measured_points_y=[-0.2, 0.0, 0.3])
    _, pts = height_scan_points(t)
    want = np.array([[0.5, -0.2], [0.5, 0.0], [0.5, 0.3], [-0.5, -0.2], [-0.5, 0.0], [-0.5, 0.3]], dtype=np.float32)
    assert np.array_equal(pts, want)


def test_off_and_absent_keep_14_privileged_observations():
    cfg = load_cfg("T1")
    assert cfg["terrain"]["measure_heights"] is False and cfg["env"]["num_privileged_obs"] == 14
    on, pts = height_scan_points(cfg["terrain"])
    assert not on and pts.shape == (0, 2)
    absent = {k: v for k, v in cfg["terrain"].items() if k not in ("measure_heights", "measured_points_x", "measured_points_y")}
    on, pts = height_scan_points(absent)
    assert not on and pts.shape == (0, 2)
    # without the scan, 14 + P privileged observations is the build's old error
    from booster_gym_amd.envs import T1

    with pytest.raises(ValueError, match="14 privileged observations"):
        T1(load_cfg("T1", {"env.num_envs": 4, "env.num_privileged_obs": 14 + P}))


@pytest.mark.parametrize("over, match", [
    ({"terrain.type": "plane"}, r"terrain\.measure_heights"),
    ({"env.num_privileged_obs": 14}, r"env\.num_privileged_obs.*set env\.num_privileged_obs to 201"),
    ({"env.num_privileged_obs": 61}, r"201"),
    ({"terrain.measured_points_x": []}, r"terrain\.measured_points_x"),
    ({"terrain.measured_points_y": []}, r"terrain\.measured_points_y"),
    ({"terrain.measured_points_x": [0.1 * i for i in range(42)]}, r"terrain\.measured_points_x.*exceeds 512"),
])
def test_config_errors_name_the_key(over, match):
    from booster_gym_amd.envs import T1

    with pytest.raises(ValueError, match=match):
        T1(_scan_cfg(**over))


def test_size_checks_accept_the_scan_widths():
    """check_env_sizes (what T1 runs before it touches the device): 14 + P accepted with the scan, 61 + P = 512 exactly (41 x 11 = 451 points) too."""
    from booster_gym_amd.envs.t1 import MAX_CRITIC_INPUT, check_env_sizes

    assert MAX_CRITIC_INPUT == 512
    check_env_sizes(_scan_cfg(), P)
    check_env_sizes(load_cfg("T1"), 0)
    check_env_sizes(_scan_cfg(**{"env.num_privileged_obs": 14 + 451}), 451)
    with pytest.raises(ValueError, match="exceeds 512"):
        check_env_sizes(_scan_cfg(**{"env.num_privileged_obs": 14 + 462}), 462)


def test_critic_pad_helper():
    from booster_gym_amd.utils.runner import pad_input

    assert pad_input(47) == 64 and pad_input(61) == 64 and pad_input(64) == 64
    assert pad_input(61 + 4) == 128 and pad_input(128) == 128
    assert pad_input(61 + P) == 256 and pad_input(256) == 256
    assert pad_input(257) == 512 and pad_input(512) == 512
    with pytest.raises(ValueError, match="512"):
        pad_input(513)


def _switches(**over):
    sw = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
              defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
    sw.update(over)
    return sw


@pytest.mark.parametrize("symmetry", [False, True])
def test_plan_with_the_scan_critic(symmetry):
    """A critic on a 256-column input is not chainable: it runs the per-layer fp32-MFMA kernels with its weight gradients in the grouped launch (ci = 256
    among them); the actor keeps its chained kernels; the forward-ahead and the one-stream form turn off by the existing rules."""
    from booster_gym_amd.utils.runner import plan_update

    p = plan_update(((61 + P, 256, 256, 128, 1), 256), ((47, 256, 128, 128, 12), 64), 24 * 4096, symmetry=symmetry, **_switches())
    assert p.critic.fwd == "layer" and p.critic.bwd == "layer" and all(p.critic.grouped[:-1])  # (the output layer: the fused head)
    assert p.actor.fwd == "chain_split"
    assert p.ahead is False and p.one_stream is False and p.chain_values is False
    # without the scan: both chained, as before
    q = plan_update(((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64), 24 * 4096, symmetry=symmetry, **_switches())
    assert q.critic.fwd == q.actor.fwd == "chain_split" and q.ahead is not symmetry
