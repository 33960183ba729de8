"""The critic's terrain height scan on the GPU (terrain.measure_heights): bg_height_scan against a float64 numpy restatement from the stored state, the
scan-off outputs unchanged bit for bit, a ragged env count, and the Runner's training, checkpoint and export with a 248-input critic."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 187
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ov(n, scan=True, **over):
    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV}
    if scan:
        ov.update({"terrain.measure_heights": True, "env.num_privileged_obs": 14 + P})
    ov.update(over)
    return ov


def _env(n, scan=True, **over):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    return T1(load_cfg("T1", _ov(n, scan, **over)))


def _scan_ref(env):
    """clip(z - h(xy + Rz(yaw) p) - base_height_target, -1, 1) * height_measurements in float64, from T1.root_states and Terrain.height_field_raw."""
    root = env.root_states.cpu().numpy().astype(np.float64)
    t, cfg = env.terrain, env.cfg
    qx, qy, qz, qw = root[:, 3], root[:, 4], root[:, 5], root[:, 6]
    yaw = np.arctan2(2.0 * (qw * qz + qx * qy), qw * qw + qx * qx - qy * qy - qz * qz)
    pts = env.height_points.cpu().numpy().astype(np.float64)
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    wx = root[:, 0:1] + c * pts[None, :, 0] - s * pts[None, :, 1]
    wy = root[:, 1:2] + s * pts[None, :, 0] + c * pts[None, :, 1]
    hf = t.height_field_raw.astype(np.float64)
    px, py = t.border_pixels + wx / t.horizontal_scale, t.border_pixels + wy / t.horizontal_scale
    x1 = np.clip(np.floor(px).astype(np.int64), 0, hf.shape[0] - 2)
    y1 = np.clip(np.floor(py).astype(np.int64), 0, hf.shape[1] - 2)
    fx, fy = px - x1, py - y1
    h = ((1 - fx) * (1 - fy) * hf[x1, y1] + fx * (1 - fy) * hf[x1 + 1, y1] + (1 - fx) * fy * hf[x1, y1 + 1] + fx * fy * hf[x1 + 1, y1 + 1]) * t.vertical_scale
    v = np.clip(root[:, 2:3] - h - cfg["rewards"]["base_height_target"], -1.0, 1.0)
    return v * cfg["normalization"]["height_measurements"]


def _actions(n, k, amp=0.6):
    g = torch.Generator(device="cpu").manual_seed(1000 + k)
    return ((torch.rand(n, 12, generator=g) * 2 - 1) * amp).to(DEV)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("curriculum", [False, True])
def test_scan_matches_numpy_restatement(dtype, curriculum):
    n = 256
    env = _env(n, **{"sim.state_dtype": dtype, "terrain.curriculum": curriculum})
    assert env.num_height_points == P and tuple(env.height_points.shape) == (P, 2)
    assert tuple(env.privileged_obs_buf.shape) == (n, 14 + P)
    env.reset()
    torch.cuda.synchronize()
    scan = env.privileged_obs_buf[:, 14:].cpu().numpy()
    assert np.abs(scan - _scan_ref(env)).max() < 1e-4
    for k in range(60):
        if k == 20:  # base yaws spread over the circle (the reset draws them too; this makes sure every quadrant is covered)
            root = env.root_states.cpu().numpy().copy()
            yw = np.linspace(-np.pi, np.pi, n, endpoint=False)
            root[:, 3:7] = np.stack([np.zeros(n), np.zeros(n), np.sin(yw / 2), np.cos(yw / 2)], axis=1)
            env.set_field("root_states", torch.from_numpy(root).float())
        env.step(_actions(n, k, 0.3))
    torch.cuda.synchronize()
    scan = env.privileged_obs_buf[:, 14:].cpu().numpy()
    ref = _scan_ref(env)
    assert np.isfinite(scan).all()
    err = np.abs(scan - ref).max()
    assert err < 1e-4, err
    # the scan sees the terrain: not a constant, and within the clip
    assert scan.std() > 1e-3 and np.abs(scan).max() <= 5.0 + 1e-6


def test_scan_off_leaves_every_output_bitwise_unchanged():
    n = 192
    envs = {scan: _env(n, scan) for scan in (False, True)}
    for e in envs.values():
        e.reset()
    torch.cuda.synchronize()
    assert torch.equal(envs[False].obs_buf, envs[True].obs_buf)
    assert torch.equal(envs[False].privileged_obs_buf, envs[True].privileged_obs_buf[:, :14])
    resets = 0
    for k in range(100):
        if k == 40:  # some robots lying on their side: reset at the end of this step, in both envs alike
            for e in envs.values():
                root = e.root_states.cpu().numpy().copy()
                root[:32, 2] -= 0.4
                root[:32, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
                e.set_field("root_states", torch.from_numpy(root).float())
        a = _actions(n, k)
        out = {}
        for scan, e in envs.items():
            obs, rew, done, extras = e.step(a)
            out[scan] = [t.clone() for t in (obs, rew, done, extras["time_outs"], extras["privileged_obs"][:, :14])]
        for x, y in zip(out[False], out[True]):
            assert torch.equal(x, y), k
        resets += int(out[True][2].sum())
    assert resets >= 32


def test_ragged_env_count_writes_every_row_and_nothing_past_n():
    n = 1000
    env = _env(n)
    env.reset()
    S = 14 + P
    big = torch.full((n + 7, S), float("nan"), device=DEV)
    obs = torch.empty(n, 47, device=DEV)
    rew = torch.empty(n, device=DEV)
    done = torch.empty(n, dtype=torch.bool, device=DEV)
    tout = torch.empty(n, dtype=torch.bool, device=DEV)
    for k in range(3):
        env.step_to(_actions(n, k, 0.3), obs, big[:n], rew, done, tout)
    torch.cuda.synchronize()
    b = big.cpu().numpy()
    assert np.isfinite(b[:n]).all()
    assert np.isnan(b[n:]).all()
    assert np.abs(b[:n, 14:] - _scan_ref(env)).max() < 1e-4


class _Rec:
    def __init__(self):
        self.stats = {}

    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        return None


def _runner(n, scan=True, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    ov = _ov(n, scan, **{"runner.mini_epochs": 2})
    ov.update(over)
    return Runner(cfg=load_cfg("T1", ov))


def _train(r, iters):
    rec = _Rec()
    r.begin_training(recorder=rec)
    for it in range(iters):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    return rec


def test_runner_trains_checkpoints_and_exports_with_the_scan(tmp_path):
    r = _runner(256)
    assert r.model.critic[0].in_features == 61 + P and r.model.actor[0].in_features == 47
    assert r._critic_in.shape[-1] == 256 and r._actor_in.shape[-1] == 64
    rec = _train(r, 3)
    assert len(rec.stats) == 3
    for it, s in rec.stats.items():
        for k, v in s.items():
            assert np.isfinite(float(v)), (it, k, v)
    assert torch.isfinite(r.optimizer.flat).all()
    plan = r._resolve_plan()
    assert plan.critic.fwd == "layer" and plan.actor.fwd == "chain_split" and not plan.ahead
    ck = r.checkpoint_dict()
    path = str(tmp_path / "model_3.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r

    r2 = _runner(256, **{"basic.checkpoint": path})
    for k, v in r2.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    _train(r2, 1)
    del r2
    with pytest.raises(ValueError, match=r"248 inputs.*61.*terrain\.measure_heights"):
        _runner(256, scan=False, **{"basic.checkpoint": path})

    r3 = _runner(256, scan=False)
    path_off = str(tmp_path / "model_off.pth")
    torch.save(r3.checkpoint_dict(), path_off)
    del r3
    with pytest.raises(ValueError, match=r"61 inputs.*248.*terrain\.measure_heights"):
        _runner(256, **{"basic.checkpoint": path_off})

    # export_model.py: the 47-input actor, from the default config
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={path}"], cwd=str(tmp_path), env=env, check=True,
                   timeout=300)
    actor = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    mu = actor(torch.zeros(3, 47))
    assert tuple(mu.shape) == (3, 12)
    assert torch.allclose(actor(torch.ones(1, 47)), _actor_from(sd)(torch.ones(1, 47)), atol=1e-6)


def _actor_from(sd):
    from booster_gym_amd.utils.model import ActorCritic, hidden_of

    m = ActorCritic(12, 47, 14 + P, actor_hidden=hidden_of(sd, "actor"), critic_hidden=hidden_of(sd, "critic"))
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    return m.actor


def test_symmetry_loss_with_the_scan():
    r = _runner(256, **{"algorithm.symmetry_loss": True})
    rec = _train(r, 1)
    s = rec.stats[0]
    assert "symmetry_loss" in s and all(np.isfinite(float(v)) for v in s.values())
