"""The critic's privileged extras on the GPU (env.privileged_extras): bg_priv_extras against a numpy restatement from the stored fields at every step of
runs in which envs reset, the first 14 + P columns and the observations against an env with the key off (bitwise), its place beside bg_height_scan,
bg_obs_stack and bg_obs_assemble, step_to, a plane, the key absent against [], one PPO update against the reference loop, the estimator on the feet
columns, the checkpoint's refusal, evaluate / export, and bg_env_create's argument check."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT_EPISODES = {"rewards.episode_length_s": 0.13}  # 7 steps: every env resets several times inside a run (tests/test_gpu_actor_memory.py)
ALL = ["feet", "ground", "joints"]
WIDTH = {"feet": 6, "ground": 6, "joints": 12}
GRID_3x2 = {"terrain.measure_heights": True, "terrain.measured_points_x": [-0.2, 0.0, 0.2], "terrain.measured_points_y": [-0.1, 0.1]}
N, STEPS = 70, 60  # two blocks of 64 envs, the second ragged


def _ov(n, groups, P=0, **over):
    X = sum(WIDTH[g] for g in groups or ())
    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV, "env.num_privileged_obs": 14 + P + X}
    ov.update(SHORT_EPISODES)
    if groups is not None:
        ov["env.privileged_extras"] = list(groups)
    ov.update(over)
    return ov


def _env(n, groups, P=0, **over):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    return T1(load_cfg("T1", _ov(n, groups, P, **over)))


def _actions(n, k, amp=0.6):
    g = torch.Generator(device="cpu").manual_seed(1000 + k)
    return ((torch.rand(n, 12, generator=g) * 2 - 1) * amp).to(DEV)


def _heights64(t, x, y):
    """Terrain.terrain_heights' bilinear rule (indices clamped to the field) in float64; 0 on a plane."""
    if t.type == "plane":
        return np.zeros_like(x)
    hf = t.height_field_raw.astype(np.float64)
    px, py = t.border_pixels + x / t.horizontal_scale, t.border_pixels + y / t.horizontal_scale
    x1 = np.clip(np.floor(px).astype(np.int64), 0, hf.shape[0] - 2)
    y1 = np.clip(np.floor(py).astype(np.int64), 0, hf.shape[1] - 2)
    fx, fy = px - x1, py - y1
    return ((1 - fx) * (1 - fy) * hf[x1, y1] + fx * (1 - fy) * hf[x1 + 1, y1] + (1 - fx) * fy * hf[x1, y1 + 1] + fx * fy * hf[x1 + 1, y1 + 1]) * t.vertical_scale


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_extras(env, priv, where):
    """The extras' columns of `priv` [n][14 + P + X] (numpy) against the stored fields of `env`, read through its field getter: every env, every column.
    Returns the worst clearance error."""
    f = {k: env.get_field(k).cpu().numpy() for k in ("feet_contact", "feet_contact_forces", "feet_pos", "foot_material", "dof_friction")}
    off, groups = env.privileged_extras_offset, env.privileged_extras
    assert priv.shape[1] == off + env.num_privileged_extras
    c, err = off, 0.0
    if "feet" in groups:
        assert np.isin(f["feet_contact"], (0.0, 1.0)).all(), where
        assert np.array_equal(_bits(priv[:, c : c + 2]), _bits(f["feet_contact"])), where
        s = np.float32(env.cfg["normalization"].get("contact_force", 0.003))
        force = np.clip(np.float32(f["feet_contact_forces"][:, [2, 5]]) * s, np.float32(-5), np.float32(5))
        assert force.dtype == np.float32 and np.array_equal(_bits(priv[:, c + 2 : c + 4]), _bits(force)), where
        fp = f["feet_pos"].astype(np.float64).reshape(-1, 2, 3)
        h = _heights64(env.terrain, fp[:, :, 0], fp[:, :, 1])
        clear = np.clip(fp[:, :, 2] - h, -1.0, 1.0) * float(env.cfg["normalization"].get("height_measurements", 5.0))
        err = float(np.abs(priv[:, c + 4 : c + 6].astype(np.float64) - clear).max())
        assert err < 1e-4, (where, err)
        c += 6
    if "ground" in groups:
        assert np.array_equal(_bits(priv[:, c : c + 6]), _bits(f["foot_material"])), where
        c += 6
    if "joints" in groups:
        assert np.array_equal(_bits(priv[:, c : c + 12]), _bits(f["dof_friction"])), where
        c += 12
    assert c == priv.shape[1]
    return err


def _run(env, steps, amp=0.6):
    """reset() and `steps` steps of the shared actions: per step (obs, privileged, rew, done, time_outs) on the host, the extras checked at each."""
    out, worst, resets = [], 0.0, 0
    env.reset()
    for k in range(steps + 1):
        if k:
            env.step(_actions(env.num_envs, k - 1, amp))
        torch.cuda.synchronize()
        row = [t.cpu().numpy().copy() for t in (env.obs_buf, env.privileged_obs_buf, env.rew_buf, env.reset_buf, env.time_out_buf)]
        assert np.isfinite(row[1]).all(), k
        if env.num_privileged_extras:
            worst = max(worst, _check_extras(env, row[1], f"step {k}"))
        resets += int(row[3].sum()) if k else 0
        out.append(row)
    return out, worst, resets


def _same_but_the_extras(on, off, width):
    """Every output of the key-on run bitwise that of the key-off run; of the privileged rows, the first `width` columns."""
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(_bits(a[0]), _bits(b[0])), k
        assert b[1].shape[1] == width and np.array_equal(_bits(a[1][:, :width]), _bits(b[1])), k
        for x, y in zip(a[2:], b[2:]):
            assert np.array_equal(x, y), k


# ------------------------------------------------------------------ 1. values
_OFF_RUNS = {}


def _off_run(dtype):
    """The run with the key off on the same seed and actions, once per state dtype, shared and left unchanged."""
    if dtype not in _OFF_RUNS:
        _OFF_RUNS[dtype] = _run(_env(N, None, **{"terrain.type": "trimesh", "terrain.curriculum": True, "sim.state_dtype": dtype}), STEPS)[0]
    return _OFF_RUNS[dtype]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("groups", [["feet"], ["ground"], ["joints"], ALL], ids=lambda g: "+".join(g))
def test_extras_match_the_stored_fields_at_every_step(groups, dtype):
    env = _env(N, groups, **{"terrain.type": "trimesh", "terrain.curriculum": True, "sim.state_dtype": dtype})
    X = sum(WIDTH[g] for g in groups)
    assert env.privileged_extras == tuple(groups) and env.num_privileged_extras == X and env.privileged_extras_offset == 14
    assert len(env.privileged_extra_names) == X and tuple(env.privileged_obs_buf.shape) == (N, 14 + X)
    on, worst, resets = _run(env, STEPS)
    print(f"{groups} {dtype}: worst clearance error {worst:.3e}, {resets} resets in {STEPS} steps")
    assert resets >= 4 * N  # (episodes of 7 steps: the reset-step rule is part of what was compared)
    _same_but_the_extras(on, _off_run(dtype), 14)
    last = on[-1][1][:, 14:]
    if "feet" in groups:  # the columns carry something: both contact states occur, forces and clearances vary
        feet = np.concatenate([r[1][:, 14:20] for r in on])
        assert set(np.unique(feet[:, :2])) == {0.0, 1.0} and feet[:, 2:4].std() > 1e-3 and feet[:, 4:6].std() > 1e-3
        assert np.abs(feet[:, 2:4]).max() <= 5.0 and np.abs(feet[:, 4:6]).max() <= 5.0
    if "ground" in groups:
        assert last[:, -18 if "joints" in groups else -6].std() > 0.1  # the left sole's friction, 0.1 .. 2.0 over the envs
    if "joints" in groups:
        assert last[:, -12:].std() > 0.1 and last[:, -12:].min() >= 0.0 and last[:, -12:].max() <= 2.0


# ------------------------------------------------------------------ 2. beside the other launches
@pytest.mark.parametrize("kind", ["height_scan", "frame_stack", "actor_heights"])
def test_extras_beside_the_other_post_step_launches(kind):
    over = {"terrain.type": "trimesh"}
    P = 0
    if kind == "height_scan":
        over.update(GRID_3x2); P = 6
    elif kind == "frame_stack":
        over.update({"env.frame_stack": 3, "env.num_observations": 141})
    else:
        over.update(GRID_3x2); P = 6
        over.update({"terrain.actor_heights": True, "env.num_observations": 47 + P})
    on_env = _env(N, ALL, P, **over)
    assert on_env.privileged_extras_offset == 14 + P and tuple(on_env.privileged_obs_buf.shape) == (N, 38 + P)
    on, worst, resets = _run(on_env, 30)
    off, _, _ = _run(_env(N, None, P, **over), 30)
    print(f"{kind}: worst clearance error {worst:.3e}, {resets} resets")
    assert resets >= 2 * N
    _same_but_the_extras(on, off, 14 + P)
    if P:
        assert np.concatenate([r[1][:, 14 : 14 + P] for r in on]).std() > 1e-3  # the scan's columns are the scan


def test_step_to_writes_the_extras_into_the_callers_rows_and_nothing_past_n():
    env = _env(N, ALL, **{"terrain.type": "trimesh"})
    env.reset()
    S = 38
    slab = torch.full((3, N + 5, S), float("nan"), device=DEV)
    obs, rew = torch.empty(N, 47, device=DEV), torch.empty(N, device=DEV)
    done, tout = torch.empty(N, dtype=torch.bool, device=DEV), torch.empty(N, dtype=torch.bool, device=DEV)
    for k in range(9):
        row = slab[k % 3]
        row.fill_(float("nan"))
        env.step_to(_actions(N, k), obs, row[:N], rew, done, tout)
        torch.cuda.synchronize()
        b = row.cpu().numpy()
        assert np.isfinite(b[:N]).all() and np.isnan(b[N:]).all(), k
        _check_extras(env, b[:N], f"step_to {k}")
    with pytest.raises(RuntimeError, match=f"privileged_obs of {N} x 38"):
        env.step_to(_actions(N, 0), obs, torch.empty(N, 14, device=DEV), rew, done, tout)


def test_on_a_plane_the_clearance_is_the_foot_height():
    env = _env(N, ALL, **{"terrain.type": "plane"})
    on, worst, resets = _run(env, 20)
    assert resets >= N and worst < 1e-4
    z = env.get_field("feet_pos").cpu().numpy()[:, [2, 5]]
    assert np.array_equal(_bits(on[-1][1][:, 18:20]), _bits(np.clip(z, -1, 1) * np.float32(5.0)))  # h = 0: nothing to round but the product


# ------------------------------------------------------------------ 3. off is off
class _Rec:
    def __init__(self):
        self.stats = {}

    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        return None


def _runner(n, groups, P=0, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    return Runner(cfg=load_cfg("T1", _ov(n, groups, P, **over)))


def _train(r, iters):
    rec = _Rec()
    r.begin_training(recorder=rec)
    for it in range(iters):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    return rec


def _digest(r, rec):
    h = hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [r.optimizer.exp_avg, r.optimizer.exp_avg_sq]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    for it in sorted(rec.stats):
        for k in sorted(rec.stats[it]):
            h.update(f"{it} {k} {float(rec.stats[it][k])!r}\n".encode())
    return h.hexdigest()


def test_the_key_absent_and_the_empty_list_are_the_same_run():
    digests, keys = [], []
    for groups in (None, []):
        r = _runner(64, groups, **{"terrain.type": "plane", "runner.mini_epochs": 2})
        assert r.env.privileged_extras == () and r.model.critic[0].in_features == 61 and r._critic_in.shape[-1] == 64
        rec = _train(r, 2)
        assert len(rec.stats) == 2
        digests.append(_digest(r, rec))
        ck = r.checkpoint_dict()
        keys.append(sorted(ck))
        assert "privileged_extras" not in ck
        del r
    assert digests[0] == digests[1] and keys[0] == keys[1]
    runs = [_run(_env(64, groups, **{"terrain.type": "plane"}), STEPS)[0] for groups in (None, [])]
    _same_but_the_extras(runs[0], runs[1], 14)


# ------------------------------------------------------------------ 4. the update
def test_update_with_all_three_groups_matches_the_reference_loop():
    """Critic input 47 + 14 + 24 = 85, padded to 128: the per-layer kernels for the critic, the chained ones for the actor; helper and bounds of the
    wide-critic update tests (tests/test_gpu_actor_heights.py's plain case: tests/test_gpu_mini_batches.py's compare_with_reference)."""
    from test_gpu_mini_batches import compare_with_reference

    from booster_gym_amd.utils.model import ActorCritic
    from oracle.ppo_ref import ppo_update_reference

    E, T, n = 3, 24, 128
    r = _runner(n, ALL, **{"terrain.type": "plane", "runner.mini_epochs": E, "runner.horizon_length": T})
    assert r.model.critic[0].in_features == 85 and r.model.actor[0].in_features == 47
    assert r._critic_in.shape[-1] == 128 and r._actor_in.shape[-1] == 64
    plan = r._resolve_plan()
    assert plan.critic.fwd == "layer" and plan.critic.bwd == "layer" and plan.actor.fwd == "chain_split" and not plan.ahead and plan.fused_head
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    r.rollout()
    b = r.buffer
    assert tuple(b["privileged_obses"].shape) == (T + 1, n, 38) and b["privileged_obses"][:, :, 14:20].std() > 1e-3 and bool(b["dones"].any())
    ref_model = ActorCritic(12, 47, 38).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    rewards_ref = b["rewards"].clone()
    stats_ref, lr_ref = ppo_update_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), b["obses"][:T].clone(), b["privileged_obses"][:T].clone(),
                                             b["actions"].clone(), rewards_ref, b["dones"].clone(), b["time_outs"].clone(), b["obses"][T].clone(),
                                             b["privileged_obses"][T].clone(), mini_epochs=E, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    acc = r.update()
    torch.cuda.synchronize()
    compare_with_reference(r, ref_model, stats_ref, lr_ref, p_start, acc)
    for (k, p), (_, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    assert torch.allclose(b["rewards"], rewards_ref, atol=1e-5)


@pytest.mark.parametrize("over", [{"algorithm.symmetry_loss": True}, {"algorithm.empirical_normalization": True, "runner.num_mini_batches": 2},
                                  {"algorithm.rnn_hidden_size": 128}, {"sim.state_dtype": "fp16", "commands.curriculum": True}],
                         ids=["symmetry", "normalisation+mini_batches", "recurrent", "fp16+command_curriculum"])
def test_the_key_composes_with_the_other_training_keys(over):
    r = _runner(128, ALL, **{"terrain.type": "plane", "runner.mini_epochs": 2}, **over)
    assert r.model.critic[0].in_features == 85
    rec = _train(r, 2)
    assert len(rec.stats) == 2
    for it, s in rec.stats.items():
        for k, v in s.items():
            assert np.isfinite(float(v)), (it, k, v)
    assert torch.isfinite(r.optimizer.flat).all()


# ------------------------------------------------------------------ 5. the estimator on the feet columns
def test_estimator_regresses_the_feet_columns():
    from booster_gym_amd.utils.estimator import estimator_targets

    targets = [4, 5, 6, 7, 14, 15]
    r = _runner(128, ["feet"], **{"terrain.type": "plane", "runner.mini_epochs": 2, "estimator.enabled": True, "estimator.targets": targets})
    names = r.env.privileged_extra_names
    assert [r.env.privileged_extras_offset + names.index(k) for k in ("feet.contact_left", "feet.contact_right")] == [14, 15]
    assert r._est.targets == tuple(targets) and r.model.actor[0].in_features == 47 + 6 and r.model.critic[0].in_features == 47 + 20
    r.begin_training(recorder=_Rec())
    T = r.cfg["runner"]["horizon_length"]
    for it in range(2):
        r.rollout()
        priv = r.buffer["privileged_obses"][:T].reshape(T * 128, -1).clone()
        stats = r.update()
        torch.cuda.synchronize()
        # the rows the update has just regressed onto are still in the trainer: the chosen privileged columns, then zeros
        tr = r._est_trainer
        assert torch.equal(tr.target[:, :6], priv[:, targets]) and not tr.target[:, 6:].any(), it
        assert torch.equal(tr.target, estimator_targets(priv, r._est.targets)), it
        contact = tr.target[:, 4:6]
        assert bool(((contact == 0) | (contact == 1)).all()) and 0.0 < float(contact.mean()) < 1.0, it
        loss = r._summarize(stats)["estimator/loss"]
        print(f"iteration {it}: estimator/loss {loss!r}")
        assert np.isfinite(loss) and loss > 0, (it, loss)
        r.buffer.roll()


# ------------------------------------------------------------------ 6. checkpoint, evaluate, export
def test_checkpoint_names_the_groups_and_a_config_that_disagrees_is_refused(tmp_path):
    from booster_gym_amd.utils.evaluate import Evaluator

    base = {"terrain.type": "plane", "runner.mini_epochs": 2, "runner.horizon_length": 4}
    r = _runner(64, ["ground", "feet"], **base)
    _train(r, 1)
    ck = r.checkpoint_dict()
    assert ck["privileged_extras"] == ["feet", "ground"]
    path = str(tmp_path / "model_1.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r
    r2 = _runner(64, ["feet", "ground"], **base, **{"basic.checkpoint": path})
    for k, v in r2.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    del r2
    with pytest.raises(ValueError, match=r"env\.privileged_extras = \['feet', 'ground'\].*env\.privileged_extras = \['feet'\]"):
        _runner(64, ["feet"], **base, **{"basic.checkpoint": path})
    with pytest.raises(ValueError, match=r"env\.privileged_extras = \['feet', 'ground'\].*env\.privileged_extras = \[\]"):
        _runner(64, None, **base, **{"basic.checkpoint": path})
    with pytest.raises(ValueError, match=r"env\.privileged_extras = \['feet', 'ground'\].*env\.privileged_extras = \['joints'\]"):
        _runner(64, ["joints"], **base, **{"basic.checkpoint": path})  # 12 columns either way: the critic's width alone would not tell
    # a checkpoint saved with the key off, under a config with it on
    r3 = _runner(64, None, **base)
    path_off = str(tmp_path / "model_off.pth")
    torch.save(r3.checkpoint_dict(), path_off)
    del r3
    with pytest.raises(ValueError, match=r"env\.privileged_extras = \[\].*env\.privileged_extras = \['feet', 'ground'\]"):
        _runner(64, ["feet", "ground"], **base, **{"basic.checkpoint": path_off})

    ev = Evaluator(checkpoint=path, overrides=_ov(64, ["feet", "ground"], **{"terrain.type": "plane", "rewards.episode_length_s": 0.4, "runner.horizon_length": 4}))
    rep = ev.run()
    assert rep["all"]["robots"] == 64 and rep["all"]["unfinished"] == 0
    del ev
    torch.cuda.synchronize()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={path}"], cwd=str(tmp_path), env=env, check=True,
                   timeout=300)
    actor = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    assert tuple(actor(torch.zeros(3, 47)).shape) == (3, 12)


# ------------------------------------------------------------------ 7. the C ABI's check
def test_env_create_refuses_an_unknown_bit():
    from booster_gym_amd import _lib

    env = _env(4, ["joints"], **{"terrain.type": "plane"})
    cfg = env._cfg_struct()
    assert cfg.priv_extras == _lib.PRIV_EXTRA_JOINTS and cfg.priv_force_scale == 0.0
    lib = env._lib
    for mask in (8, 7 | 16, -1):
        cfg.priv_extras = mask
        out = C.c_void_p()
        assert lib.bg_env_create(C.byref(cfg), env._model, C.byref(out)) == -1 and b"priv_extras" in lib.bg_last_error(), mask
