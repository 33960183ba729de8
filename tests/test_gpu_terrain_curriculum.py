"""The terrain curriculum on the GPU (terrain.curriculum): the level update in the env step's reset path (bg_env.h) against a numpy restatement of
legged_gym's rule, the device's level sum and origins after many steps, T1.reset(), and the Runner's log and checkpoint."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 6  # levels of these tests


def _env(n=320, **over):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": n, "terrain.curriculum": True, "terrain.num_levels": L, "terrain.max_init_level": 3, "basic.sim_device": DEV,
          "basic.rl_device": DEV}
    ov.update(over)
    return T1(load_cfg("T1", ov))


def _rule(p_xy, o_xy, cmd_xy, level, tile_length, episode_length_s):
    """legged_gym's _update_terrain_curriculum for envs that are reset, before any wrap past the top level (-> values >= num_levels)."""
    d = np.linalg.norm(p_xy - o_xy, axis=1)
    up = d > tile_length / 2
    down = ~up & (d < np.linalg.norm(cmd_xy, axis=1) * episode_length_s * 0.5)
    return np.maximum(level + up.astype(int) - down.astype(int), 0)


def _centres(env, levels, cols):
    return env.terrain.tile_centres(np.asarray(levels), np.asarray(cols))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_level_update_at_reset_follows_the_rule(dtype):
    env = _env(**{"sim.state_dtype": dtype})
    n, cfg = env.num_envs, env.cfg
    tl, border = cfg["terrain"]["terrain_length"], cfg["terrain"]["border_size"]
    env.reset()
    assert env.max_terrain_level == L
    # groups of envs placed by hand: far / near with a large command / near with none / on the top level and far / outside the teleport bound
    A, B, C, D, E = np.arange(0, 16), np.arange(16, 32), np.arange(32, 48), np.arange(48, 112), np.arange(112, 128)
    placed = np.concatenate([A, B, C, D, E])
    lv = env.terrain_levels.cpu().numpy().copy()
    lv[D] = L - 1
    env.terrain_levels = torch.from_numpy(lv)  # moves the origins of D to their top-level tiles
    lv0 = env.terrain_levels.cpu().numpy()
    cols = env.terrain_types.cpu().numpy()
    assert np.array_equal(lv0, lv) and int(env.terrain_level_sum().item()) == int(lv.sum())
    o0 = env.get_field("env_origins").cpu().numpy()
    assert np.allclose(o0, _centres(env, lv0, cols), atol=1e-4)

    root = env.root_states.cpu().numpy().copy()
    cmd = env.commands.cpu().numpy().copy()
    p = o0[:, :2].copy()
    sgn = np.where(lv0 < L // 2, 1.0, -1.0)
    p[A, 1] += 7.5 * sgn[A]
    p[D, 1] += 7.5 * sgn[D]
    p[B, 0] += 0.5
    p[C, 0] += 0.5
    p[E, 0] = -0.8 * border  # beyond the teleport bound at -0.75 border: an env that crossed the wrap lands far from its origin
    cmd[B] = [1.0, 0.5, 0.2]
    cmd[C] = 0.0
    h = env.terrain.terrain_heights(np.c_[p, np.zeros(n)]).cpu().numpy()
    # lying on its side, trunk 0.3 m above the ground (below terminate_height 0.45): feet in the air, reset at the end of the step
    root[placed, 0:2] = p[placed]
    root[placed, 2] = h[placed] + 0.3
    root[placed, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
    root[placed, 7:13] = 0.0
    env.set_field("root_states", torch.from_numpy(root).float())
    env.set_field("commands", torch.from_numpy(cmd).float())
    cmd_used = env.commands.cpu().numpy()  # (fp16 state: the command as stored)

    env.step(torch.zeros(n, 12, device=DEV))
    done = env.reset_buf.cpu().numpy().astype(bool)
    lv1 = env.terrain_levels.cpu().numpy()
    o1 = env.get_field("env_origins").cpu().numpy()
    r1 = env.root_states.cpu().numpy()
    assert done[placed].all()

    want = _rule(p, o0[:, :2], cmd_used[:, :2], lv0, tl, cfg["rewards"]["episode_length_s"])
    assert (want[A] == np.minimum(lv0[A] + 1, L)).all() and (want[C] == lv0[C]).all() and (want[E] == lv0[E] + 1).all()
    assert (want[B] == np.maximum(lv0[B] - 1, 0)).all() and (lv0[B] > 0).any() and (want[D] == L).all()
    stay = placed[want[placed] < L]
    assert np.array_equal(lv1[stay], want[stay])
    wrapped = placed[want[placed] >= L]
    assert len(wrapped) >= len(D)
    assert lv1[wrapped].min() >= 0 and lv1[wrapped].max() < L and len(np.unique(lv1[wrapped])) > 1
    # reset envs: origin = centre of the new tile; spawn inside the init_base_pos_xy box around it, at base_init z above the ground
    r = done
    assert np.allclose(o1[r, :2], _centres(env, lv1, cols)[r, :2], atol=1e-5)
    assert np.allclose(o1[r, 2], _centres(env, lv1, cols)[r, 2], atol=1e-4)
    lo, hi = cfg["randomization"]["init_base_pos_xy"]["range"]
    base = np.asarray(cfg["init_state"]["pos"])
    off = r1[r, :2] - base[:2] - o1[r, :2]
    assert (off >= lo - 1e-4).all() and (off <= hi + 1e-4).all()
    hs = env.terrain.terrain_heights(np.c_[r1[r, :2], np.zeros(r.sum())]).cpu().numpy()
    assert np.allclose(r1[r, 2], base[2] + hs, atol=2e-3)
    # envs that were not reset keep their level and origin
    k = ~done
    assert k.sum() > 100
    assert np.array_equal(lv1[k], lv0[k]) and np.array_equal(o1[k], o0[k])
    assert int(env.terrain_level_sum().item()) == int(lv1.sum())


@pytest.mark.parametrize("over", [{}, {"sim.state_dtype": "fp16"},
                                  {"commands.curriculum": True, "parallel.exact_still_count": True, "parallel.same_step_curriculum": True}],
                         ids=["fp32", "fp16", "command_curriculum"])
def test_level_sum_and_origins_after_random_steps(over):
    env = _env(**over)
    n = env.num_envs
    env.reset()
    lv_start = env.terrain_levels.cpu().numpy()
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(300):
        env.step(torch.randn(n, 12, device=DEV, generator=g))
    lv = env.terrain_levels.cpu().numpy()
    cols = env.terrain_types.cpu().numpy()
    assert lv.min() >= 0 and lv.max() < L and (lv != lv_start).any()
    assert int(env.terrain_level_sum().item()) == int(lv.sum())
    o = env.get_field("env_origins").cpu().numpy()
    c = _centres(env, lv, cols)
    assert np.allclose(o[:, :2], c[:, :2], atol=1e-5) and np.allclose(o[:, 2], c[:, 2], atol=1e-4)
    assert np.allclose(env.env_origins.cpu().numpy(), o)
    # T1.reset() never moves a level
    env.reset()
    assert np.array_equal(env.terrain_levels.cpu().numpy(), lv) and int(env.terrain_level_sum().item()) == int(lv.sum())
    assert np.isfinite(env.root_states.cpu().numpy()).all()


def test_curriculum_off_has_no_level_state():
    env = _env(n=64, **{"terrain.curriculum": False})
    with pytest.raises(RuntimeError, match="terrain curriculum"):
        env.get_field("terrain_level")
    assert isinstance(env.env_origins, torch.Tensor) and env.env_origins is env.env_origins


class _Rec:
    def __init__(self):
        self.stats = {}

    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        return None


def _runner(n, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    ov = {"env.num_envs": n, "terrain.curriculum": True, "terrain.num_levels": L, "terrain.max_init_level": 3, "runner.mini_epochs": 2}
    ov.update(over)
    return Runner(cfg=load_cfg("T1", ov))


def test_runner_logs_mean_level_and_checkpoint_restores_levels(tmp_path, capsys):
    r = _runner(128)
    rec = _Rec()
    r.begin_training(recorder=rec)
    for it in range(3):
        r.train_iteration(it)
    r._flush_log()
    m = rec.stats[2]["terrain/mean_level"]
    lv = r.env.terrain_levels
    assert np.isfinite(m) and 0.0 <= m <= L - 1 and abs(m - float(lv.double().mean())) < 1e-9
    ck = r.checkpoint_dict()
    assert torch.equal(ck["terrain_levels"], lv)
    path = str(tmp_path / "model_3.pth")
    torch.save(ck, path)
    del r

    r2 = _runner(128, **{"basic.checkpoint": path, "basic.seed": 7})
    assert torch.equal(r2.env.terrain_levels.cpu(), lv.cpu())
    assert int(r2.env.terrain_level_sum().item()) == int(lv.sum())
    o = r2.env.get_field("env_origins").cpu().numpy()
    assert np.allclose(o, r2.env.terrain.tile_centres(lv.cpu().numpy(), r2.env.terrain_types.cpu().numpy()), atol=1e-4)
    del r2
    # another env count: the initial draw stays, with a message; a checkpoint without levels loads as before
    r3 = _runner(96, **{"basic.checkpoint": path})
    assert "terrain levels" in capsys.readouterr().out
    assert torch.equal(r3.env.terrain_levels.cpu(), torch.from_numpy(r3.env._terrain_init[0]))
    del r3
    ck.pop("terrain_levels")
    torch.save(ck, path)
    r4 = _runner(128, **{"basic.checkpoint": path})
    assert torch.equal(r4.env.terrain_levels.cpu(), torch.from_numpy(r4.env._terrain_init[0]))
