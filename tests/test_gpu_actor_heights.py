"""The actor's terrain height scan on the GPU (terrain.actor_heights): bg_obs_assemble's clean scan against the critic's columns (bitwise) and a float64
restatement, the frame columns against an env with the key off (bitwise), the noise against oracle/task_ref.py's restatement of the generator on the
new stream ids, a ragged env count through step_to, the rollout actor at K = 234 and 328, the Runner's update against the reference loop (plain; with
normalisation + mini-batches + a frame stack; with the symmetry loss), checkpoint and export, and the key off against the key absent.

The default 17 x 11 grid (P = 187) fits the critic's 512 inputs up to H = 2 (47 H + 187 + 14 + 187), so the H = 3 cases run on a 9 x 5 grid (P = 45)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from test_gpu_height_scan import _scan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 187
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_9x5 = {"terrain.measured_points_x": [round(-0.4 + 0.1 * i, 1) for i in range(9)], "terrain.measured_points_y": [-0.2, -0.1, 0.0, 0.1, 0.2]}
NO_NOISE = {"noise.height_measurements": {"range": [0.0, 0.0], "operation": "additive", "distribution": "uniform"}}
RS_SCAN, RS_SCAN_RESET = 128, 384  # booster_gym_amd/csrc/bg_rng.h


def _ov(n, H=1, actor=True, **over):
    """Overrides of an env with the critic's scan, and with actor = True the actor's; H = 3 on the 9 x 5 grid."""
    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV, "terrain.measure_heights": True, "env.frame_stack": H}
    if H > 2:
        ov.update(GRID_9x5)
    p = 45 if H > 2 else P
    ov.update({"env.num_privileged_obs": 14 + p, "env.num_observations": 47 * H + (p if actor else 0), "terrain.actor_heights": actor})
    ov.update(over)
    return ov


def _env(n, H=1, actor=True, **over):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    return T1(load_cfg("T1", _ov(n, H, actor, **over)))


def _actions(n, k, amp=0.6):
    g = torch.Generator(device="cpu").manual_seed(1000 + k)
    return ((torch.rand(n, 12, generator=g) * 2 - 1) * amp).to(DEV)


def _tip_over(e, count=32):
    root = e.root_states.cpu().numpy().copy()
    root[:count, 2] -= 0.4
    root[:count, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
    e.set_field("root_states", torch.from_numpy(root).float())


# ------------------------------------------------------------------ 1. the clean part
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("curriculum", [False, True])
def test_clean_scan_equals_the_critics_bitwise_and_the_float64_restatement(dtype, curriculum, H):
    n = 256
    env = _env(n, H, **{"sim.state_dtype": dtype, "terrain.curriculum": curriculum, **NO_NOISE})
    p, F = env.num_height_points, 47 * H
    assert p == (P if H < 3 else 45) and (env.num_scan_obs, env.scan_obs_offset, env.num_single_obs, env.num_obs) == (p, F, 47, F + p)
    assert tuple(env.obs_buf.shape) == (n, F + p) and tuple(env.privileged_obs_buf.shape) == (n, 14 + p) and env._cfg_c.actor_heights == 1

    def check(what):
        torch.cuda.synchronize()
        a, c = env.obs_buf[:, F:], env.privileged_obs_buf[:, 14:]
        assert torch.equal(a, c), what
        err = np.abs(a.cpu().numpy() - _scan_ref(env)).max()
        print(f"{what}: max |scan - float64| {err:.3e}")
        assert err < 1e-4, (what, err)
        return a.cpu().numpy()

    env.reset()
    check("reset-all")
    for k in range(60):
        if k == 20:  # base yaws spread over the circle, as tests/test_gpu_height_scan.py does
            root = env.root_states.cpu().numpy().copy()
            yw = np.linspace(-np.pi, np.pi, n, endpoint=False)
            root[:, 3:7] = np.stack([np.zeros(n), np.zeros(n), np.sin(yw / 2), np.cos(yw / 2)], axis=1)
            env.set_field("root_states", torch.from_numpy(root).float())
        env.step(_actions(n, k, 0.3))
    scan = check("60 steps")
    assert np.isfinite(scan).all() and scan.std() > 1e-3 and np.abs(scan).max() <= 5.0 + 1e-6  # the scan sees the terrain, within the clip


# ------------------------------------------------------------------ 2. the frames
@pytest.mark.parametrize("H", [1, 3])
def test_frames_rewards_and_privileged_columns_equal_the_key_off_env_bitwise(H):
    n = 192
    on, off = _env(n, H), _env(n, H, actor=False)
    F = 47 * H
    assert tuple(off.obs_buf.shape) == (n, F) and off.num_scan_obs == 0 and off.scan_obs_offset == F
    for rep in range(2):  # (the second reset-all forgets the frames of the first)
        o1, x1 = on.reset()
        o0, x0 = off.reset()
        torch.cuda.synchronize()
        assert torch.equal(o1[:, :F], o0) and torch.equal(x1["privileged_obs"][:, :14], x0["privileged_obs"][:, :14])
        assert not o1[:, : F - 47].any()
    resets, worst = 0, 0.0
    for k in range(100):
        if k == 40:  # some robots lying on their side: reset at the end of this step, in both envs alike
            _tip_over(on); _tip_over(off)
        a = _actions(n, k)
        o1, r1, d1, x1 = on.step(a)
        o0, r0, d0, x0 = off.step(a)
        torch.cuda.synchronize()
        assert torch.equal(o1[:, :F], o0), k
        assert torch.equal(r1, r0) and torch.equal(d1, d0) and torch.equal(x1["time_outs"], x0["time_outs"]), k
        assert torch.equal(x1["privileged_obs"][:, :14], x0["privileged_obs"][:, :14]), k  # the env step's 14 columns
        # the clean scan is bg_height_scan's formula in another kernel, compiled under the relaxed floating-point flags on its own: the same values
        # to fp32 rounding (both are held to 1e-4 of the float64 restatement above), not the same bits
        worst = max(worst, (x1["privileged_obs"][:, 14:] - x0["privileged_obs"][:, 14:]).abs().max().item())
        if H > 1 and d1.any():  # bg_obs_stack's reset rule: H - 1 zero frames, the new observation last
            assert not o1[d1][:, : F - 47].any() and o1[d1][:, F - 47 : F].any(), k
        resets += int(d1.sum())
    assert resets >= 32, resets
    print(f"H {H}: max |clean scan of bg_obs_assemble - bg_height_scan| {worst:.3e}")
    assert worst < 1e-4, worst
    assert o1[:, :47].abs().sum() > 0  # (the oldest frame is in use by now)
    assert not torch.equal(o1[:, F:], x1["privileged_obs"][:, 14:])  # ... and the actor's scan carries the default noise


# ------------------------------------------------------------------ 3. / 4. the noise
def _draws(env, step, base, p):
    """(u, n) [N][p] of the scan's draws: entry q & 3 of rand4(seed, env, step, base + (q >> 2)) (oracle/task_ref.py)."""
    from oracle.task_ref import rand4

    N, q = env.num_envs, np.arange(p)
    u, g = rand4(int(env._cfg_c.seed), np.arange(N)[:, None], step, (base + (q >> 2))[None, :])
    return u[:, q, q & 3], g[:, q, q & 3]


def _noise_of(env):
    """(actor column - critic column) / S [N][P], float64."""
    torch.cuda.synchronize()
    F, S = env.scan_obs_offset, env.cfg["normalization"]["height_measurements"]
    return (env.obs_buf[:, F:].double() - env.privileged_obs_buf[:, 14:].double()).cpu().numpy() / S


def test_uniform_noise_is_the_oracle_generators_on_the_new_streams():
    """Values are at most 5.5 in magnitude (|clip| S + S 0.1), where the fp32 ulp is 4.8e-7; the difference of two of them divided by S = 5 carries
    a few roundings of that size (the product, the sum with a possible FMA contraction, apply_rand's own), well inside 1e-5."""
    from oracle.task_ref import apply_rand

    n = 256
    env, twin = _env(n), _env(n)
    spec = env.cfg["noise"]["height_measurements"]
    assert spec == {"range": [-0.1, 0.1], "operation": "additive", "distribution": "uniform"}

    def check(step, base, what):
        got = _noise_of(env)
        u, g = _draws(env, step, base, P)
        want = apply_rand(np.zeros((n, P)), spec, u.astype(np.float64), g.astype(np.float64))
        err = np.abs(got - want).max()
        print(f"{what}: max |noise - oracle| {err:.3e}, noise in [{got.min():.4f}, {got.max():.4f}]")
        assert err < 1e-5, (what, err)
        assert torch.equal(env.obs_buf, twin.obs_buf) and torch.equal(env.privileged_obs_buf, twin.privileged_obs_buf), what
        return got

    env.reset(); twin.reset()
    at_reset = check(0, RS_SCAN_RESET, "reset-all")
    assert np.abs(at_reset).max() <= 0.1 + 1e-5 and np.abs(at_reset).max() > 0.09
    for k in range(7):
        a = _actions(n, k, 0.3)
        env.step(a); twin.step(a)
        if k == 0:
            first = check(0, RS_SCAN, "step 1")  # the step counter is still 0: the reset-all's draws must not come back
            assert np.abs(first - at_reset).max() > 0.05 and np.abs(first - at_reset).mean() > 0.02
    assert env.common_step_counter == 7
    check(6, RS_SCAN, "step 7")


def test_gaussian_noise_has_its_moments_and_no_point_shares_a_draw():
    n, sigma = 256, 0.05
    env = _env(n, **{"noise.height_measurements": {"range": [0.0, sigma], "operation": "additive", "distribution": "gaussian"}})
    env.reset()
    env.step(_actions(n, 0, 0.3))
    x = _noise_of(env)
    u, g = _draws(env, 0, RS_SCAN, P)
    assert np.abs(x - sigma * g.astype(np.float64)).max() < 1e-5
    cnt = x.size
    assert cnt == 256 * 187
    print(f"mean {x.mean():.3e} (bound {5 * sigma / np.sqrt(cnt):.3e}), std {x.std():.6f} (bound +- {5 * sigma / np.sqrt(2 * cnt):.3e})")
    assert abs(x.mean()) <= 5 * sigma / np.sqrt(cnt)
    assert abs(x.std() - sigma) <= 5 * sigma / np.sqrt(2 * cnt)
    # no two points of an env share a draw: their addresses (stream, entry) are pairwise distinct, exactly, and the device's values were just shown
    # to be those draws' to 1e-5.  The issue asks that no two points share a VALUE; as fp32 numbers independent draws still coincide now and then
    # (the actor's column has an ulp of up to 4.8e-7, 1e-7 in these units: of the 187 x 186 / 2 pairs of an env about 17,391 x 1e-7 x 8, the density
    # of N(0, 0.05) at its mode, = 0.014 coincide, some 4 over the 256 envs), so the device-side count is held to 16, four times that expectation
    # (a Poisson tail below 1e-5), where points sharing a stream entry would coincide in at least half of all values (24,000)
    q = np.arange(P)
    assert len({(int(RS_SCAN + (k >> 2)), int(k & 3)) for k in q}) == P
    dup = sum(P - len(np.unique(x[e])) for e in range(n))
    print(f"coinciding values within an env, all envs: {dup}")
    assert dup <= 16, dup


# ------------------------------------------------------------------ 5. a ragged count through step_to
def test_ragged_env_count_through_step_to_writes_every_row_and_nothing_past_n():
    n, W = 200, 47 + P
    on, off = _env(n, **NO_NOISE), _env(n, actor=False)
    on.reset(); off.reset()
    rew, done, tout = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV)
    for k in range(3):
        a = _actions(n, k, 0.3)
        o0, _, d0, x0 = off.step(a)
        slab = torch.full((n + 7, W), float("nan"), device=DEV)  # a different destination at every step, as the rows of a rollout buffer
        pslab = torch.full((n + 7, 14 + P), float("nan"), device=DEV)
        on.step_to(a, slab[:n], pslab[:n], rew, done, tout)
        torch.cuda.synchronize()
        assert torch.isfinite(slab[:n]).all() and torch.isnan(slab[n:]).all() and torch.isfinite(pslab[:n]).all() and torch.isnan(pslab[n:]).all(), k
        assert torch.equal(slab[:n, :47], o0) and torch.equal(done, d0) and torch.equal(pslab[:n, :14], x0["privileged_obs"][:, :14]), k
        assert torch.equal(slab[:n, 47:], pslab[:n, 14:]), k
        assert np.abs(slab[:n, 47:].cpu().numpy() - _scan_ref(on)).max() < 1e-4, k
    with pytest.raises(RuntimeError, match="obs of 200 x 234"):
        on.step_to(a, torch.empty(n, 47, device=DEV), pslab[:n], rew, done, tout)


# ------------------------------------------------------------------ 6. the rollout actor
@pytest.mark.parametrize("K,scan", [(234, 187), (328, 187)])
def test_rollout_actor_of_a_perceptive_row_matches_float64(K, scan):
    """bg_actor_sample_mlp's kernel at a first layer that is no multiple of 47 (its 48-column k-chunks run over the frame boundaries and end inside a
    chunk: 234 = 4 x 48 + 42, 328 = 6 x 48 + 40), with tests/test_gpu_frame_stack.py's bound; the noise is bg_actor_sample's."""
    from test_gpu_frame_stack import _actor_f64, _zero_output_layer

    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(K)
    n = 128
    model, default = ActorCritic(12, K, 14 + scan).to(DEV), ActorCritic(12, 47, 14).to(DEV)
    with torch.no_grad():
        model.logstd.copy_(torch.linspace(-2.5, 0.5, 12, device=DEV).view(1, 12))
        default.logstd.copy_(model.logstd)
    obs = torch.randn(n, K, device=DEV)
    mu_buf, act_buf = torch.full((n + 16, 12), 7.0, device=DEV), torch.full((n + 16, 12), 7.0, device=DEV)
    model.sample_actions(obs, act_buf[:n], 1234567, 17, mu_out=mu_buf[:n], scan=scan)
    ref = _actor_f64(model, obs)
    err = (mu_buf[:n].double() - ref).abs().max().item()
    print(f"K {K}: max error {err:.3e}, |ref|max {ref.abs().max().item():.3f}")
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (K, err)
    assert torch.all(mu_buf[n:] == 7.0) and torch.all(act_buf[n:] == 7.0), "rows past N were written"
    # every input column counts: the last one, too (a k-chunk that stopped short of K would lose it)
    obs2 = obs.clone(); obs2[:, K - 1] += 1.0
    mu2 = torch.empty(n, 12, device=DEV)
    model.sample_actions(obs2, torch.empty(n, 12, device=DEV), 1234567, 17, mu_out=mu2, scan=scan)
    assert (mu2.double() - _actor_f64(model, obs2)).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item()) and not torch.equal(mu2, mu_buf[:n])
    _zero_output_layer(model); _zero_output_layer(default)
    a_new, a_old = torch.empty(n, 12, device=DEV), torch.empty(n, 12, device=DEV)
    model.sample_actions(obs, a_new, 1234567, 17, scan=scan)
    default.sample_actions(obs[:, :47].contiguous(), a_old, 1234567, 17)
    assert torch.equal(a_new, a_old), "the noise differs from bg_actor_sample's"
    # a width that is not 47 H + scan, or beyond the LDS tile, stays an argument error
    lib, o = _lib.load(), torch.zeros(4, 600, device=DEV)
    for k_in, sc in ((234, 186), (47 * 10 + 14, 14), (47 + 1025, 1025)):
        descs = (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(16, 16, k_in, 128), _lib.MlpLayerDesc(16, 16, 128, 128), _lib.MlpLayerDesc(16, 16, 128, 12))
        assert lib.bg_actor_sample_mlp_scan(4, _lib.ptr(o), 3, descs, sc, _lib.ptr(o), 0, 0, None, _lib.ptr(o), None) < 0, (k_in, sc)


# ------------------------------------------------------------------ 7. training
def _runner(n, H=1, actor=True, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    ov = _ov(n, H, actor, **{"runner.mini_epochs": 3, "runner.horizon_length": 24})
    ov.update(over)
    return Runner(cfg=load_cfg("T1", ov))


def _start(r):
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])


def _second_iteration(r):
    """Iteration 1 as the runner makes it, then the rollout of iteration 2 with the Adam state cleared, so that a restatement's fresh torch.optim.Adam
    starts where the runner does (tests/test_gpu_mini_batches.py compares its combined case the same way)."""
    _start(r)
    r.iteration()
    opt = r.optimizer
    opt.exp_avg.zero_(); opt.exp_avg_sq.zero_(); opt.step_count = 0; opt.lr.fill_(1e-5)
    r.invalidate()
    r.rollout()


def test_update_matches_the_reference_loop_plain():
    from test_gpu_mini_batches import compare_with_reference

    from booster_gym_amd.utils.model import ActorCritic
    from oracle.ppo_ref import ppo_update_reference

    E, T, n = 3, 24, 128
    r = _runner(n)
    assert r.model.actor[0].in_features == 234 and r.model.critic[0].in_features == 435
    assert r._actor_in.shape[-1] == 256 and r._critic_in.shape[-1] == 512
    plan = r._resolve_plan()
    assert plan.actor.fwd == "layer" and plan.actor.bwd == "layer" and plan.critic.fwd == "layer" and not plan.ahead and plan.fused_head
    _second_iteration(r)
    ref_model = ActorCritic(12, 234, 201).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    assert tuple(b["obses"].shape) == (T + 1, n, 234) and b["obses"][:, :, 47:].std() > 1e-3
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


def test_update_matches_the_reference_loop_with_normalisation_mini_batches_and_a_frame_stack():
    from test_gpu_mini_batches import compare_with_reference, device_batches, reference_update_with_mini_batches

    from booster_gym_amd.utils.model import ActorCritic

    E, T, n, K, H = 3, 24, 128, 2, 3
    r = _runner(n, H, **{"runner.num_mini_batches": K, "algorithm.empirical_normalization": True})
    no, npv = r.env.num_obs, r.env.num_privileged_obs
    assert (no, npv) == (141 + 45, 59) and r._actor_in.shape[-1] == 256 and r._critic_in.shape[-1] == 256
    _second_iteration(r)
    assert r._mb_plan.critic.fwd == r._mb_plan.actor.fwd == "layer"
    norm = r.obs_norm
    ref_model = ActorCritic(12, no, npv).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    hn = lambda x: (x - norm.mean_dev[:no]) * norm.inv_std_dev[:no]
    hp = lambda x: (x - norm.mean_dev[no : no + npv]) * norm.inv_std_dev[no : no + npv]
    batches = device_batches(r, E, K)
    stats_ref, lr_ref = reference_update_with_mini_batches(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), hn(b["obses"][:T]), hp(b["privileged_obses"][:T]),
                                                           b["actions"].clone(), b["rewards"].clone(), b["dones"].clone(), b["time_outs"].clone(), hn(b["obses"][T]),
                                                           hp(b["privileged_obses"][T]), batches)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    acc = r.update()
    torch.cuda.synchronize()
    assert norm.count == 2 * T * n
    compare_with_reference(r, ref_model, stats_ref, lr_ref, p_start, acc)


def test_update_matches_the_reference_loop_with_the_symmetry_loss():
    from test_gpu_mini_batches import assert_same_adam_steps
    from test_gpu_symmetry import ppo_update_sym_reference

    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.utils import mirror_rows

    E, T, n = 3, 24, 128
    r = _runner(n, **{"algorithm.symmetry_loss": True})
    src, sign = r._obs_mirror
    assert len(src) == 256 and src[47:234] == [47 + int(s) for s in r.env.mirror_maps()[0][47:] - 47] and all(s == 1.0 for s in sign[47:])
    x = torch.randn(40, 256, device=DEV); x[:, 234:] = 0.0
    y = torch.full_like(x, float("nan"))
    mirror_rows(x, y, src, sign)  # the scan block on the device: point (x_i, y_j) takes (x_i, -y_j)
    assert torch.equal(y[:, 47:234].reshape(40, 17, 11), x[:, 47:234].reshape(40, 17, 11).flip(2)) and not y[:, 234:].any()
    _second_iteration(r)
    ref_model = ActorCritic(12, 234, 201).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    stats_ref, lr_ref = ppo_update_sym_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), b["obses"][:T].clone(),
                                                 b["privileged_obses"][:T].clone(), b["actions"].clone(), b["rewards"].clone(), b["dones"].clone(),
                                                 b["time_outs"].clone(), b["obses"][T].clone(), b["privileged_obses"][T].clone(), r.env.mirror_maps(),
                                                 mini_epochs=E, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    summ = r._summarize(r.update())
    for (k, p), (k2, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        assert k == k2
        assert_same_adam_steps(k, p, q, p_start[k])
        assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    assert stats_ref["symmetry_loss"] > 0
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean", "symmetry_loss"):
        print(f"{k}: {summ[k]!r} against {stats_ref[k]!r}")
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9


def test_asymmetric_grid_with_the_symmetry_loss_is_a_value_error_in_the_runner():
    ys = [-0.2, -0.1, 0.0, 0.1]
    with pytest.raises(ValueError, match=r"algorithm\.symmetry_loss.*terrain\.actor_heights.*terrain\.measured_points_y"):
        _runner(128, **{"algorithm.symmetry_loss": True, "terrain.measured_points_x": [0.0, 0.1], "terrain.measured_points_y": ys,
                        "env.num_observations": 47 + 8, "env.num_privileged_obs": 14 + 8})


# ------------------------------------------------------------------ 8. checkpoint and export
class _Rec:
    def __init__(self):
        self.stats = {}

    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        return None


def _train(r, iters):
    rec = _Rec()
    r.begin_training(recorder=rec)
    for it in range(iters):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    return rec


def test_checkpoint_round_trip_height_points_width_mismatch_and_export(tmp_path):
    from booster_gym_amd.utils.model import ActorCritic

    r = _runner(128, **{"runner.mini_epochs": 2})
    rec = _train(r, 2)
    assert len(rec.stats) == 2 and all(np.isfinite(float(v)) for s in rec.stats.values() for v in s.values())
    d = r.checkpoint_dict()
    assert tuple(d["height_points"].shape) == (P, 2) and torch.equal(d["height_points"], r.env.height_points)
    ck = str(tmp_path / "model_2.pth")
    torch.save(d, ck)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r
    r2 = _runner(128, **{"runner.mini_epochs": 2, "basic.checkpoint": ck})
    for k, v in r2.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    _train(r2, 1)
    del r2
    # the key off (the critic's scan still on): named before any guess at a frame stack
    with pytest.raises(ValueError, match=r"234 inputs, 187 of them.*takes 47.*terrain\.actor_heights"):
        _runner(128, actor=False, **{"basic.checkpoint": ck})
    r0 = _runner(128, actor=False, **{"runner.mini_epochs": 2})
    d0 = r0.checkpoint_dict()
    assert "height_points" not in d0
    ck0 = str(tmp_path / "model_off.pth")
    torch.save(d0, ck0)
    del r0
    with pytest.raises(ValueError, match=r"47 inputs, 0 of them.*takes 234.*terrain\.actor_heights"):
        _runner(128, **{"basic.checkpoint": ck0})

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={ck}"], cwd=str(tmp_path), env=env, check=True,
                         timeout=300, capture_output=True, text=True).stdout
    assert "47 x 1 observations, then 187 heights, grid" in out, out
    actor = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    m = ActorCritic(12, 234, 201)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    x = torch.linspace(-1, 1, 234).reshape(1, 234)
    y = actor(x)
    assert tuple(y.shape) == (1, 12) and torch.allclose(y, m.actor(x), atol=1e-6)


# ------------------------------------------------------------------ 9. the off switch
def test_key_false_equals_key_absent_bitwise_in_the_env_and_in_two_iterations():
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    def cfg(absent, **over):
        c = load_cfg("T1", {"env.num_envs": 128, "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.mini_epochs": 2, **over})
        assert c["terrain"]["actor_heights"] is False
        if absent:
            del c["terrain"]["actor_heights"], c["noise"]["height_measurements"]
        return c

    envs = [T1(cfg(absent)) for absent in (False, True)]
    assert all(e.num_scan_obs == 0 and e.scan_obs_offset == 47 and e._cfg_c.actor_heights == 0 and tuple(e.obs_buf.shape) == (128, 47) for e in envs)
    outs = [[t.clone() for t in (e.reset()[0], e.extras["privileged_obs"])] for e in envs]
    for k in range(12):
        a = _actions(128, k)
        for e, o in zip(envs, outs):
            obs, rew, done, extras = e.step(a)
            o.extend(t.clone() for t in (obs, rew, done, extras["time_outs"], extras["privileged_obs"]))
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(x, y) for x, y in zip(*outs))
    del envs

    runs = []
    for absent in (False, True):
        r = Runner(cfg=cfg(absent, **{"terrain.type": "plane"}))
        rec = _train(r, 2)
        runs.append(({k: v.clone() for k, v in r.model.state_dict().items()}, {k: r.buffer[k].clone() for k in ("obses", "privileged_obses", "actions", "rewards", "dones")},
                     rec.stats, "height_points" in r.checkpoint_dict()))
        del r
    (p0, b0, s0, h0), (p1, b1, s1, h1) = runs
    assert not h0 and not h1
    assert p0.keys() == p1.keys() and all(torch.equal(p0[k], p1[k]) for k in p0)
    assert all(torch.equal(b0[k], b1[k]) for k in b0)
    assert s0.keys() == s1.keys() and all(s0[it].keys() == s1[it].keys() for it in s0)
    for it in s0:
        for k in s0[it]:
            x, y = s0[it][k], s1[it][k]
            assert (torch.equal(torch.as_tensor(x), torch.as_tensor(y))) or (x != x and y != y), (it, k, x, y)
