"""Empirical observation normalisation on the GPU (algorithm.empirical_normalization): bg_obs_moments and bg_obs_normalize against float64,
off is off, one iteration against oracle/ppo_ref.py on host-normalised inputs, the statistics of three iterations, the first ratio, the checkpoint
round trip and play()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 187
EPS64 = float(np.finfo(np.float64).eps)
U32 = 2.0 ** -23  # the spacing of fp32 relative to a value (bound of one rounding: half of it)
KEY = "algorithm.empirical_normalization"


def _ov(n, H=1, scan=False, **over):
    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV, "terrain.type": "plane"}
    if H != 1:
        ov.update({"env.frame_stack": H, "env.num_observations": 47 * H})
    if scan:
        ov.update({"terrain.type": "trimesh", "terrain.measure_heights": True, "env.num_privileged_obs": 14 + P})
    ov.update(over)
    return ov


def _runner(n, H=1, scan=False, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    return Runner(cfg=load_cfg("T1", _ov(n, H, scan, **over)))


def _start(r):
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])


# ------------------------------------------------------------------ bg_obs_moments
def _moments(a, b):
    """bg_obs_moments on the column blocks a [M, ca] / b [M, cb] or None (views with their own row strides) -> (sum, sumsq) float64 numpy."""
    from booster_gym_amd import _lib

    M, ca = a.shape
    cb = 0 if b is None else b.shape[1]
    C = ca + cb
    out = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.full((_lib.OBS_MOMENTS_MAX_GROUPS * 2 * C,), float("nan"), dtype=torch.float64, device=DEV)
    assert a.stride(1) == 1 and (b is None or b.stride(1) == 1)
    _lib.check(_lib.load().bg_obs_moments(M, _lib.ptr(a), ca, a.stride(0), _lib.ptr(b), cb, 0 if b is None else b.stride(0), _lib.ptr(out), _lib.ptr(out[C:]),
                                          _lib.ptr(scratch), _lib.current_stream_ptr()), "bg_obs_moments")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:C], o[C:]


def _check_moments(a, b, what):
    """Against numpy float64.  Bound: every input is exact in float64 and so is its square (24-bit x 24-bit); each of the M - 1 additions of a
    column's sum rounds at eps_f64 / 2 relative to the partial sum, which never exceeds sum |x| (sum x^2), whatever the fixed order: |error| <=
    M eps_f64 sum |x|, and M eps_f64 sum x^2; numpy's pairwise sum lies inside the same bound.  Two launches on the same input: the same bits."""
    x = torch.cat((a, b), dim=1) if b is not None else a
    x64 = x.detach().cpu().double().numpy()
    M = x64.shape[0]
    s, ss = _moments(a, b)
    s2, ss2 = _moments(a, b)
    assert np.array_equal(s, s2) and np.array_equal(ss, ss2), what
    bs, bss = M * EPS64 * np.abs(x64).sum(0), M * EPS64 * (x64 * x64).sum(0)
    es, ess = np.abs(s - x64.sum(0)), np.abs(ss - (x64 * x64).sum(0))
    print(f"{what}: M {M} C {x64.shape[1]}: worst sum error / bound {np.max(es / np.maximum(bs, 1e-300)):.3e}, sumsq {np.max(ess / np.maximum(bss, 1e-300)):.3e}")
    assert (es <= bs).all() and (ess <= bss).all(), what
    return s, ss


def test_moments_of_random_rows_with_spread_scales():
    g = torch.Generator(device=DEV).manual_seed(3)
    for M, ca, cb in ((4096 * 24, 47, 14), (5000, 141, 201), (3001, 512, 201), (777, 300, 0), (4 * 32 + 5, 94, 14), (1, 47, 14), (31, 64, 64)):
        C = ca + cb
        scale = 10.0 ** torch.linspace(-3, 3, C, device=DEV)[torch.randperm(C, device=DEV, generator=g)]
        offset = scale * torch.randn(C, device=DEV, generator=g) * 3
        x = offset + scale * torch.randn(M, C, device=DEV, generator=g)
        a = x[:, :ca].contiguous()
        b = x[:, ca:].contiguous() if cb else None
        _check_moments(a, b, f"random rows {M} x ({ca} + {cb})")
    # blocks that are column ranges of wider rows (row strides beyond the blocks' columns)
    wide = torch.randn(1000, 300, device=DEV, generator=g)
    _check_moments(wide[:, 3:50], wide[:, 100:114], "strided blocks")


def test_moments_of_real_rollout_rows_with_stack_and_scan():
    r = _runner(256, 3, scan=True, **{"runner.mini_epochs": 1})
    _start(r)
    r.rollout()
    torch.cuda.synchronize()
    T = r.cfg["runner"]["horizon_length"]
    obs, priv = r.buffer["obses"][:T].reshape(T * 256, 141), r.buffer["privileged_obses"][:T].reshape(T * 256, 14 + P)
    assert obs.stride(0) == 141 and priv.stride(0) == 201  # two column blocks with different strides
    s, ss = _check_moments(obs, priv, "rollout rows, frame_stack 3 + height scan")
    assert np.abs(s).max() > 0


# ------------------------------------------------------------------ bg_obs_normalize
def _norm_bound(x64, mean32, inv32):
    """y = fl(fl(x - mean) * inv_std): the subtract rounds at 2^-24 |x - mean| <= 2^-24 (|x| + |mean|) and is then scaled by |inv_std|; the multiply
    rounds at 2^-24 |y|.  Stated with 2^-23 (twice the worst case of round-to-nearest, covering the second-order term):
        |err| <= 2^-23 (|x| + |mean|) |inv_std| + 2^-23 |y|."""
    m, i = mean32.astype(np.float64), inv32.astype(np.float64)
    y = (x64 - m) * i
    return y, U32 * (np.abs(x64) + np.abs(m)) * np.abs(i) + U32 * np.abs(y)


def _trained(cols, seed=1):
    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    rng = np.random.default_rng(seed)
    norm = ObsNormalizer(cols, 1.0e-2, DEV)
    mean, std = rng.uniform(-3, 3, cols) * 10.0 ** rng.uniform(-2, 2, cols), 10.0 ** rng.uniform(-3, 2, cols)
    norm.merge(mean, std * std, 1000)
    return norm, mean, std


def test_normalize_every_form_the_runner_uses():
    norm, mean, std = _trained(141 + 201)
    no, npv, N, T = 141, 201, 128, 5
    rng = np.random.default_rng(2)
    obs = torch.from_numpy((mean[:no] + std[:no] * rng.standard_normal((T + 1, N, no))).astype(np.float32)).to(DEV)
    priv = torch.from_numpy((mean[no:] + std[no:] * rng.standard_normal((T + 1, N, npv))).astype(np.float32)).to(DEV)
    obs0, priv0 = obs.clone(), priv.clone()
    o64, p64 = obs.cpu().double().numpy(), priv.cpu().double().numpy()
    yo, bo = _norm_bound(o64, norm.mean32[:no], norm.inv_std32[:no])
    yp, bp = _norm_bound(p64, norm.mean32[no:], norm.inv_std32[no:])

    def close(got, want, bound, what):
        err = np.abs(got.cpu().double().numpy() - want)
        print(f"{what}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all(), what

    # the rollout form: one step's [N][num_obs] rows into a dense scratch
    scratch = torch.full((N, no), float("nan"), device=DEV)
    norm.normalize_into(obs[2], scratch)
    close(scratch, yo[2], bo[2], "rollout form")
    # the update form: the padded critic input (observation block, then the privileged block with the padding behind it) and the actor input
    ci = torch.full((T + 1, N, 512), float("nan"), device=DEV)
    norm.normalize_into(obs, ci[:, :, :no])
    norm.normalize_into(priv, ci[:, :, no:], col0=no, dst_cols=512 - no)
    close(ci[:, :, :no], yo, bo, "critic input, observation block")
    close(ci[:, :, no : no + npv], yp, bp, "critic input, privileged block")
    assert torch.equal(ci[:, :, no + npv :], torch.zeros_like(ci[:, :, no + npv :]))  # the padded columns: exactly 0.0
    ai = torch.full((T, N, 256), float("nan"), device=DEV)
    norm.normalize_into(obs[:T], ai, dst_cols=256)
    assert torch.equal(ai[:, :, no:], torch.zeros_like(ai[:, :, no:]))
    assert torch.equal(ai[2, :, :no], scratch) and torch.equal(ci[2, :, :no], scratch)  # the rollout form and the update forms: the same bits
    # the forward-ahead form: a range of steps of the same tensors
    ci2 = torch.zeros_like(ci)
    norm.normalize_into(obs[1:3], ci2[1:3, :, :no])
    norm.normalize_into(priv[1:3], ci2[1:3, :, no:], col0=no, dst_cols=512 - no)
    assert torch.equal(ci2[1:3], ci[1:3]) and not ci2[0].any() and not ci2[3:].any()
    # the mirrored rows: a dense [B][num_obs] source into rows of the padded actor input
    flat = obs[:T].reshape(T * N, no)
    dst = torch.full((T * N, 256), float("nan"), device=DEV)
    norm.normalize_into(flat, dst, dst_cols=256)
    assert torch.equal(dst, ai.reshape(T * N, 256))
    torch.cuda.synchronize()
    assert torch.equal(obs, obs0) and torch.equal(priv, priv0)  # the source is untouched


# ------------------------------------------------------------------ the runner
class _Rec:
    def __init__(self):
        self.stats = {}

    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        return None


def _train(r, iters, first=0, begin=True):
    if begin:
        r.begin_training(recorder=_Rec())
    for it in range(first, first + iters):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    return r.recorder


def _count_calls(monkeypatch):
    from booster_gym_amd import _lib

    lib, counts = _lib.load(), {"bg_obs_moments": 0, "bg_obs_normalize": 0}
    for name in counts:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


def test_off_is_off(monkeypatch):
    """Key absent and key false: the same bits in every parameter, buffer and log scalar after two iterations, no new log or checkpoint name, and
    neither new entry point is called."""
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    counts = _count_calls(monkeypatch)
    res = []
    for absent in (True, False):
        cfg = load_cfg("T1", _ov(256, **{"runner.mini_epochs": 3, "basic.seed": 5}))
        if absent:
            del cfg["algorithm"]["empirical_normalization"], cfg["algorithm"]["normalization_eps"]
        else:
            assert cfg["algorithm"]["empirical_normalization"] is False
        r = Runner(cfg=cfg)
        assert r.obs_norm is None and not hasattr(r, "_obs_normed")
        rec = _train(r, 2)
        assert sorted(r.checkpoint_dict()) == ["curriculum", "model", "optimizer"]
        assert not any(k.startswith("obs_norm") for s in rec.stats.values() for k in s)
        res.append(([r.optimizer.flat.clone(), r.optimizer.exp_avg.clone(), r.optimizer.exp_avg_sq.clone(), r.optimizer.lr.clone(), r.buffer["obses"].clone(),
                     r.buffer["privileged_obses"].clone(), r.buffer["actions"].clone(), r.buffer["rewards"].clone(), r._critic_in.clone(), r._actor_in.clone(),
                     r._old_logp.clone()], rec.stats))
        del r
    for k, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        assert torch.equal(a, b), k
    assert res[0][1] == res[1][1] and len(res[0][1]) == 2
    assert counts == {"bg_obs_moments": 0, "bg_obs_normalize": 0}


def _assert_same_adam_steps(name, p, q, start):
    """As in test_gpu_ppo: all but 0.5 % of the elements within 2 % of the distance the tensor's parameters moved, none further than twice that."""
    moved = (q - start).abs().max().item()
    d = (p - q).abs()
    off = (d > 0.02 * moved + 2e-6).float().mean().item()
    assert off <= 0.005 and d.max().item() <= 2.0 * moved + 2e-6, (name, off, d.max().item(), moved)


def _host_normalise(norm, x, col0=0):
    """(x - mean) * inv_std in fp32 torch on the device from the runner's fp32 copies: the same two roundings as the kernel."""
    c = x.shape[-1]
    return (x - norm.mean_dev[col0 : col0 + c]) * norm.inv_std_dev[col0 : col0 + c]


@pytest.mark.parametrize("H,scan", [(1, False), (3, True)])
def test_second_iteration_matches_reference_loop_on_host_normalised_inputs(H, scan):
    """Iteration 2 (after one statistics update, so the statistics are not the initial ones) against oracle/ppo_ref.ppo_update_reference fed the
    buffers normalised on the host with the runner's statistics.  The Adam state of iteration 1 is cleared before (and the runner told so with
    invalidate()), so that the oracle's fresh torch.optim.Adam starts where the runner does.  Tolerances: those of tests/test_gpu_ppo.py and
    tests/test_gpu_frame_stack.py for the same comparison."""
    from booster_gym_amd.utils.model import ActorCritic
    from oracle.ppo_ref import ppo_update_reference

    E, T, n = 3, 24, 256
    r = _runner(n, H, scan, **{"runner.mini_epochs": E, KEY: True})
    no, npv = r.env.num_obs, r.env.num_privileged_obs
    assert (no, npv) == (47 * H, 14 + (P if scan else 0)) and r.obs_norm.cols == no + npv
    _start(r)
    r.iteration()
    norm = r.obs_norm
    assert norm.count == T * n and np.abs(norm.mean).max() > 0
    opt = r.optimizer
    opt.exp_avg.zero_(); opt.exp_avg_sq.zero_(); opt.step_count = 0; opt.lr.fill_(1e-5)
    r.invalidate()
    r.rollout()
    ref_model = ActorCritic(12, no, npv).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    rewards_ref = b["rewards"].clone()
    hn = lambda x: _host_normalise(norm, x)
    hp = lambda x: _host_normalise(norm, x, no)
    stats_ref, lr_ref = ppo_update_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), hn(b["obses"][:T]), hp(b["privileged_obses"][:T]),
                                             b["actions"].clone(), rewards_ref, b["dones"].clone(), b["time_outs"].clone(), hn(b["obses"][T]),
                                             hp(b["privileged_obses"][T]), mini_epochs=E, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    raw = b["obses"].clone()
    want_in = hn(raw)  # (with the statistics of the rollout: update() changes them when it ends)
    acc = r.update()
    torch.cuda.synchronize()
    assert torch.equal(b["obses"], raw)  # the buffer keeps the raw rows
    assert torch.equal(r._critic_in[:, :, :no], want_in) and not r._critic_in[:, :, no + npv :].any()  # ... and the networks read the normalised ones
    assert norm.count == 2 * T * n
    summ = r._summarize(acc)
    for (k, p), (k2, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        assert k == k2
        print(f"{k}: max |p - q| {(p - q).abs().max().item():.3e}, moved {(q - p_start[k]).abs().max().item():.3e}")
        _assert_same_adam_steps(k, p, q, p_start[k])
        assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean"):
        print(f"{k}: {summ[k]!r} against {stats_ref[k]!r}")
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9


def test_symmetry_loss_mirrors_raw_rows_and_normalises_them_with_the_same_statistics():
    """_actor_in[T:] = normalise(M_o x), what the policy computes on the mirrored raw observation -- not the mirror of the normalised rows (the
    statistics of a left and a right joint differ)."""
    r = _runner(256, **{"runner.mini_epochs": 2, KEY: True, "algorithm.symmetry_loss": True})
    _start(r)
    r.iteration()
    r.rollout()
    T, B, no = 24, 24 * 256, 47
    stats_before = (r.obs_norm.mean32.copy(), r.obs_norm.inv_std32.copy())
    raw = r.buffer["obses"][:T].reshape(B, no).clone()
    # update() builds the inputs first and changes the statistics last: capture the inputs through the plan's own entry
    u = r._update_begin(r._resolve_plan())
    torch.cuda.synchronize()
    src, sign = np.array(r._obs_mirror_raw[0]), np.array(r._obs_mirror_raw[1])
    mirrored = sign * raw.cpu().double().numpy()[:, src]
    want, bound = _norm_bound(mirrored, stats_before[0][:no], stats_before[1][:no])
    got = r._actor_in[T:].reshape(B, -1)
    err = np.abs(got[:, :no].cpu().double().numpy() - want)
    print(f"mirrored rows: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all() and not got[:, no:].any()
    first = r._actor_in[:T].reshape(B, -1)[:, :no]
    assert torch.equal(first, _host_normalise(r.obs_norm, raw))
    assert np.array_equal(r.obs_norm.mean32, stats_before[0])  # (nothing above has changed the statistics)
    wrong = sign * first.cpu().double().numpy()[:, src]  # the mirror of the normalised rows: a different thing
    assert np.abs(wrong - want).max() > 1e-3
    del u
    r.invalidate()
    acc = r.update()
    torch.cuda.synchronize()
    assert torch.isfinite(acc).all() and torch.isfinite(r.optimizer.flat).all()


def test_statistics_after_three_iterations_equal_the_host_merge_of_the_rollouts():
    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    n, T = 256, 24
    r = _runner(n, **{"runner.mini_epochs": 2, KEY: True})
    _start(r)
    host = ObsNormalizer(61)
    for it in range(3):
        r.rollout()
        rows = torch.cat((r.buffer["obses"][:T], r.buffer["privileged_obses"][:T]), dim=-1).reshape(T * n, 61).cpu().double().numpy()
        r.update()
        r.buffer.roll()
        host.merge(rows.mean(0), rows.var(0), rows.shape[0])
    assert r.obs_norm.count == 3 * T * n == host.count
    # the device's sums carry M eps_f64 sum|x| / sum x^2 (the moments bound); through mean = s / M and var = ss / M - mean^2 that is at most
    # M eps_f64 (mean|x|) on the mean and M eps_f64 (mean x^2 + 2 |mean| mean|x|) <= 3 M eps_f64 mean x^2 on a batch's variance; three merges of a
    # few float64 operations each add 64 eps_f64 x 3 x max(var, mean^2) (tests/test_obs_norm.py)
    M = T * n
    ex2 = host.var + host.mean**2
    b_mean = 3 * M * EPS64 * np.sqrt(ex2) + 64 * 3 * EPS64 * np.sqrt(ex2)
    b_var = 3 * 3 * M * EPS64 * ex2 + 64 * 3 * EPS64 * ex2
    e_mean, e_var = np.abs(r.obs_norm.mean - host.mean), np.abs(r.obs_norm.var - host.var)
    print(f"mean: worst error / bound {np.max(e_mean / np.maximum(b_mean, 1e-300)):.3e}; var: {np.max(e_var / np.maximum(b_var, 1e-300)):.3e}")
    assert (e_mean <= b_mean).all() and (e_var <= b_var).all()


def test_first_ratio_is_what_it_is_without_the_feature():
    """runner.mini_epochs: 1: the logged kl_mean is the divergence between the old policy and the policy of mini-epoch 0 -- the same weights on the
    same normalised bits, so the means agree exactly and what is left is the rounding of the log-std terms of the KL formula (~1e-8, not 0.0: a
    function of the log-std alone, the same for every row).  It must be the value a key-false runner logs under that setting FROM THE SAME
    WEIGHTS: the key-false runner is handed the key-true runner's weights in front of every iteration (the two train differently, so their own
    weights part after the first update).  A normaliser whose rollout and update forms differed in a bit, or statistics that moved between the
    rollout and the update, would put (mu - old_mu)^2 / sigma^2 on top: with sigma = e^-2 a last-bit difference of the means shows as ~1e-12
    per row against a value that is otherwise reproduced bit for bit."""
    for ahead in (True, False):  # the forward passes during the rollout, and at the start of update()
        on = _runner(256, **{"runner.mini_epochs": 1, KEY: True, "basic.seed": 3})
        off = _runner(256, **{"runner.mini_epochs": 1, "basic.seed": 3})
        for r in (on, off):
            r._rollout_forward = ahead
            r.begin_training(recorder=_Rec())
        assert on._resolve_plan().ahead == ahead
        for it in range(3):
            off.model.load_state_dict(on.model.state_dict())
            off.invalidate()
            on.train_iteration(it)
            off.train_iteration(it)
        for r in (on, off):
            r._flush_log()
        torch.cuda.synchronize()
        s_on, s_off = on.recorder.stats, off.recorder.stats
        kl_on, kl_off = [s_on[it]["kl_mean"] for it in range(3)], [s_off[it]["kl_mean"] for it in range(3)]
        print(f"forward passes during the rollout {ahead}: kl_mean with the key {kl_on}, without {kl_off}")
        assert kl_on == kl_off
        assert [s_on[it]["obs_norm/count"] for it in range(3)] == [24.0 * 256 * (it + 1) for it in range(3)]
        assert all(np.isfinite(s_on[it]["obs_norm/max_abs_mean"]) and s_on[it]["obs_norm/min_std"] >= 0 for it in range(3))
        assert not any(k.startswith("obs_norm") for k in s_off[0])
        assert s_on[2]["value_loss"] != s_off[2]["value_loss"]  # (the two runs do differ: the inputs are normalised in one of them)
        del on, off


def test_forward_ahead_with_frozen_statistics_changes_no_bit():
    res = []
    for ahead in (True, False):
        r = _runner(256, **{"runner.mini_epochs": 3, KEY: True, "basic.seed": 7})
        assert r._rollout_forward
        r._rollout_forward = ahead
        _start(r)
        for _ in range(2):
            stats = r.iteration().clone()
        torch.cuda.synchronize()
        res.append((r.optimizer.flat.clone(), r.optimizer.exp_avg_sq.clone(), stats, r._old_logp.clone(), r._critic_in.clone(), r._actor_in.clone(),
                    torch.from_numpy(r.obs_norm.var)))
        del r
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_checkpoint_round_trip_and_play(tmp_path):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    over = {"runner.mini_epochs": 2, KEY: True, "basic.seed": 9}
    r = _runner(256, **over)
    _train(r, 2)
    ck = str(tmp_path / "model_2.pth")
    torch.save(r.checkpoint_dict(), ck)
    # the env's state is not part of a checkpoint, so "the next iteration" is the next update on one fixed batch: the uninterrupted runner's
    # against the reloaded runner's
    batch = {k: r.buffer[k].clone() for k in ("obses", "privileged_obses", "actions", "rewards", "dones", "time_outs")}

    def next_update(q):
        for k, v in batch.items():
            q.buffer[k].copy_(v)
        q.invalidate()
        acc = q.update().clone()
        torch.cuda.synchronize()
        return acc, q.optimizer.flat.clone(), q._critic_in.clone(), q.obs_norm.mean.copy(), q.obs_norm.var.copy(), q.obs_norm.count

    def first_rollout(q):
        """One rollout() from a common first observation with a common action counter: the env's state is not part of a checkpoint, so the later
        steps differ, but step 0 -- the rows bg_obs_normalize hands the sampling kernel, the sampled actions, and the forward-ahead's inputs, old
        means and values of those rows -- reads only the observation, the weights and the normaliser's device copies."""
        q.env.reset()
        q.buffer["obses"][0].copy_(batch["obses"][0]); q.buffer["privileged_obses"][0].copy_(batch["privileged_obses"][0])
        q._act_counter = 1000
        q.invalidate()
        assert q._resolve_plan().ahead
        q.rollout()
        torch.cuda.synchronize()
        n = q.env.num_envs
        return (q.buffer["actions"][0].clone(), q._critic_in[0].clone(), q._actor_in[0].clone(), q._old_mu[:n].clone(), q._values_all[:n].clone(),
                q._old_logp[:n].clone())

    r._lr_restart = True  # what a restored runner does on its first optimiser step (reference resume semantics): the same on both sides
    want_first = first_rollout(r)
    want = next_update(r)
    del r
    p = Runner(test=True, cfg=load_cfg("T1", _ov(256, **dict(over, **{"basic.checkpoint": ck}))))
    got_first = first_rollout(p)
    for k, (a, b) in enumerate(zip(want_first, got_first)):
        assert torch.equal(a, b), k
    assert (got_first[2][:, :47] - batch["obses"][0]).abs().max().item() > 1e-3  # (normalised rows, not the raw ones)
    got = next_update(p)
    for a, b in zip(want[:3], got[:3]):
        assert torch.equal(a, b)
    assert np.array_equal(want[3], got[3]) and np.array_equal(want[4], got[4]) and want[5] == got[5] == 3 * 24 * 256
    # play(): the actor is fed normalised rows
    seen = {}
    actor = p.model.actor
    orig = actor.forward

    def spy(x):
        seen.setdefault("x", x.clone())
        y = orig(x)
        seen.setdefault("y", y.clone())
        return y
    actor.forward = spy
    env_reset = p.env.reset

    def reset():
        o, infos = env_reset()
        seen["raw"] = o.clone()
        return o, infos
    p.env.reset = reset
    assert p.play(max_steps=3) == 3
    x = _host_normalise(p.obs_norm, seen["raw"])
    assert torch.equal(seen["x"], x)  # the first rows the actor saw: the normalised first observation
    with torch.no_grad():
        want_act = orig(x)
    assert (seen["y"] - want_act).abs().max().item() < 1e-5
    assert (x - seen["raw"]).abs().max().item() > 1e-3  # the rows did change: the statistics are not the identity
    del p
    with pytest.raises(ValueError, match=r"carries an observation normaliser but the config has algorithm\.empirical_normalization: false"):
        _runner(256, **{"basic.checkpoint": ck})
