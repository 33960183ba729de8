"""The action-smoothness loss on real kernels (algorithm.smoothness_loss): bg_partner_rows against the numpy restatement of tests/test_smoothness.py,
bg_actor_head_sym on the identity action map against float64 autograd, Runner.update() against the reference loop plus the term, two ranks,
reproducibility, the key off, and what the loss does to a policy."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_ppo import _assert_same_adam_steps
from test_gpu_symmetry import _head_ref
from test_smoothness import partner_draw, partner_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (list(range(12)), [1.0] * 12)
LOSSES = ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean", "smoothness_loss")


# ------------------------------------------------------------------ bg_partner_rows
SHAPES = [(1, 5, 64), (3, 37, 64), (5, 128, 256), (24, 100, 128)]
GUARD = 7.0


def _case(T, N, cols, flags, seed=0):
    """x, x_last with columns 0 / 1 laid out so that u can be read back: in column t % 2 a row of step t holds 0 and its successor 1."""
    rng = np.random.default_rng(1000 * T + N + cols + seed)
    x, x_last = rng.standard_normal((T, N, cols)).astype(np.float32), rng.standard_normal((N, cols)).astype(np.float32)
    for t in range(T + 1):
        row = x[t] if t < T else x_last
        row[:, t % 2], row[:, 1 - t % 2] = 0.0, 1.0
    if flags == "none":
        dones, time_outs = np.zeros((T, N), bool), np.zeros((T, N), bool)
    elif flags == "all":
        dones = rng.random((T, N)) < 0.5
        time_outs = ~dones | (rng.random((T, N)) < 0.3)
    else:  # about a fifth of the rows cut, by either flag or by both
        dones, time_outs = rng.random((T, N)) < 0.1, rng.random((T, N)) < 0.11
    return x, x_last, dones, time_outs


def _run(x, x_last, dones, time_outs, mode, seed=0, update=0, epoch=0, as_bool=True):
    """bg_partner_rows through its wrapper into a buffer with a guard step behind the T N rows; returns y as numpy and checks the guard."""
    from booster_gym_amd.utils.utils import partner_rows

    T, N, cols = x.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = torch.full((T + 1, N, cols), GUARD, device=DEV)
    fl = (lambda a: dev(a)) if as_bool else (lambda a: dev(a.astype(np.uint8) * 255))
    partner_rows(dev(x), dev(x_last), fl(dones), fl(time_outs), out[:T], mode, seed, update, epoch)
    torch.cuda.synchronize()
    assert bool((out[T] == GUARD).all()), "rows past T N were written"
    return out[:T].cpu().numpy()


@pytest.mark.parametrize("flags", ["fifth", "all", "none"])
@pytest.mark.parametrize("T,N,cols", SHAPES)
def test_partner_rows_next_is_a_bit_exact_copy(T, N, cols, flags):
    x, x_last, dones, time_outs = _case(T, N, cols, flags)
    cut = dones | time_outs
    assert {"none": not cut.any(), "all": cut.all(), "fifth": 0.1 < cut.mean() < 0.35 or T * N < 50}[flags]
    ref, _ = partner_rows_ref(x, x_last, dones, time_outs)
    for as_bool in (True, False):
        y = _run(x, x_last, dones, time_outs, "next", as_bool=as_bool)
        assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(y[cut].view(np.uint32), x[cut].view(np.uint32))  # a cut pair's row is x itself
    if T > 1 and not cut[0].all():
        e = int(np.flatnonzero(~cut[0])[0])
        assert np.array_equal(y[0, e], x[1, e])
    if not cut[T - 1].all():
        e = int(np.flatnonzero(~cut[T - 1])[0])
        assert np.array_equal(y[T - 1, e], x_last[e])


@pytest.mark.parametrize("flags", ["fifth", "all", "none"])
@pytest.mark.parametrize("T,N,cols", SHAPES)
def test_partner_rows_interpolate_draws_the_host_generators_u(T, N, cols, flags):
    """u bit for bit (read back from the column where x = 0 and x+ - x = 1), the values within 2 ulp of the fp32 restatement, cut rows bit-equal to x.
    The ulp is that of the larger operand, max(|x|, |x+|): the restatement rounds p = u (x+ - x) and then x + p, the kernel's fma rounds once, so the
    two differ by at most ulp(p) / 2 + ulp(y), and |p| <= 2 max(|x|, |x+|), |y| <= max(|x|, |x+|).  Beside it the kernel's own contract: one rounding of
    the exact x + u fl(x+ - x), against float64."""
    seed, update, epoch = 0x1234_5678_9ABC, 3, 2
    x, x_last, dones, time_outs = _case(T, N, cols, flags)
    cut = dones | time_outs
    ref, u = partner_rows_ref(x, x_last, dones, time_outs, "interpolate", seed, update, epoch)
    y = _run(x, x_last, dones, time_outs, "interpolate", seed, update, epoch)
    assert np.array_equal(u.reshape(-1), partner_draw(seed, T * N, update, epoch)) and u.min() >= 0 and u.max() < 1
    got_u = np.where((np.arange(T) % 2 == 0)[:, None], y[:, :, 0], y[:, :, 1])
    live = ~cut
    assert np.array_equal(got_u[live].view(np.uint32), u[live].view(np.uint32))
    assert np.array_equal(y[cut].view(np.uint32), x[cut].view(np.uint32))
    nxt = np.concatenate([x[1:], x_last[None]], axis=0)
    scale = np.spacing(np.maximum(np.abs(x), np.abs(nxt)).astype(np.float32))
    err = np.abs(y.astype(np.float64) - ref.astype(np.float64)) / scale
    exact = x.astype(np.float64) + u[..., None].astype(np.float64) * (nxt - x).astype(np.float64)
    err1 = (np.abs(y.astype(np.float64) - exact) / np.spacing(np.abs(y)))[live]
    print(f"({T}, {N}, {cols}) {flags}: max |y - restatement| {err.max():.3f} ulp of the operands, max |y - exact| {err1.max() if live.any() else 0.0:.4f} ulp of y")
    assert err.max() <= 2.0
    assert not live.any() or err1.max() <= 0.5 + 1e-6


def test_partner_rows_draw_changes_with_mini_epoch_and_update_and_repeats():
    T, N, cols = 3, 37, 64
    x, x_last, dones, time_outs = _case(T, N, cols, "none")
    us = {}
    for key in ((42, 0, 0), (42, 0, 1), (42, 1, 0), (43, 0, 0), (42, 0, 0)):
        y = _run(x, x_last, dones, time_outs, "interpolate", *key)
        u = np.where((np.arange(T) % 2 == 0)[:, None], y[:, :, 0], y[:, :, 1])
        assert np.array_equal(u.reshape(-1), partner_draw(*((key[0], T * N) + key[1:])))
        if key in us:
            assert np.array_equal(us[key], u)  # equal on a repeat
        us[key] = u
    keys = list(us)
    for i, a in enumerate(keys):  # two mini-epochs, two updates, two seeds: all different
        for b in keys[i + 1 :]:
            assert not np.array_equal(us[a], us[b]), (a, b)


def test_partner_rows_refuses_bad_arguments():
    from booster_gym_amd import _lib

    lib = _lib.load()
    T, N, cols = 2, 8, 64
    x, y, xl = torch.zeros(T, N, cols + 4, device=DEV), torch.zeros(T, N, cols + 4, device=DEV), torch.zeros(N, cols + 4, device=DEV)
    f = torch.zeros(T, N, dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, None
    ok = dict(T=T, N=N, cols=cols, x=p(x), x_last=p(xl), dones=p(f), time_outs=p(f), mode=0, seed=1, update=0, epoch=0, y=p(y))
    bad = [dict(T=0), dict(N=0), dict(T=-1), dict(cols=0), dict(cols=6), dict(cols=62), dict(cols=516), dict(cols=1024), dict(x=None), dict(x_last=None),
           dict(dones=None), dict(time_outs=None), dict(y=None), dict(mode=2), dict(mode=-1), dict(x=x.data_ptr() + 4), dict(x_last=xl.data_ptr() + 8),
           dict(y=y.data_ptr() + 4), dict(y=p(x)), dict(y=x.data_ptr() + 16), dict(y=p(xl)), dict(T=1 << 16, N=1 << 16)]
    for b in bad:
        a = {**ok, **b}
        rc = lib.bg_partner_rows(*[a[k] for k in ("T", "N", "cols", "x", "x_last", "dones", "time_outs", "mode", "seed", "update", "epoch", "y")], st)
        assert rc == -1 and b"bg_partner_rows" in lib.bg_last_error(), (b, rc, lib.bg_last_error())
    torch.cuda.synchronize()
    assert not y.any() and not x.any()  # refused before any launch
    assert lib.bg_partner_rows(*[ok[k] for k in ("T", "N", "cols", "x", "x_last", "dones", "time_outs", "mode", "seed", "update", "epoch", "y")], st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the head with the identity action map
@pytest.mark.parametrize("B", [40, 1000])
def test_head_with_the_identity_map_matches_float64_autograd_and_cut_pairs_add_nothing(B):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import actor_head_sym_loss_backward, head_scratch, reduce_group

    g = torch.Generator(device="cpu").manual_seed(B + 5)
    A = 12
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    h = torch.nn.functional.elu(rnd(2 * B, 128))
    cut = torch.rand(B, generator=g).to(DEV) < 0.2
    cut[0] = cut[B - 1] = True
    h[B:][cut] = h[:B][cut]  # a cut pair: both rows are one row
    W, b = rnd(A, 128) * 0.1, rnd(A) * 0.1
    logstd = torch.full((A,), -2.0, device=DEV) + 0.1 * rnd(A)
    old_logstd = torch.full((A,), -2.0, device=DEV)
    old_mu = (h[:B] @ W.t() + b) + 0.02 * rnd(B, A)
    actions = old_mu + 0.135 * rnd(B, A)
    old_logp = (-0.5 * ((actions - old_mu) / old_logstd.exp()) ** 2 - old_logstd - 0.9189385332046727).sum(-1)
    adv = rnd(B)
    adv_stats = torch.stack([adv.double().sum(), (adv.double() ** 2).sum(), torch.tensor(float(B), dtype=torch.float64, device=DEV)])
    coef = 10.0
    rel = lambda x, r: ((x.double() - r.double()).abs().max() / max(1e-30, r.double().abs().max())).item()

    def run(hh, deferred):
        g_hidden, mu = torch.empty(2 * B, 128, device=DEV), torch.empty(2 * B, A, device=DEV)
        dW, db, dbh = torch.empty(A, 128, device=DEV), torch.empty(A, device=DEV), torch.empty(128, device=DEV)
        gls, st = torch.zeros(A, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
        fin = _lib.ReduceProblem() if deferred else None
        actor_head_sym_loss_backward(hh, W, b, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, 0.2, 1.0, -0.01, coef, IDENTITY, g_hidden, dW, db, dbh,
                                     gls, st, head_scratch(DEV), mu_out=mu, finish=fin)
        if deferred:
            reduce_group([fin])
        torch.cuda.synchronize()
        return mu, g_hidden, dW, db, dbh, gls, st

    ref = _head_ref(h, W, b, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, 1.0, -0.01, coef, *IDENTITY)
    mu_ref, g_ref, dW_ref, db_ref, dbh_ref, gls_ref, st_ref = ref
    assert st_ref[5].item() > 0
    for deferred in (False, True):
        mu, g_hidden, dW, db, dbh, gls, st = run(h, deferred)
        assert rel(mu, mu_ref) < 2e-5
        assert rel(g_hidden, g_ref) < 2e-3 and rel(g_hidden[B:], g_ref[B:]) < 1e-4
        assert rel(dW, dW_ref) < 2e-3 and rel(db, db_ref) < 2e-3 and rel(dbh, dbh_ref) < 2e-3
        assert rel(gls, gls_ref) < 2e-3
        assert st[0] == 0 and rel(st[1:], st_ref[1:]) < 1e-4
        assert abs(st[5].item() - st_ref[5].item()) < 1e-5 * st_ref[5].item()
        assert torch.equal(mu[B:][cut], mu[:B][cut])  # equal rows, equal means, bit for bit
        assert not g_hidden[B:][cut].any(), "a cut pair's partner row carries a gradient"
        assert g_hidden[B:][~cut].any(dim=1).all()
    # every pair cut: the sixth statistic is exactly 0, no partner row carries a gradient, and the original rows' gradients are those of coefficient 0
    hh = torch.cat([h[:B], h[:B]])
    for deferred in (False, True):
        mu, g_hidden, dW, db, dbh, gls, st = run(hh, deferred)
        assert st[5].item() == 0.0 and not g_hidden[B:].any()
    ref0 = _head_ref(hh, W, b, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, 1.0, -0.01, 0.0, *IDENTITY)
    assert rel(g_hidden[:B], ref0[1][:B]) < 2e-3 and rel(dW, ref0[2]) < 2e-3


# ------------------------------------------------------------------ the update against the reference loop
def ppo_update_smooth_reference(model, optimizer, obses, privileged_obses, actions, rewards, dones, time_outs, last_obs, last_privileged_obs, pairs, draw_key,
                                mini_epochs=20, gamma=0.995, lam=0.95, bound_coef=1.0, entropy_coef=-0.01, smoothness_coef=10.0, desired_kl=0.01,
                                learning_rate=1e-5, max_grad_norm=1.0):
    """tests/test_gpu_symmetry.ppo_update_sym_reference (the reference's loop, runner.py:123-189, plus a pair term) with mu(x') - mu(x) in place of the
    symmetry term: smoothness_coef * mean |mu(x') - mu(x)|^2 differentiated through both means, x' from the restated partner rule on the rows the
    actor reads (obses [T, N, K], last_obs [N, K]); draw_key = (seed, update): the draw of pairs "interpolate" is fresh in every mini-epoch.  Returns
    (stats with smoothness_loss, final lr)."""
    import torch.nn.functional as F

    from oracle.ppo_ref import discount_values, surrogate_loss

    x_np, xl_np = obses.cpu().numpy(), last_obs.cpu().numpy()
    d_np, t_np = dones.cpu().numpy().astype(bool), time_outs.cpu().numpy().astype(bool)
    with torch.no_grad():
        old_dist = model.act(obses)
        old_actions_log_prob = old_dist.log_prob(actions).sum(dim=-1)
    sums = dict(value_loss=0.0, actor_loss=0.0, bound_loss=0.0, entropy=0.0, smoothness_loss=0.0)
    for n in range(mini_epochs):
        partner = torch.from_numpy(partner_rows_ref(x_np, xl_np, d_np, t_np, pairs, draw_key[0], draw_key[1], n)[0]).to(obses.device)
        values = model.est_value(obses, privileged_obses)
        last_values = model.est_value(last_obs, last_privileged_obs)
        with torch.no_grad():
            rewards[time_outs] = values[time_outs]
            advantages = discount_values(rewards, dones | time_outs, values, last_values, gamma, lam)
            returns = values + advantages
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
        value_loss = F.mse_loss(values, returns)
        dist = model.act(obses)
        actions_log_prob = dist.log_prob(actions).sum(dim=-1)
        actor_loss = surrogate_loss(old_actions_log_prob, actions_log_prob, advantages)
        bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
        entropy = dist.entropy().sum(dim=-1)
        smooth_loss = (model.actor(partner) - dist.loc).square().mean()
        loss = value_loss + actor_loss + bound_coef * bound_loss + entropy_coef * entropy.mean() + smoothness_coef * smooth_loss
        optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
        optimizer.step()
        with torch.no_grad():
            kl = torch.sum(torch.log(dist.scale / old_dist.scale)
                           + 0.5 * (torch.square(old_dist.scale) + torch.square(dist.loc - old_dist.loc)) / torch.square(dist.scale) - 0.5, axis=-1)
            kl_mean = torch.mean(kl)
            if kl_mean > desired_kl * 2:
                learning_rate = max(1e-5, learning_rate / 1.5)
            elif kl_mean < desired_kl / 2:
                learning_rate = min(1e-2, learning_rate * 1.5)
            for param_group in optimizer.param_groups:
                param_group["lr"] = learning_rate
        for k, v in zip(sums, (value_loss, actor_loss, bound_loss, entropy.mean(), smooth_loss)):
            sums[k] += v.item()
    out = {k: v / mini_epochs for k, v in sums.items()}
    out["kl_mean"] = float(kl_mean)
    return out, learning_rate


COEF = 10.0


def _runner(n, E=3, T=24, seed=None, pairs="next", coef=COEF, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    o = {"env.num_envs": n, "terrain.type": "plane", "runner.mini_epochs": E, "runner.horizon_length": T, "algorithm.smoothness_loss": True,
         "algorithm.smoothness_coef": coef, "algorithm.smoothness_pairs": pairs}
    if seed is not None:
        o["basic.seed"] = seed
    o.update(over)
    r = Runner(cfg=load_cfg("T1", o))
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    return r


def _draw_key(r):
    return int(r.cfg["basic"]["seed"]) + 1000003 * (r.rank + 1), r._smooth_updates


def _compare(r, E, T, ref_model, stats_ref, lr_ref, p_start, rewards_ref):
    summ = r._summarize(r.update())
    for (k, p), (k2, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        assert k == k2
        _assert_same_adam_steps(k, p, q, p_start[k])
        if E <= 5:
            assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    assert torch.allclose(r.buffer["rewards"], rewards_ref, atol=1e-5)
    assert "symmetry_loss" not in summ
    for k in LOSSES:
        print(f"{k}: {summ[k]!r} against {stats_ref[k]!r}")
    assert stats_ref["smoothness_loss"] > 0 and summ["smoothness_loss"] > 0
    for k in LOSSES:
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9
    return summ


@pytest.mark.parametrize("n,E,T,pairs", [(128, 3, 24, "next"), (100, 2, 24, "next"), (384, 2, 5, "next"), (128, 3, 24, "interpolate")])
def test_smooth_update_matches_reference_loop(n, E, T, pairs):
    """Runner.update() with algorithm.smoothness_loss on against the reference's loop plus the term, from the same weights on the same rollout:
    parameters (test_full_update_matches_reference_loop's bound), every logged loss including smoothness_loss, the learning rate.  Fails where the
    key is ignored (no smoothness_loss in the log, 5 statistics)."""
    from booster_gym_amd.utils.model import ActorCritic

    r = _runner(n, E, T, pairs=pairs)
    plan = r._resolve_plan()
    assert plan.smoothness and plan.symmetry and not plan.ahead and r._n_stats == 6 and tuple(r._actor_in.shape) == (2 * T, n, 64)
    r.rollout()
    ref_model = ActorCritic(12, 47, 14).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    cut = b["dones"] | b["time_outs"]
    rewards_ref = b["rewards"].clone()
    stats_ref, lr_ref = ppo_update_smooth_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), b["obses"][:T].clone(),
                                                    b["privileged_obses"][:T].clone(), b["actions"].clone(), rewards_ref, b["dones"].clone(), b["time_outs"].clone(),
                                                    b["obses"][T].clone(), b["privileged_obses"][T].clone(), pairs, _draw_key(r), mini_epochs=E,
                                                    smoothness_coef=COEF, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    _compare(r, E, T, ref_model, stats_ref, lr_ref, p_start, rewards_ref)
    assert r._smooth_updates == 1
    # the rows the actor trained on: the batch, then its partners (pairs "next": the successors, cut rows themselves; the padding stays zero)
    if pairs == "next":
        want, _ = partner_rows_ref(b["obses"][:T].cpu().numpy(), b["obses"][T].cpu().numpy(), b["dones"].cpu().numpy(), b["time_outs"].cpu().numpy())
        assert np.array_equal(r._actor_in[T:, :, :47].cpu().numpy(), want) and not r._actor_in[:, :, 47:].any()
        assert torch.equal(r._actor_in[T:][cut], r._actor_in[:T][cut])


def test_smooth_update_composed_with_a_frame_stack_normalisation_and_the_actors_scan():
    """env.frame_stack 3 + algorithm.empirical_normalization + terrain.actor_heights on the 9 x 5 grid, pairs "interpolate", in the second iteration (the
    statistics are not the initial ones, the draw's update counter is 1): against the loop fed the rows normalised on the host, interpolated there."""
    from test_gpu_actor_heights import _ov
    from test_gpu_obs_norm import _host_normalise

    from booster_gym_amd.utils.model import ActorCritic

    E, T, n, H = 3, 24, 128, 3
    r = _runner(n, E, T, pairs="interpolate", **_ov(n, H, **{"algorithm.empirical_normalization": True, "terrain.type": "trimesh"}))
    no, npv = r.env.num_obs, r.env.num_privileged_obs
    assert (no, npv) == (141 + 45, 59) and tuple(r._actor_in.shape) == (2 * T, n, 256) and tuple(r._actor_last.shape) == (n, 256)
    r.iteration()
    opt = r.optimizer
    opt.exp_avg.zero_(); opt.exp_avg_sq.zero_(); opt.step_count = 0; opt.lr.fill_(1e-5)
    r.invalidate()
    r.rollout()
    norm = r.obs_norm
    assert norm.count == T * n and r._smooth_updates == 1
    ref_model = ActorCritic(12, no, npv).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    hn, hp = (lambda x: _host_normalise(norm, x)), (lambda x: _host_normalise(norm, x, no))
    rewards_ref = b["rewards"].clone()
    stats_ref, lr_ref = ppo_update_smooth_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), hn(b["obses"][:T]), hp(b["privileged_obses"][:T]),
                                                    b["actions"].clone(), rewards_ref, b["dones"].clone(), b["time_outs"].clone(), hn(b["obses"][T]),
                                                    hp(b["privileged_obses"][T]), "interpolate", _draw_key(r), mini_epochs=E, smoothness_coef=COEF,
                                                    learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    want_last = hn(b["obses"][T])
    _compare(r, E, T, ref_model, stats_ref, lr_ref, p_start, rewards_ref)
    assert torch.equal(r._actor_last[:, :no], want_last) and not r._actor_last[:, no:].any() and not r._actor_in[:, :, no:].any()


# ------------------------------------------------------------------ behaviour
def _train(n, iters, seed, **over):
    r = _runner(n, E=4, seed=seed, **over)
    start = r.optimizer.flat.clone()
    for _ in range(iters):
        stats = r.iteration().clone()
    torch.cuda.synchronize()
    return r, start, stats


@pytest.mark.parametrize("pairs", ["next", "interpolate"])
def test_smooth_training_is_reproducible(pairs):
    res = []
    for _ in range(2):
        r, _, stats = _train(512, 3, 11, pairs=pairs, **{"terrain.type": "trimesh", "commands.curriculum": True})
        assert r._smooth_updates == 3
        res.append((r.optimizer.flat.clone(), r.optimizer.exp_avg.clone(), r.optimizer.exp_avg_sq.clone(), r.optimizer.lr.clone(), stats, r.buffer["obses"].clone(),
                    r.buffer["actions"].clone(), r._actor_in.clone()))
        del r
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"item {k} differs between two identical runs"


def test_zero_coefficient_equals_the_loss_off():
    """smoothness_coef 0: the loss is on (2B actor rows, the pair head) but adds nothing: the loss-off update, within the Adam-step bound."""
    on, start, s_on = _train(256, 1, 3, coef=0.0)
    off, _, s_off = _train(256, 1, 3, **{"algorithm.smoothness_loss": False})
    assert on._n_stats == 6 and off._n_stats == 5 and s_on[5] > 0
    _assert_same_adam_steps("flat", on.optimizer.flat, off.optimizer.flat, start)
    so, sf = on._summarize(s_on), off._summarize(s_off)
    assert "smoothness_loss" in so and "smoothness_loss" not in sf and "symmetry_loss" not in so and "symmetry_loss" not in sf
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean"):
        assert abs(so[k] - sf[k]) <= 1e-3 * max(1.0, abs(sf[k])), (k, so[k], sf[k])


def test_key_off_runs_todays_calls_alone(monkeypatch):
    """Key absent, null and false (whatever the other two keys hold): the same library calls in the same order, the same bits, no new buffer, log name or
    checkpoint key; with the key on bg_partner_rows runs once per update (pairs "next") or once per mini-epoch ("interpolate")."""
    import hashlib

    from booster_gym_amd import _lib

    lib, seq = _lib.load(), []
    for name in _lib.SYMBOLS:
        if name in ("bg_last_error", "bg_version"):
            continue
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            seq.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    runs = []
    for alg in ({}, {"algorithm.smoothness_loss": None}, {"algorithm.smoothness_loss": False, "algorithm.smoothness_coef": "unread", "algorithm.smoothness_pairs": 7}):
        from booster_gym_amd.utils.config import load_cfg
        from booster_gym_amd.utils.runner import Runner

        r = Runner(cfg=load_cfg("T1", {"env.num_envs": 256, "terrain.type": "plane", "runner.mini_epochs": 3, "basic.seed": 5, **alg}))
        obs, infos = r.env.reset()
        r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
        assert not r._smooth and r._n_stats == 5 and not hasattr(r, "_actor_last") and tuple(r._actor_in.shape) == (24, 256, 64)
        del seq[:]
        acc = r.iteration().clone()
        first = list(seq)
        acc = r.iteration().clone()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in [r.optimizer.flat, r.optimizer.exp_avg, r.optimizer.exp_avg_sq, r.optimizer.lr, acc] + [r.buffer[k] for k in sorted(r.buffer.names())]:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        runs.append((first, h.hexdigest(), sorted(r.checkpoint_dict()), sorted(r._summarize(acc))))
        del r
    assert runs[0] == runs[1] == runs[2]
    assert not any(s in runs[0][0] for s in ("bg_partner_rows", "bg_actor_head_sym", "bg_actor_head_sym_partial", "bg_mirror_rows"))
    assert runs[0][2] == ["curriculum", "model", "optimizer"] and "smoothness_loss" not in runs[0][3]
    E = 3
    for pairs, want in (("next", 1), ("interpolate", E)):
        r = _runner(256, E, pairs=pairs, seed=5)
        del seq[:]
        r.iteration()
        assert seq.count("bg_partner_rows") == want and seq.count("bg_actor_head_sym_partial") + seq.count("bg_actor_head_sym") == E
        assert "bg_mirror_rows" not in seq and seq.count("bg_actor_head_partial") == 0
        assert sorted(r.checkpoint_dict()) == ["curriculum", "model", "optimizer"]  # checkpoints gain no key
        del r


def _worker(rank, world, port, q):
    try:
        _worker_body(rank, world, port, q)
    except BaseException as ex:
        import traceback

        q.put(("error", rank, "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))))
        raise


def _worker_body(rank, world, port, q):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      BG_DIST_BACKEND="gloo", BG_LOCAL_DEVICE="0")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist

    from booster_gym_amd.utils.model import ActorCritic

    E, n, T = 2, 64, 24
    r = _runner(n, E, T)
    assert r.world_size == 2 and r.rank == rank
    r.rollout()
    sd0 = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    b = r.buffer

    def gather(t, dim):
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t.contiguous())
        return torch.cat(parts, dim=dim)

    full = {k: gather(b[k].to(torch.uint8) if b[k].dtype == torch.bool else b[k], 1) for k in ("obses", "privileged_obses", "actions", "rewards", "dones", "time_outs")}
    summ = r._summarize(r.update())
    flat = torch.cat([p.detach().reshape(-1) for p in r.model.parameters()])
    other = gather(flat.view(1, -1), 0)
    ref_model = ActorCritic(12, 47, 14).to(r.device)
    ref_model.load_state_dict(sd0)
    # pairs "next": every env's partner is its own successor, so the union's partner rows are the ranks' partner rows side by side
    stats_ref, lr_ref = ppo_update_smooth_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), full["obses"][:T], full["privileged_obses"][:T],
                                                    full["actions"], full["rewards"].clone(), full["dones"].bool(), full["time_outs"].bool(), full["obses"][T],
                                                    full["privileged_obses"][T], "next", (0, 0), mini_epochs=E, smoothness_coef=COEF, learning_rate=1e-5)
    ref_flat = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    start = torch.cat([sd0[k].reshape(-1) for k, _ in r.model.named_parameters()])
    q.put((rank, float((other[0] - other[1]).abs().max()), float((flat - ref_flat).abs().max()), float((flat - start).abs().max()),
           summ["smoothness_loss"], stats_ref["smoothness_loss"], summ["kl_mean"], stats_ref["kl_mean"], summ["lr"], lr_ref))
    r.dp.shutdown()


def test_two_rank_smooth_update_equals_reference_on_the_union():
    """tests/test_gpu_symmetry.test_two_rank_symmetric_update_equals_reference_on_the_union with this key: each rank pairs its own rows, the ranks end
    identical and the result is the single-process update on the union."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = []
        for _ in procs:
            item = q.get(timeout=300)
            if item[0] == "error":
                pytest.fail(f"rank {item[1]} raised:\n{item[2]}")
            res.append(item)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    for rank, rank_diff, ref_diff, moved, sm, sm_ref, kl, kl_ref, lr, lr_ref in res:
        assert rank_diff == 0.0, "ranks diverged"
        assert moved > 1e-6
        assert ref_diff < 5e-6 + 1e-3 * moved, (rank, ref_diff, moved)
        assert sm > 0 and abs(sm - sm_ref) <= 2e-4 * max(1.0, abs(sm_ref)) and abs(kl - kl_ref) <= 2e-4 * max(1.0, abs(kl_ref))
        assert abs(lr - lr_ref) < 1e-9


def test_the_loss_makes_the_policy_smoother():
    """Same seed, 1,024 envs, 10 iterations with the loss on and off: the final actor's mean |mu(x_t) - mu(x_t+1)|^2 over the uncut pairs of its last
    rollout is strictly lower with the loss on.  (How much lower is a measurement: DESIGN.md section 6.19.)"""
    rough = []
    for on in (True, False):
        r, _, _ = _train(1024, 10, 21, **{"algorithm.smoothness_loss": on})
        b = r.buffer
        live = ~(b["dones"] | b["time_outs"])[1:]  # (iteration() has rolled the buffer: row 0 is the next rollout's, so the pairs of steps 1 .. T - 1)
        with torch.no_grad():
            mu = r.model.actor(b["obses"][1:])  # [T, N, 12]
        d = (mu[1:] - mu[:-1]).square().mean(-1)
        rough.append(d[live].mean().item())
        del r
    print(f"mean |mu(x_t) - mu(x_t+1)|^2 over the uncut pairs of the last rollout: loss on {rough[0]:.6e}, loss off {rough[1]:.6e}, ratio {rough[0] / rough[1]:.4f}")
    assert rough[0] < rough[1], rough
