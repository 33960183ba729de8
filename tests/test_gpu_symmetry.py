"""The mirror-symmetry loss on real kernels (algorithm.symmetry_loss): bg_mirror_rows, bg_actor_head_sym against float64 autograd, Runner.update()
against the reference loop plus the loss term, every switch of the update path, reproducibility, two ranks, and what the loss does to a policy."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_ppo import SWITCHES, _assert_same_adam_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    import json

    from booster_gym_amd.envs.mirror import mirror_maps

    m = json.load(open(os.path.join(ROOT, "booster_gym_amd", "resources", "T1", "T1_locomotion.flat.json")))
    return mirror_maps(m["dof_names"], [a for a in m["joint_axis"] if a], [-0.2, 0, 0, 0.4, -0.25, 0] * 2, 47)


def test_mirror_kernel_equals_torch_indexing():
    from booster_gym_amd.utils.utils import mirror_rows

    obs_src, obs_sign, _, _ = _maps()
    g = torch.Generator(device="cpu").manual_seed(0)
    for rows, pad in ((98304, 64), (1000, 64), (777, 47)):
        x = torch.randn(rows, pad, generator=g).to(DEV)
        if pad == 64:
            x[:, 47:] = 0
        src = obs_src.tolist() + [-1] * (pad - 47)
        sign = obs_sign.tolist() + [1.0] * (pad - 47)
        y = torch.full_like(x, float("nan"))
        mirror_rows(x, y, src, sign)
        torch.cuda.synchronize()
        ref = torch.zeros_like(x)
        ref[:, :47] = x[:, torch.as_tensor(obs_src, dtype=torch.long, device=DEV)] * torch.as_tensor(obs_sign, device=DEV)
        assert torch.equal(y, ref)
        z = torch.empty_like(x)
        mirror_rows(y, z, src, sign)  # an involution
        torch.cuda.synchronize()
        assert torch.equal(z, x)


def _head_ref(h, W, b, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, bound_coef, entropy_coef, coef, act_src, act_sign):
    """float64 autograd of the actor's loss (runner.py:145-161) on rows [0, B) plus coef / (B A) sum |mu(rows B..) - M_a mu(rows ..B)|^2."""
    dd = lambda t: t.detach().double().clone().requires_grad_(True)
    h64, W64, b64, ls64 = dd(h), dd(W), dd(b), dd(logstd)
    B, A = h.shape[0] // 2, W.shape[0]
    mu = h64 @ W64.t() + b64
    mo, mm = mu[:B], mu[B:]
    cnt = adv_stats[2].item()
    mean = adv_stats[0].item() / cnt
    std = np.sqrt(max(0.0, (adv_stats[1].item() - cnt * mean * mean) / (cnt - 1.0)))
    an = (adv.double() - mean) / (std + 1e-8)
    logp = (-0.5 * ((actions.double() - mo) / ls64.exp()) ** 2 - ls64 - 0.5 * np.log(2 * np.pi)).sum(-1)
    ratio = torch.exp(logp - old_logp.double())
    surr = torch.max(-an * ratio, -an * torch.clamp(ratio, 0.8, 1.2))
    bound = torch.clip(mo - 1.0, min=0.0).square() + torch.clip(mo + 1.0, max=0.0).square()
    ent = (0.5 + 0.5 * np.log(2 * np.pi) + ls64).sum()
    d = mm - mo[:, torch.as_tensor(act_src, dtype=torch.long, device=h.device)] * torch.as_tensor(act_sign, dtype=torch.float64, device=h.device)
    loss = surr.mean() + bound_coef * bound.mean() + entropy_coef * ent + coef * (d * d).mean()
    loss.backward()
    with torch.no_grad():
        ols = old_logstd.double()
        kl = (ls64 - ols + 0.5 * (torch.exp(2 * ols) + (mo - old_mu.double()) ** 2) / torch.exp(2 * ls64) - 0.5).sum(-1)
        stats = torch.stack([torch.zeros((), dtype=torch.float64, device=h.device), surr.sum(), bound.sum(), B * ent, kl.sum(), (d * d).sum()])
    g_hidden = h64.grad * torch.where(h > 0, torch.ones_like(h), h + 1).double()
    return mu.detach(), g_hidden, W64.grad, b64.grad, g_hidden.sum(0), ls64.grad, stats


@pytest.mark.parametrize("B", [1000, 49152, 40])
def test_symmetric_head_matches_float64_autograd(B):
    from booster_gym_amd.utils.utils import actor_head_sym_loss_backward, head_scratch, reduce_group
    from booster_gym_amd import _lib

    _, _, act_src, act_sign = _maps()
    g = torch.Generator(device="cpu").manual_seed(B)
    A = 12
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    h = torch.nn.functional.elu(rnd(2 * B, 128))
    W, b = rnd(A, 128) * 0.1, rnd(A) * 0.1
    logstd = torch.full((A,), -2.0, device=DEV) + 0.1 * rnd(A)
    old_logstd = torch.full((A,), -2.0, device=DEV)
    old_mu = (h[:B] @ W.t() + b) + 0.02 * rnd(B, A)
    actions = old_mu + 0.135 * rnd(B, A)
    old_logp = (-0.5 * ((actions - old_mu) / old_logstd.exp()) ** 2 - old_logstd - 0.9189385332046727).sum(-1)
    adv = rnd(B)
    adv_stats = torch.stack([adv.double().sum(), (adv.double() ** 2).sum(), torch.tensor(float(B), dtype=torch.float64, device=DEV)])
    coef = 10.0
    ref = _head_ref(h, W, b, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, 1.0, -0.01, coef, act_src, act_sign)
    rel = lambda x, r: ((x.double() - r.double()).abs().max() / max(1e-30, r.double().abs().max())).item()
    for deferred in (False, True):
        g_hidden, mu = torch.empty(2 * B, 128, device=DEV), torch.empty(2 * B, A, device=DEV)
        dW, db, dbh = torch.empty(A, 128, device=DEV), torch.empty(A, device=DEV), torch.empty(128, device=DEV)
        gls, st = torch.zeros(A, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
        fin = _lib.ReduceProblem() if deferred else None
        actor_head_sym_loss_backward(h, W, b, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, 0.2, 1.0, -0.01, coef, (act_src, act_sign),
                                     g_hidden, dW, db, dbh, gls, st, head_scratch(DEV), mu_out=mu, finish=fin)
        if deferred:
            reduce_group([fin])
        torch.cuda.synchronize()
        mu_ref, g_ref, dW_ref, db_ref, dbh_ref, gls_ref, st_ref = ref
        assert rel(mu, mu_ref) < 2e-5
        # (tolerances of tests/test_gpu_head.py: the ratio's exp() amplifies the last bits of mu by |adv| / sigma^2)
        assert rel(g_hidden, g_ref) < 2e-3 and rel(g_hidden[B:], g_ref[B:]) < 1e-4  # (the mirrored rows carry the symmetry term only)
        assert rel(dW, dW_ref) < 2e-3 and rel(db, db_ref) < 2e-3 and rel(dbh, dbh_ref) < 2e-3
        assert rel(gls, gls_ref) < 2e-3
        assert st[0] == 0 and rel(st[1:], st_ref[1:]) < 1e-4
        assert abs(st[5].item() - st_ref[5].item()) < 1e-5 * st_ref[5].item()
        if not deferred:
            first = (g_hidden.clone(), dW.clone(), db.clone(), dbh.clone(), gls.clone(), st.clone())
    for x, y in zip(first, (g_hidden, dW, db, dbh, gls, st)):
        assert torch.equal(x, y)  # the deferred form adds the same partial sums in the same order


def ppo_update_sym_reference(model, optimizer, obses, privileged_obses, actions, rewards, dones, time_outs, last_obs, last_privileged_obs, mirror,
                             mini_epochs=20, gamma=0.995, lam=0.95, bound_coef=1.0, entropy_coef=-0.01, symmetric_coef=10.0, desired_kl=0.01,
                             learning_rate=1e-5, max_grad_norm=1.0):
    """oracle/ppo_ref.ppo_update_reference (the reference's loop, runner.py:123-189) with the mirror-symmetry term added to every mini-epoch's loss:
    symmetric_coef * mean |mu(M_o x) - M_a mu(x)|^2, differentiated through both means.  Returns (stats with the symmetry loss, final lr)."""
    import torch.nn.functional as F

    from oracle.ppo_ref import discount_values, surrogate_loss

    obs_src, obs_sign, act_src, act_sign = (torch.as_tensor(np.asarray(v), device=obses.device) for v in mirror)
    obses_m = obses[..., obs_src.long()] * obs_sign
    with torch.no_grad():
        old_dist = model.act(obses)
        old_actions_log_prob = old_dist.log_prob(actions).sum(dim=-1)
    sums = dict(value_loss=0.0, actor_loss=0.0, bound_loss=0.0, entropy=0.0, symmetry_loss=0.0)
    for n in range(mini_epochs):
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
        sym_loss = (model.actor(obses_m) - dist.loc[..., act_src.long()] * act_sign).square().mean()
        loss = value_loss + actor_loss + bound_coef * bound_loss + entropy_coef * entropy.mean() + symmetric_coef * sym_loss
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
        for k, v in zip(sums, (value_loss, actor_loss, bound_loss, entropy.mean(), sym_loss)):
            sums[k] += v.item()
    out = {k: v / mini_epochs for k, v in sums.items()}
    out["kl_mean"] = float(kl_mean)
    return out, learning_rate


def _runner(n, E=3, T=24, seed=None, **over):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    o = {"env.num_envs": n, "terrain.type": "plane", "runner.mini_epochs": E, "runner.horizon_length": T, "algorithm.symmetry_loss": True}
    if seed is not None:
        o["basic.seed"] = seed
    o.update(over)
    r = Runner(cfg=load_cfg("T1", o))
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    return r


@pytest.mark.parametrize("n,E,T", [(128, 3, 24), (4096, 20, 24), (100, 2, 24), (384, 2, 5)])
def test_symmetric_update_matches_reference_loop(n, E, T):
    """Runner.update() with algorithm.symmetry_loss on against the reference's loop plus the symmetry term, from the same weights on the same rollout:
    parameters (test_full_update_matches_reference_loop's bound), every logged loss including symmetry_loss, the learning rate.  Fails where the key is
    ignored.  (384, 2, 5): B / 128 = 15 slabs, so the mirrored half starts on an odd slab."""
    from booster_gym_amd.utils.model import ActorCritic

    r = _runner(n, E, T)
    plan = r._resolve_plan()
    assert plan.symmetry and not plan.ahead and r._n_stats == 6
    r.rollout()
    ref_model = ActorCritic(12, 47, 14).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    rewards_ref = b["rewards"].clone()
    stats_ref, lr_ref = ppo_update_sym_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), b["obses"][:T].clone(),
                                                 b["privileged_obses"][:T].clone(), b["actions"].clone(), rewards_ref, b["dones"].clone(), b["time_outs"].clone(),
                                                 b["obses"][T].clone(), b["privileged_obses"][T].clone(), r.env.mirror_maps(), mini_epochs=E, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    summ = r._summarize(r.update())
    for (k, p), (k2, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        assert k == k2
        _assert_same_adam_steps(k, p, q, p_start[k])
        if E <= 5:
            assert torch.allclose(p, q, rtol=1e-3, atol=2e-6), (k, (p - q).abs().max().item())
    assert torch.allclose(b["rewards"], rewards_ref, atol=1e-5)
    assert stats_ref["symmetry_loss"] > 0
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean", "symmetry_loss"):
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9


def _sym_update_under(switch, **over):
    from booster_gym_amd.utils.model import MLPTrainer

    attrs, cls_attrs = SWITCHES[switch]
    saved = {k: getattr(MLPTrainer, k) for k in cls_attrs}
    try:
        for k, v in cls_attrs.items():
            setattr(MLPTrainer, k, v)
        r = _runner(256, seed=11, **over)
        for k, v in attrs.items():
            assert hasattr(r, k)
            setattr(r, k, v)
        start = r.optimizer.flat.clone()
        acc = r.iteration().clone()
        torch.cuda.synchronize()
        first = (r.optimizer.flat.clone(), acc, r._summarize(acc))
        acc2 = r.iteration().clone()
        torch.cuda.synchronize()
        return start, first, (r.optimizer.flat.clone(), acc2, r.buffer["actions"].clone())
    finally:
        for k, v in saved.items():
            setattr(MLPTrainer, k, v)


@pytest.fixture(scope="module")
def default_sym_update():
    return _sym_update_under("default")


@pytest.mark.parametrize("switch", [k for k in SWITCHES if k != "default"])
def test_symmetric_update_through_every_switch_matches_the_default(switch, default_sym_update):
    """test_update_through_every_switch_matches_the_default with the symmetry loss on.  The library-GEMM output layers cannot carry it: a ValueError
    names the reason.  The forward-ahead switches change nothing (the loss turns the forward-ahead off): identical bits."""
    if switch == "output_layers_as_library_gemms":
        with pytest.raises(ValueError, match="fused output layers"):
            _sym_update_under(switch)
        return
    start, (p0, a0, s0), (q0, b0, act0) = default_sym_update
    _, (p1, a1, s1), (q1, b1, act1) = _sym_update_under(switch)
    if switch.startswith("rollout_forward") or switch in ("chain_one_workgroup_per_slab", "backward_chain_one_workgroup_per_slab", "two_launches_on_two_streams"):
        assert torch.equal(p1, p0) and torch.equal(a1, a0) and torch.equal(q1, q0) and torch.equal(b1, b0) and torch.equal(act1, act0)
        return
    _assert_same_adam_steps(switch, p1, p0, start)
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean", "symmetry_loss"):
        assert abs(s1[k] - s0[k]) <= 1e-3 * max(1.0, abs(s0[k])), (k, s1[k], s0[k])
    assert abs(s1["lr"] - s0["lr"]) < 1e-9


def test_symmetric_update_of_other_widths_matches_reference_loop():
    from booster_gym_amd.utils.model import ActorCritic

    T, E = 24, 2
    r = _runner(128, E, T, **{"algorithm.actor_hidden": [512, 256, 128]})
    r.rollout()
    ref_model = ActorCritic(12, 47, 14, (512, 256, 128)).to(DEV)
    ref_model.load_state_dict(r.model.state_dict())
    b = r.buffer
    stats_ref, lr_ref = ppo_update_sym_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), b["obses"][:T].clone(),
                                                 b["privileged_obses"][:T].clone(), b["actions"].clone(), b["rewards"].clone(), b["dones"].clone(),
                                                 b["time_outs"].clone(), b["obses"][T].clone(), b["privileged_obses"][T].clone(), r.env.mirror_maps(),
                                                 mini_epochs=E, learning_rate=1e-5)
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    summ = r._summarize(r.update())
    for (k, p), (_, q) in zip(r.model.named_parameters(), ref_model.named_parameters()):
        _assert_same_adam_steps(k, p, q, p_start[k])
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean", "symmetry_loss"):
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])


def _train(n, iters, seed, **over):
    r = _runner(n, E=4, seed=seed, **over)
    start = r.optimizer.flat.clone()
    for _ in range(iters):
        stats = r.iteration().clone()
    torch.cuda.synchronize()
    return r, start, stats


def test_symmetric_training_is_reproducible_and_zero_coefficient_equals_the_loss_off():
    res = []
    for _ in range(2):
        r, _, stats = _train(512, 3, 11, **{"terrain.type": "trimesh", "commands.curriculum": True})
        res.append((r.optimizer.flat.clone(), r.optimizer.exp_avg.clone(), r.optimizer.exp_avg_sq.clone(), r.optimizer.lr.clone(), stats, r.buffer["obses"].clone(),
                    r.buffer["actions"].clone()))
        del r
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"item {k} differs between two identical runs"
    # symmetric_coef 0: the loss is on (2B actor rows, the symmetric head) but adds nothing: the loss-off update, within the Adam-step bound
    on, start, s_on = _train(256, 1, 3, **{"algorithm.symmetric_coef": 0.0})
    off, _, s_off = _train(256, 1, 3, **{"algorithm.symmetry_loss": False})
    assert on._n_stats == 6 and off._n_stats == 5 and s_on[5] > 0
    _assert_same_adam_steps("flat", on.optimizer.flat, off.optimizer.flat, start)
    so, sf = on._summarize(s_on), off._summarize(s_off)
    assert "symmetry_loss" in so and "symmetry_loss" not in sf
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean"):
        assert abs(so[k] - sf[k]) <= 1e-3 * max(1.0, abs(sf[k])), (k, so[k], sf[k])


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
    stats_ref, lr_ref = ppo_update_sym_reference(ref_model, torch.optim.Adam(ref_model.parameters(), lr=1e-5), full["obses"][:T], full["privileged_obses"][:T],
                                                 full["actions"], full["rewards"].clone(), full["dones"].bool(), full["time_outs"].bool(), full["obses"][T],
                                                 full["privileged_obses"][T], r.env.mirror_maps(), mini_epochs=E, learning_rate=1e-5)
    ref_flat = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    start = torch.cat([sd0[k].reshape(-1) for k, _ in r.model.named_parameters()])
    q.put((rank, float((other[0] - other[1]).abs().max()), float((flat - ref_flat).abs().max()), float((flat - start).abs().max()),
           summ["symmetry_loss"], stats_ref["symmetry_loss"], summ["kl_mean"], stats_ref["kl_mean"], summ["lr"], lr_ref))
    r.dp.shutdown()


def test_two_rank_symmetric_update_equals_reference_on_the_union():
    """tests/test_gpu_dp.py with the symmetry loss on: each rank mirrors its own rows, the result is the single-process update on the union."""
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
    for rank, rank_diff, ref_diff, moved, sym, sym_ref, kl, kl_ref, lr, lr_ref in res:
        assert rank_diff == 0.0, "ranks diverged"
        assert moved > 1e-6
        assert ref_diff < 5e-6 + 1e-3 * moved, (rank, ref_diff, moved)
        assert abs(sym - sym_ref) <= 2e-4 * max(1.0, abs(sym_ref)) and abs(kl - kl_ref) <= 2e-4 * max(1.0, abs(kl_ref))
        assert abs(lr - lr_ref) < 1e-9


def test_the_loss_makes_the_policy_more_symmetric():
    """Same seed, 1,024 envs, a few iterations with the loss on and off: the final actor's mean squared asymmetry on the last rollout's observations
    is at most half of the loss-off run's."""
    asym = []
    for on in (True, False):
        r, _, _ = _train(1024, 10, 21, **{"algorithm.symmetry_loss": on})
        obs_src, obs_sign, act_src, act_sign = (torch.as_tensor(np.asarray(v), device=DEV) for v in r.env.mirror_maps())
        x = r.buffer["obses"][:-1].reshape(-1, 47)
        with torch.no_grad():
            d = r.model.actor(x[:, obs_src.long()] * obs_sign) - r.model.actor(x)[:, act_src.long()] * act_sign
        asym.append(d.square().mean().item())
        del r
    assert asym[0] <= 0.5 * asym[1], asym
