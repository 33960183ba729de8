"""runner.num_env_mini_batches on the GPU: bg_gather_sequences against torch indexing (one launch over mixed streams, guards, an out-of-range
entry) and its argument errors; one update at K = 2 against the float64 restatement of the reference loop with the K-step inner loop
(tests/test_gpu_mini_batches.py's, on a model whose act() runs the GRU cell over the T steps of the mini-batch's envs from their h0 rows with their
resets), fed the env permutations read back from the device; the first step's gradients against float64 autograd on mini-batch 0; H = 256 with K = 3;
reproducibility; off is off; training, resuming and loading for evaluation.

Bounds are the project's own: parameters by assert_same_adam_steps, the logged terms 2e-4 max(1, |ref|), lr 1e-9 (tests/test_gpu_mini_batches.py), the
gradients 1e-4 of the tensor's largest entry (_grad_bound of tests/test_gpu_distill_memory.py)."""
import hashlib

import pytest
import torch

from test_gpu_actor_memory import SHORT_EPISODES, _float64_copy
from test_gpu_distill import _Rec
from test_gpu_distill_memory import _grad_bound
from test_gpu_mini_batches import compare_with_reference, reference_update_with_mini_batches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, NO = 12, 47
KEY, RNN = "runner.num_env_mini_batches", "algorithm.rnn_hidden_size"
CLIP = 0.25  # max_grad_norm of the update test, on both of its sides (as tests/test_gpu_actor_memory.py)


def _cfg(N=80, T=16, K=2, H=128, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "terrain.type": "plane", "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "runner.mini_epochs": 2}
    if H:
        ov[RNN] = H
    if K is not None:
        ov[KEY] = K
    ov.update(over)
    return load_cfg("T1", ov)


def _runner(cfg=None, **kw):
    from booster_gym_amd.utils.runner import Runner

    r = Runner(cfg=cfg if cfg is not None else _cfg(**kw))
    r.begin_training(recorder=_Rec())
    return r


def _spy(monkeypatch, names=("bg_gather_sequences", "bg_gather_rows", "bg_perm_fill")):
    from booster_gym_amd import _lib

    lib, counts = _lib.load(), {k: 0 for k in names}
    for name in counts:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


def _is_permutation(p, n):
    return p.dtype == torch.int32 and torch.equal(torch.sort(p.long()).values, torch.arange(n, device=p.device))


def _by_envs(src, sigma, K):
    """torch indexing of the per-row rule: src [T][N][...] -> [K][T][n][...] with mini-batch k the envs sigma[k n : (k + 1) n]."""
    T, N = src.shape[:2]
    return src[:, sigma.long()].reshape(T, K, N // K, *src.shape[2:]).transpose(0, 1).contiguous()


# ------------------------------------------------------------------ 1. the launch against torch indexing
GUARD = 16  # rows in front of and behind every destination (16 rows of any stream below keep the destination on the 16-byte grid)
STREAMS = ((64, torch.float32, 0), (12, torch.float32, 0), (76, torch.float32, 0), (1, torch.float32, 0), (13, torch.float32, 0), (128, torch.float32, 1),
           (1, torch.uint8, 0))  # (width, dtype, per env): 16-byte pieces for 64, 12, 76 and the per-env 128; single elements for 1, 13 and the bytes


def _sentinel(dtype):
    return 0xA5 if dtype == torch.uint8 else -7.0


def _launch(T, N, K, sigma, srcs):
    from booster_gym_amd import _lib

    dsts = []
    for (w, dtype, per_env), s in zip(STREAMS, srcs):
        rows = N if per_env else T * N
        dsts.append(torch.full((rows + 2 * GUARD, w), _sentinel(dtype), dtype=dtype, device=DEV))
    arr = (_lib.SequenceStream * len(srcs))(*[_lib.SequenceStream(s.data_ptr(), d[GUARD:].data_ptr(), w, s.element_size(), per_env, 0)
                                              for (w, _, per_env), s, d in zip(STREAMS, srcs, dsts)])
    _lib.check(_lib.load().bg_gather_sequences(T, N, K, _lib.ptr(sigma), arr, len(srcs), _lib.current_stream_ptr()), "bg_gather_sequences")
    torch.cuda.synchronize()
    for (w, dtype, _), d in zip(STREAMS, dsts):
        assert bool((d[:GUARD] == _sentinel(dtype)).all()) and bool((d[-GUARD:] == _sentinel(dtype)).all()), (w, dtype)
    return [d[GUARD:-GUARD] for d in dsts]


@pytest.mark.parametrize("T,N,K", [(5, 48, 3), (3, 40, 2)])
def test_gather_sequences_equals_torch_indexing_in_one_launch_over_mixed_streams(T, N, K, monkeypatch):
    from booster_gym_amd import _lib

    g = torch.Generator(device=DEV).manual_seed(T * N + K)
    srcs = []
    for w, dtype, per_env in STREAMS:
        shape = (N, w) if per_env else (T, N, w)
        srcs.append(torch.randint(0, 160, shape, device=DEV, generator=g).to(torch.uint8) if dtype == torch.uint8 else torch.randn(shape, device=DEV, generator=g))
    rand = torch.zeros(N, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().bg_perm_fill(N, 42 + 1000003, 3, 1, _lib.ptr(rand), _lib.current_stream_ptr()), "bg_perm_fill")
    assert _is_permutation(rand, N) and not torch.equal(rand, torch.arange(N, dtype=torch.int32, device=DEV))
    counts = _spy(monkeypatch, ("bg_gather_sequences", "bg_gather_rows"))
    n = N // K
    for sigma in (torch.arange(N, dtype=torch.int32, device=DEV), rand):
        counts.update(bg_gather_sequences=0, bg_gather_rows=0)
        outs = _launch(T, N, K, sigma, srcs)
        assert counts == {"bg_gather_sequences": 1, "bg_gather_rows": 0}
        for (w, dtype, per_env), s, o in zip(STREAMS, srcs, outs):
            want = s[sigma.long()] if per_env else _by_envs(s, sigma, K).reshape(T * N, w)
            assert o.dtype == dtype and torch.equal(o, want), (w, dtype, per_env)
    # one entry outside [0, N): exactly its T rows of every per-row stream and its one per-env row keep what they held
    for where, value in ((5, N + 3), (N - 1, -1)):
        bad = rand.clone()
        bad[where] = value
        k, j = divmod(where, n)
        outs = _launch(T, N, K, bad, srcs)
        for (w, dtype, per_env), s, o in zip(STREAMS, srcs, outs):
            want = s[rand.long()] if per_env else _by_envs(s, rand, K).reshape(T * N, w)
            kept = torch.zeros(o.shape[0], dtype=torch.bool, device=DEV)
            kept[[where] if per_env else [(k * T + t) * n + j for t in range(T)]] = True
            assert torch.equal(o[~kept], want[~kept]) and bool((o[kept] == _sentinel(dtype)).all()), (where, w, dtype, per_env)


# ------------------------------------------------------------------ 2. argument errors
def test_gather_sequences_argument_errors_name_the_entry_point():
    from booster_gym_amd import _lib

    lib, S = _lib.load(), _lib.SequenceStream
    T, N = 4, 8
    x, y, sigma = torch.zeros(T * N, 4, device=DEV), torch.zeros(T * N, 4, device=DEV), torch.arange(N, dtype=torch.int32, device=DEV)
    one = lambda *f: (S * 1)(S(*f))
    good = one(x.data_ptr(), y.data_ptr(), 4, 4, 0, 0)
    assert lib.bg_gather_sequences(T, N, 2, _lib.ptr(sigma), good, 1, None) == 0
    many = (S * 13)(*[S(x.data_ptr(), y.data_ptr(), 4, 4, 0, 0) for _ in range(13)])
    for what, args in (("N not divisible by K", (T, N, 3, _lib.ptr(sigma), good, 1)),
                       ("a NULL source", (T, N, 2, _lib.ptr(sigma), one(None, y.data_ptr(), 4, 4, 0, 0), 1)),
                       ("a NULL destination", (T, N, 2, _lib.ptr(sigma), one(x.data_ptr(), None, 4, 4, 0, 0), 1)),
                       ("a NULL permutation", (T, N, 2, None, good, 1)),
                       ("element size 2", (T, N, 2, _lib.ptr(sigma), one(x.data_ptr(), y.data_ptr(), 4, 2, 0, 0), 1)),
                       ("13 streams", (T, N, 2, _lib.ptr(sigma), many, 13)),
                       ("overlapping buffers", (T, N, 2, _lib.ptr(sigma), one(x.data_ptr(), x.data_ptr() + 16, 4, 4, 0, 0), 1)),
                       ("overlapping per-env buffers", (T, N, 2, _lib.ptr(sigma), one(x.data_ptr(), x.data_ptr() + 16, 4, 4, 1, 0), 1))):
        assert lib.bg_gather_sequences(*args, None) != 0 and b"bg_gather_sequences" in lib.bg_last_error(), (what, lib.bg_last_error())
    torch.cuda.synchronize()
    assert not bool(y[N:].any())  # (the one good call copied zeros; no refused call launched anything)


# ------------------------------------------------------------------ 3. one update against the float64 restatement
class _RestatedRows:
    """What reference_update_with_mini_batches asks of a model, on a float64 ActorCritic with memory.  Every observation row carries its env number in
    a column behind the 47 observations, so that act(rows) -- rows step-major [T][n'] of any n' envs -- runs the cell over the T steps of exactly
    those envs: from their h0 rows, a zero state behind their resets (tests/test_gpu_actor_memory.py's _Restated, for any subset of the envs)."""

    def __init__(self, net, h0, resets):
        self.net, self.h0, self.resets, self.T = net, h0.double(), resets, resets.shape[0]

    def parameters(self):
        return list(self.net.parameters())

    def named_parameters(self):
        return self.net.named_parameters()

    def act(self, rows):
        ids = rows[:, NO].reshape(self.T, -1)
        envs = ids[0].long()
        assert bool((ids == ids[0]).all()), "the rows are not whole sequences, step-major"
        x, h, mus = rows[:, :NO].reshape(self.T, -1, NO), self.h0[envs], []
        for t in range(self.T):
            h = self.net.memory(x[t], h * (1 - self.resets[t, envs].double()).view(-1, 1))
            mus.append(self.net.actor(h))
        mean = torch.stack(mus).reshape(-1, A)
        return torch.distributions.Normal(mean, torch.exp(self.net.logstd).expand_as(mean))

    def est_value(self, obs, privileged_obs):
        return self.net.critic(torch.cat((obs[..., :NO], privileged_obs), dim=-1)).squeeze(-1)


def _with_env_column(obs):
    """[..., N, 47] -> [..., N, 48] float64: the env number behind the observation."""
    ids = torch.arange(obs.shape[-2], device=obs.device, dtype=torch.float64).view(*([1] * (obs.dim() - 2)), -1, 1).expand(*obs.shape[:-1], 1)
    return torch.cat((obs.double(), ids), dim=-1)


def _rows_of(sigma, T, N, K):
    """The row numbers of the time-major flattened batch that each of the K steps trains on: [T][n] step-major."""
    n, s = N // K, sigma.long()
    return [(torch.arange(T, device=s.device).view(T, 1) * N + s[k * n : (k + 1) * n].view(1, n)).reshape(-1) for k in range(K)]


def test_one_update_at_two_env_mini_batches_matches_the_float64_restatement():
    """Measured on an MI355X, printed by the run: the parameter distances, the five logged terms, the learning rate, the gradient errors and whether the
    first step's KL sum is exactly 0 at log-std 0."""
    from oracle.ppo_ref import surrogate_loss

    N, T, K, H, E = 80, 16, 2, 128, 2
    r = _runner(N=N, T=T, K=K, H=H, **{"algorithm.learning_rate": 1.0e-5, **SHORT_EPISODES})
    mt, alg, n = r._mem_tr, r.cfg["algorithm"], N // K
    assert r._env_mini_batches == K and r._mini_batches == 1 and r._mb_rows == T * n == 640 and r._mem_mb.N == n and r._mem_mb.T == T
    r._fused_opt = False  # the tail as separate launches: the optimiser's step is a Python call a spy can stand in front of
    with torch.no_grad():
        r.model.logstd.zero_()  # (the head kernel's KL of a row is then exactly 0 where dmu is: tests/test_gpu_actor_memory.py)
    r.invalidate()
    r.optimizer.max_grad_norm = CLIP
    r.rollout()  # a rollout first: the one below starts from a state that is not zero
    r.buffer.roll()
    r.rollout()
    torch.cuda.synchronize()
    b = r.buffer
    assert mt.h0.abs().max().item() > 1e-3 and torch.equal(mt.resets[1:].bool(), b["dones"][: T - 1])
    assert bool(mt.resets[1:].any()) and not bool(mt.resets[1:].all())
    assert bool(b["dones"].any(dim=0).all()), "an env did not reset inside the horizon"
    plan = r._resolve_plan()
    mp = r._mb_plan
    assert not plan.ahead and not mp.one_tail and not mp.one_stream and (mp.actor.fwd, mp.actor.bwd) == ("layer", "layer") and mp.defer

    # (a) the restatement, fed the env permutations the update is about to use
    perms = [r.env_permutation(r._mb_updates, e) for e in range(E)]
    assert all(_is_permutation(p, N) for p in perms) and not torch.equal(perms[0], perms[1])
    batches = [_rows_of(p, T, N, K) for p in perms]
    ref = _float64_copy(r)
    restated = _RestatedRows(ref, mt.h0, mt.resets)
    obses, priv, actions = _with_env_column(b["obses"][:T]), b["privileged_obses"][:T].double(), b["actions"].double()
    stats_ref, lr_ref = reference_update_with_mini_batches(restated, torch.optim.Adam(restated.parameters(), lr=1.0e-5), obses, priv, actions, b["rewards"].double().clone(),
                                                           b["dones"].clone(), b["time_outs"].clone(), _with_env_column(b["obses"][T]), b["privileged_obses"][T].double(),
                                                           batches, gamma=alg["gamma"], lam=alg["lam"], bound_coef=alg["bound_coef"], entropy_coef=alg["entropy_coef"],
                                                           desired_kl=alg["desired_kl"], learning_rate=1.0e-5, max_grad_norm=CLIP)

    # (b) the update, its first step read in front of the first optimiser step
    first, calls, step = {}, [0], r.optimizer.step

    def spy():
        calls[0] += 1
        if not first:
            first.update({k: p.grad.clone() for k, p in r.model.named_parameters()}, adv=r._adv.clone(), stats=r._stats.clone(), h0=r._mb.h0.clone(),
                         resets=r._mb.resets.clone())
        step()

    r.optimizer.step = spy
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    acc = r.update()
    torch.cuda.synchronize()
    assert calls[0] == E * K and r.optimizer.step_count == E * K and r._mb_updates == 1
    assert torch.equal(r._env_perm, perms[-1])  # the last mini-epoch's permutation is the one the restatement was fed
    # the gathered state and reset flags of the first mini-epoch are the whole batch's by its permutation
    assert torch.equal(first.pop("h0"), mt.h0[perms[0].long()]) and torch.equal(first.pop("resets").view(K, T, n), _by_envs(mt.resets, perms[0], K))
    kl0 = first.pop("stats")[4].item()
    print(f"first step's KL sum at log-std 0: {kl0!r} (exactly 0: {kl0 == 0.0})")

    # (c) the first step's gradients against float64 autograd on mini-batch 0's envs, with the update's own advantages
    fresh = _float64_copy(r)
    fresh.load_state_dict({k: v.double() for k, v in p_start.items()})
    pol, idx = _RestatedRows(fresh, mt.h0, mt.resets), batches[0][0]
    obs_f, act_f = obses.reshape(T * N, -1), actions.reshape(T * N, A)
    with torch.no_grad():
        old_logp = pol.act(obs_f).log_prob(act_f).sum(-1)
    adv = first.pop("adv").double().reshape(-1)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)  # the whole batch's moments
    dist = pol.act(obs_f[idx])
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    loss = (surrogate_loss(old_logp[idx], dist.log_prob(act_f[idx]).sum(-1), adv[idx]) + alg["bound_coef"] * bound_loss
            + alg["entropy_coef"] * dist.entropy().sum(-1).mean())
    loss.backward()
    compared = 0
    for k, q in fresh.named_parameters():
        if k.startswith(("memory.", "actor.")) or k == "logstd":
            _grad_bound(first[k], q.grad, f"grad {k}")
            compared += 1
    assert compared == 4 + 8 + 1

    # (d) after E x K steps: parameters, the five logged terms, the learning rate
    assert all(not torch.equal(p, p_start[k]) for k, p in r.model.named_parameters())
    compare_with_reference(r, ref, stats_ref, lr_ref, p_start, acc)


# ------------------------------------------------------------------ 4. H = 256 and K = 3
def test_wide_cell_and_three_env_mini_batches():
    N, T, K, H = 96, 8, 3, 256
    r = _runner(N=N, T=T, K=K, H=H, **SHORT_EPISODES)
    assert r._mb_rows == 256 and r._mem_mb.H == H
    r.rollout()
    r.buffer.roll()
    r.rollout()
    mt = r._mem_tr
    r.update()
    torch.cuda.synchronize()
    E = r.cfg["runner"]["mini_epochs"]
    assert r.optimizer.step_count == E * K and torch.isfinite(r.optimizer.flat).all()
    sigma = r._env_perm
    assert _is_permutation(sigma, N) and torch.equal(sigma, r.env_permutation(0, E - 1))
    assert mt.h0.abs().max().item() > 1e-3 and bool(mt.resets.any())
    assert torch.equal(r._mb.h0, mt.h0[sigma.long()])
    assert torch.equal(r._mb.resets.view(K, T, N // K), _by_envs(mt.resets, sigma, K))
    assert torch.equal(r._mb.actions.view(K, T, N // K, A), _by_envs(r.buffer["actions"], sigma, K))
    # the mini-batch trainers' weight copies were written by the last optimiser launch: current under the clock, and the parameters' bits
    cell, trunk = r._mem_mb.copies, r._actor_mb.copies
    assert cell.current("w0pad", 0) and all(trunk.current("wt", i) for i in range(3))
    assert torch.equal(cell.tensors["w0pad", 0][:, :NO], r.model.memory.weight_ih) and not bool(cell.tensors["w0pad", 0][:, NO:].any())
    assert all(torch.equal(trunk.tensors["wt", i], r.model.actor[2 * i].weight.t()) for i in range(3))
    # ... the whole-batch trainers' are stale until their next pass rewrites them
    assert not r._mem_tr.copies.current("w0pad", 0)
    r.buffer.roll()
    r.rollout()
    r.update()
    torch.cuda.synchronize()
    assert r.optimizer.step_count == 2 * E * K and r._mb_updates == 2 and torch.isfinite(r.optimizer.flat).all()


# ------------------------------------------------------------------ 5. reproducibility
def _digest(r):
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr, r.model._memory_state, r._last_dones]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_two_runs_with_one_seed_are_bitwise_equal_and_another_seed_permutes_differently():
    res, E = [], 2
    for seed in (5, 5, 6):
        r = _runner(**{"basic.seed": seed, **SHORT_EPISODES})
        N = r.env.num_envs
        for it in range(2):
            r.train_iteration(it)
        r._flush_log()
        torch.cuda.synchronize()
        assert r._mb_updates == 2 and r.optimizer.step_count == 2 * E * 2
        perms = [r.env_permutation(u, e) for u in range(2) for e in range(E)]
        assert all(_is_permutation(p, N) for p in perms)
        assert all(not torch.equal(perms[i], perms[j]) for i in range(4) for j in range(i))  # mini-epochs and updates all key it
        assert torch.equal(r._env_perm, perms[-1])
        res.append((_digest(r), perms[0].clone()))
        del r
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][1], res[2][1]) and res[0][0] != res[2][0]


# ------------------------------------------------------------------ 6. off is off
def test_off_is_off(monkeypatch):
    counts = _spy(monkeypatch)
    shas = []
    for K in (None, 1):
        cfg = _cfg(K=K, **SHORT_EPISODES)
        assert ("num_env_mini_batches" in cfg["runner"]) == (K is not None)
        r = _runner(cfg=cfg)
        assert r._env_mini_batches == 1 and not hasattr(r, "_env_perm") and not hasattr(r, "_mem_mb") and not hasattr(r, "_critic_mb")
        for it in range(2):
            r.train_iteration(it)
        r._flush_log()
        torch.cuda.synchronize()
        assert r.optimizer.step_count == 2 * 2
        shas.append(_digest(r))
        del r
    assert shas[0] == shas[1]
    r = _runner(cfg=_cfg(K=None, H=0))  # the default path: a feed-forward actor
    assert r._env_mini_batches == 1 and r._mem_tr is None
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    assert counts == {"bg_gather_sequences": 0, "bg_gather_rows": 0, "bg_perm_fill": 0}


# ------------------------------------------------------------------ 7. training, resuming, loading for evaluation
class _Saving(_Rec):
    def save(self, d, it):
        self.saved = (it, {k: v for k, v in d.items()})


def test_training_saves_resumes_and_loads_for_evaluation(tmp_path):
    from booster_gym_amd.utils.runner import Runner

    names = []
    for K in (None, 2):
        r = Runner(cfg=_cfg(K=K, **{"runner.save_interval": 1, **SHORT_EPISODES}))
        r.begin_training(recorder=_Saving())
        for it in range(3):
            r.train_iteration(it)
        r._flush_log()
        torch.cuda.synchronize()
        stats = r.recorder.stats
        assert sorted(stats) == [0, 1, 2] and all(torch.isfinite(torch.tensor(float(v))) for s in stats.values() for v in s.values())
        names.append(sorted(stats[2]))
        it, ck = r.recorder.saved
        assert it == 3 and sorted(ck) == ["curriculum", "model", "optimizer"]  # no checkpoint key is added
        assert r.optimizer.step_count == 3 * 2 * (K or 1) and torch.isfinite(r.optimizer.flat).all()
        if K:
            path = str(tmp_path / "env_mini_batches.pth")
            torch.save(ck, path)
            sd = {k: v.clone() for k, v in r.model.state_dict().items()}
        del r
    assert names[0] == names[1]  # the log names are today's
    cfg = _cfg(**{"basic.checkpoint": path, **SHORT_EPISODES})
    r = _runner(cfg=cfg)
    assert all(torch.equal(v, sd[k]) for k, v in r.model.state_dict().items()) and r.optimizer.step_count == 12 and r._mb_updates == 0
    first = r.env_permutation(0, 1)  # update counter 0 again, the last of the two mini-epochs
    r.train_iteration(0)
    r._flush_log()
    torch.cuda.synchronize()
    assert torch.equal(r._env_perm, first) and r._mb_updates == 1 and r.optimizer.step_count == 16 and torch.isfinite(r.optimizer.flat).all()
    del r
    p = Runner(test=True, cfg=_cfg(**{"basic.checkpoint": path}))  # evaluate.py's and play.py's way in, under the same yaml: the key is not read
    assert p._env_mini_batches == 1 and p._mem_tr is None and not hasattr(p, "_env_perm")
    assert all(torch.equal(v, sd[k]) for k, v in p.model.state_dict().items())
    assert p.play(max_steps=2) == 2
