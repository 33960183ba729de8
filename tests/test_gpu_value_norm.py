"""Value normalisation on the GPU (algorithm.normalize_value): bg_value_denormalize's rounding, bg_critic_values_gae_norm in both forms against
bg_value_denormalize followed by bg_critic_values_gae, bg_value_norm_update against the float64 restatement of tests/test_value_norm.py, and a Runner
under the key: every optimiser step's gradient against float64 autograd (tests/update_grad_ref.py, the bounds of tests/test_gpu_update_gradients.py),
the returns against a float64 GAE, the statistics, determinism, the launch sequence with the key off and on, and the checkpoint rules."""
import hashlib
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_distill import _Rec
from test_value_norm import merge_f64
from update_grad_ref import model_factory, record_steps, recurrent_means, step_gradients_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "algorithm.normalize_value"
NEW = ("bg_critic_values_gae_norm", "bg_value_denormalize", "bg_value_norm_update")
BOUND, NORM_BOUND = 1e-4, 1e-3  # tests/test_gpu_update_gradients.py's: every tensor to 1e-4 of its largest entry, the clip's norm to 1e-3
GAMMA, LAM = 0.995, 0.95


def _stats(m, sigma):
    return torch.tensor([m, sigma, 1.0 / sigma], dtype=torch.float64).float().to(DEV)


# ------------------------------------------------------------------ 1. bg_value_denormalize
@pytest.mark.parametrize("sigma", [1.0, 0.013, 40.0])
@pytest.mark.parametrize("m", [0.0, -3.7, 12.5])
def test_denormalize_is_one_rounding(m, sigma):
    """v = fmaf(sigma, u, m) against float64 sigma u + m on the fp32 operands: a fused multiply-add is correctly rounded, so |v - exact| is at most
    half a unit in the last place, 2^-24 |exact| (derived, not measured).  4,099 values of magnitudes 1e-3 .. 1e3: several workgroups and a tail."""
    from booster_gym_amd.utils.utils import value_denormalize

    g = torch.Generator().manual_seed(3)
    u = (torch.randn(4099, generator=g) * 10.0 ** (6.0 * torch.rand(4099, generator=g) - 3.0)).to(DEV)
    st = _stats(m, sigma)
    v = value_denormalize(u.clone(), st)
    exact = st[1].double() * u.double() + st[0].double()  # (the product of two fp32 numbers is exact in float64; the sum is rounded to 2^-53)
    err = (v.double() - exact).abs()
    print(f"m {m} sigma {sigma}: max |v - exact| / |exact| = {(err / exact.abs()).max().item():.3e} (2^-24 = {2.0 ** -24:.3e})")
    assert torch.isfinite(v).all() and bool((err <= 2.0 ** -24 * exact.abs()).all())
    assert not torch.equal(v, u) or (m == 0.0 and sigma == 1.0)


# ------------------------------------------------------------------ 2. bg_critic_values_gae_norm
def _gae_inputs(T, N):
    """tests/test_gpu_head.py's inputs and done / time-out patterns, plus env 0 timing out on its last step and env N - 1 done on every step."""
    g = torch.Generator(device="cpu").manual_seed(7 + T + N)
    h = torch.nn.functional.elu(torch.randn((T + 1) * N, 128, generator=g)).to(DEV)
    w, b = (torch.randn(1, 128, generator=g) * 0.1).to(DEV), torch.randn(1, generator=g).to(DEV)
    rew = torch.randn(T, N, generator=g).to(DEV)
    dones = (torch.rand(T, N, generator=g) < 0.05).to(DEV)
    touts = ((torch.rand(T, N, generator=g) < 0.03).to(DEV)) & dones
    dones[T - 1, 0] = touts[T - 1, 0] = True
    dones[:, N - 1] = True
    return h, w, b, rew, dones, touts


def _run_norm(T, N, h, w, b, rew, dones, touts, values, st, scratch):
    """One call of the _norm launch on fresh NaN outputs: (values_all, adv, ret, rewards, sums)."""
    from booster_gym_amd.utils.utils import critic_values_gae_norm

    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    r, adv, ret = rew.clone(), nan(T, N), nan(T, N)
    v = nan((T + 1) * N) if h is not None else values.clone()
    s = torch.full((6,), 123.0, dtype=torch.float64, device=DEV)  # must be overwritten, not added to
    critic_values_gae_norm(h, w, b, r, dones, touts, GAMMA, LAM, v, adv, ret, st, s, scratch)
    return v, adv, ret, r, s


@pytest.mark.parametrize("T,N", [(1, 1), (5, 17), (32, 16), (3, 65), (24, 100)])
def test_gae_norm_equals_denormalize_then_gae(T, N):
    from booster_gym_amd.utils.utils import critic_head_forward, critic_values_gae, value_denormalize
    from booster_gym_amd.utils.value_norm import triple_of

    h, w, b, rew, dones, touts = _gae_inputs(T, N)
    st = torch.from_numpy(triple_of(2.5, 0.13, 1.0e-2)).to(DEV)
    m, inv = st[0], st[2]
    u0 = critic_head_forward(h, w, b, torch.empty((T + 1) * N, device=DEV))
    v0 = value_denormalize(u0.clone(), st)
    plain = lambda n: torch.zeros(3 * ((n + 15) // 16) + 1, dtype=torch.float64, device=DEV)
    r0, adv0, ret0, s0 = rew.clone(), torch.empty(T, N, device=DEV), torch.empty(T, N, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    critic_values_gae(None, w, b, r0, dones, touts, GAMMA, LAM, v0.clone(), adv0, ret0, s0, plain(N))
    assert bool(touts.any()) and not torch.equal(r0, rew)  # a time-out's reward is the value v, in reward units
    want_ret = (ret0 - m) * inv  # torch: the subtract rounded, then the multiply rounded
    want_sums = torch.stack((ret0.double().sum(), (ret0.double() ** 2).sum()))
    scratch = torch.zeros(6 * ((N + 15) // 16) + 1, dtype=torch.float64, device=DEV)
    for form, hh in (("values", h), ("scan", None)):
        first = None
        for rep in range(2):
            v1, adv1, ret1, r1, s1 = _run_norm(T, N, hh, w, b, rew, dones, touts, u0, st, scratch)
            assert torch.equal(v1, u0), (form, rep)  # values_all keeps the critic's raw output
            assert torch.equal(adv1, adv0) and torch.equal(r1, r0) and torch.equal(ret1, want_ret), (form, rep)
            if hh is None:  # the reference's form: the same sums in the same order
                assert torch.equal(s1[:3], s0), (form, s1, s0)
            else:  # 16 envs per workgroup against 64: another fixed order (tests/test_gpu_head.py's allowance)
                assert torch.allclose(s1[:3], s0, rtol=1e-12, atol=1e-9), (form, s1, s0)
            rel = ((s1[3:5] - want_sums).abs() / want_sums.abs()).max().item()
            print(f"({T}, {N}) {form}: sums of R against float64 {rel:.3e}")
            assert rel <= 1e-12 and float(s1[5]) == T * N and float(s1[2]) == T * N, (form, s1, want_sums)
            assert float(scratch[-1]) == 0.0  # the ticket
            if first is None:
                first = (v1, adv1, ret1, r1, s1)
            else:
                assert all(torch.equal(a, c) for a, c in zip(first, (v1, adv1, ret1, r1, s1))), form  # deterministic
        # the identity statistics: every output is the plain launch's, of the same form, on the raw values
        one = torch.tensor([0.0, 1.0, 1.0], device=DEV)
        v2, adv2, ret2, r2, s2 = _run_norm(T, N, hh, w, b, rew, dones, touts, u0, one, scratch)
        r3, adv3, ret3, s3 = rew.clone(), torch.empty(T, N, device=DEV), torch.empty(T, N, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
        v3 = torch.empty((T + 1) * N, device=DEV) if hh is not None else u0.clone()
        critic_values_gae(hh, w, b, r3, dones, touts, GAMMA, LAM, v3, adv3, ret3, s3, plain(N))
        assert torch.equal(v2, v3) and torch.equal(adv2, adv3) and torch.equal(ret2, ret3) and torch.equal(r2, r3) and torch.equal(s2[:3], s3), form


def test_gae_norm_refuses_a_horizon_above_32():
    from booster_gym_amd.utils.utils import critic_values_gae_norm

    N = 16
    big, st = torch.zeros(33, N, device=DEV), _stats(0.0, 1.0)
    for h in (torch.zeros(34 * N, 128, device=DEV), None):
        with pytest.raises(RuntimeError, match=r"bg_critic_values_gae_norm failed \(-4\).*horizon"):
            critic_values_gae_norm(h, torch.zeros(1, 128, device=DEV), torch.zeros(1, device=DEV), big.clone(), big.bool(), big.bool(), 0.99, 0.95,
                                   torch.zeros(34 * N, device=DEV), big.clone(), big.clone(), st, torch.zeros(6, dtype=torch.float64, device=DEV),
                                   torch.zeros(7, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------ 3. bg_value_norm_update
def test_update_merges_as_the_float64_restatement():
    from booster_gym_amd.utils.utils import value_norm_update

    eps = 1.0e-2
    rng = np.random.default_rng(5)
    batches = [rng.normal(0.05, 0.02, 640), rng.normal(1.5, 0.7, 3072), rng.normal(9.0, 2.5, 1000)]
    state = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=DEV)
    stats = torch.full((3,), float("nan"), device=DEV)
    want = (0.0, 1.0, 0.0)
    for k, x in enumerate(batches):
        sums = torch.tensor([float("nan")] * 3 + [x.sum(), (x * x).sum(), float(x.size)], dtype=torch.float64, device=DEV)  # (sums[0:3] are not read)
        value_norm_update(sums, state, stats, eps)
        want = merge_f64(want, sums[3:].tolist())
        got = state.tolist()
        rel = max(abs(g - w) / abs(w) for g, w in zip(got, want))
        print(f"merge {k}: state {got}, against float64 {rel:.3e}")
        assert rel <= 1e-12 and got[2] == want[2]
        sigma = math.sqrt(got[1]) + eps
        assert stats.tolist() == np.array([got[0], sigma, 1.0 / sigma]).astype(np.float32).tolist()  # the float64 triple, rounded
    seen = np.concatenate(batches)
    assert abs(got[0] - seen.mean()) <= 1e-12 * abs(seen.mean()) and abs(got[1] - seen.var()) <= 1e-12 * seen.var()
    # no rows: nothing is written
    s_before, t_before = state.clone(), stats.clone()
    value_norm_update(torch.tensor([0.0, 0.0, 0.0, 5.0, 7.0, 0.0], dtype=torch.float64, device=DEV), state, stats, eps)
    torch.cuda.synchronize()
    assert torch.equal(state, s_before) and torch.equal(stats, t_before)


# ------------------------------------------------------------------ 4. a Runner under the key
def _cfg(n=128, T=5, E=3, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": n, "terrain.type": "plane", "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "runner.mini_epochs": E,
          "basic.seed": 11, "algorithm.learning_rate": 1.0e-3, KEY: True}
    ov.update(over)
    return load_cfg("T1", ov)


def _runner(**over):
    from booster_gym_amd.utils.runner import Runner

    r = Runner(cfg=_cfg(**over))
    r.begin_training(recorder=_Rec())
    return r


def _gae_f64(rewards, dones, touts, v, v_last):
    """runner.py:132-141 in float64 on rewards whose time-out rows already hold the value: the returns [T][N]."""
    T = rewards.shape[0]
    adv, nxt, out = torch.zeros_like(v_last), v_last, []
    for t in reversed(range(T)):
        nn = (~(dones[t] | touts[t])).double()
        delta = rewards[t] + GAMMA * nn * nxt - v[t]
        adv = delta + GAMMA * LAM * nn * adv
        out.append(v[t] + adv)
        nxt = v[t]
    return torch.stack(out[::-1])


def _both_cells_gradients_f64(rec, r, h0_c, resets_c):
    """step_gradients_f64's loss for a model with both cells (algorithm.rnn_critic): the critic's values walk its cell over the T steps of the step's
    rows from h0_c with the flags resets_c, a zero state behind a reset; every other line is update_grad_ref's."""
    from booster_gym_amd.utils.model import ActorCritic
    from oracle.ppo_ref import surrogate_loss

    alg, H = r.cfg["algorithm"], r._memory
    model = ActorCritic(r.env.num_actions, r.env.num_obs, r.env.num_privileged_obs, r.actor_hidden, r.critic_hidden, memory_hidden=H, critic_memory_hidden=H).to(DEV).double()
    model.load_state_dict({k: v.double() for k, v in rec["params"].items()})
    T, n = rec["resets"].shape
    k_c, k_a = model.critic_memory.input_size, model.memory.input_size
    assert not rec["x_c"][:, k_c:].any() and not rec["x_a"][:, k_a:].any()
    x_c, hc, vs = rec["x_c"][:, :k_c].double().reshape(T, n, -1), h0_c.double(), []
    for t in range(T):
        hc = model.critic_memory(x_c[t], hc * (1 - resets_c[t].double()).view(n, 1))
        vs.append(model.critic(hc).squeeze(-1))
    value_loss = torch.nn.functional.mse_loss(torch.cat(vs), rec["ret"].double())
    adv_all = rec["adv_all"].double().reshape(-1)
    advantages = (rec["adv"].double() - adv_all.mean()) / (adv_all.std() + 1e-8)
    mean = recurrent_means(model, rec["x_a"][:, :k_a].double(), rec["h0"].double(), rec["resets"])
    dist = torch.distributions.Normal(mean, torch.exp(model.logstd).expand_as(mean))
    actor_loss = surrogate_loss(rec["old_logp"].double(), dist.log_prob(rec["actions"].double()).sum(dim=-1), advantages)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    (value_loss + actor_loss + alg["bound_coef"] * bound_loss + alg["entropy_coef"] * dist.entropy().sum(dim=-1).mean()).backward()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _check_gradients(name, r, steps, cells=None):
    """Every recorded step against float64 autograd: each tensor within BOUND of the reference's largest entry, the clip's norm within NORM_BOUND."""
    make_model, alg = model_factory(r), r.cfg["algorithm"]
    assert len(steps) == r.cfg["runner"]["mini_epochs"] * max(r._mini_batches, r._env_mini_batches)
    worst = (0.0, None)
    for s, rec in enumerate(steps):
        assert rec["plan"].value_norm
        ref = step_gradients_f64(rec, make_model, alg) if cells is None else _both_cells_gradients_f64(rec, r, *cells[s])
        assert list(ref) == list(rec["grads"])
        for k, g in ref.items():
            top = g.abs().max().item()
            assert top > 0, k
            e = (rec["grads"][k].double() - g).abs().max().item() / top
            worst = max(worst, (e, f"step {s} {k}"))
            assert e <= BOUND, (name, s, k, e)
        if rec["clip_sqnorm"] is not None:
            norm_ref, used = math.sqrt(sum((g ** 2).sum().item() for g in ref.values())), math.sqrt(rec["clip_sqnorm"].item())
            print(f"{name} step {s}: norm {norm_ref:.6f}, the clip's {used:.6f} ({rec['form']})")
            assert abs(used - norm_ref) <= NORM_BOUND * norm_ref, (name, s, used, norm_ref)
    print(f"{name}: largest error / |ref|max {worst[0]:.3e} ({worst[1]}), bound {BOUND}")


def test_update_under_the_key_matches_float64():
    """128 envs x 5 steps, plane, E = 3, one iteration in front (the statistics have moved off (0, 1, 0)): the gradients; the buffer's returns in reward
    units against a float64 GAE on v; the normaliser after the update against the float64 statistics of the last mini-epoch's returns."""
    r = _runner()
    vn = r.value_norm
    assert vn is not None and r._adv_sums.data_ptr() == vn.sums.data_ptr() and vn.stats.tolist() == [0.0, float(np.float32(1.01)), float(np.float32(1.0 / 1.01))]
    r.iteration()
    torch.cuda.synchronize()
    state0, st0 = vn.state.tolist(), vn.stats.double().tolist()
    assert state0[2] == 640.0 and state0 != [0.0, 1.0, 0.0] and vn.stats.tolist()[1] != float(np.float32(1.01))
    r.rollout()
    plan = r._resolve_plan()
    assert plan.value_norm and plan.ahead and plan.one_tail and plan.chain_values and r._fwd_plan == plan  # the default plan, forward-ahead on
    with record_steps(r) as steps:
        r.update()
    torch.cuda.synchronize()
    _check_gradients("128x5", r, steps)
    # the last mini-epoch's buffers: _values_all holds u, _ret the standardised returns, rewards the values v at time-outs
    m, sigma = st0[0], st0[1]
    T, N, b = 5, 128, r.buffer
    v = sigma * r._values_all.double() + m
    want = _gae_f64(b["rewards"].double(), b["dones"], b["time_outs"], v[: T * N].view(T, N), v[T * N :])
    got = r._ret.double() * sigma + m
    err, top = (got - want).abs().max().item(), want.abs().max().item()
    print(f"returns in reward units against a float64 GAE on v: {err:.3e}, largest return {top:.3e}")
    assert err <= 1e-5 * top
    assert torch.equal(steps[-1]["ret"].reshape(-1), r._ret.reshape(-1))  # what the value loss regressed onto
    # the statistics: the state in front of the update merged with the last mini-epoch's un-normalised returns
    R = got.reshape(-1).cpu().numpy()
    want_state = merge_f64(state0, (R.sum(), (R * R).sum(), float(R.size)))
    got_state = vn.state.tolist()
    rel = max(abs(g - w) / abs(w) for g, w in zip(got_state, want_state))
    print(f"normaliser after the update {got_state}, float64 {want_state}: {rel:.3e}")
    assert rel <= 1e-6 and got_state[2] == 1280.0
    s = math.sqrt(got_state[1]) + 1.0e-2
    assert vn.stats.tolist() == np.array([got_state[0], s, 1.0 / s]).astype(np.float32).tolist()
    # the public way to a value in reward units
    u = r._values_all[:7].clone()
    exact = vn.stats[1].double() * u.double() + vn.stats[0].double()
    assert bool(((vn.denormalize(u).double() - exact).abs() <= 2.0 ** -24 * exact.abs()).all()) and torch.equal(u, r._values_all[:7])  # (a new tensor)


def test_gradients_with_row_mini_batches():
    """256 envs, runner.num_mini_batches: 2 (two mini-batches of 640 rows): the gathered standardised returns are the steps' targets."""
    r = _runner(n=256, E=2, **{"runner.num_mini_batches": 2})
    r.iteration()
    r.rollout()
    with record_steps(r) as steps:
        r.update()
    torch.cuda.synchronize()
    assert r._mb_plan is not None and steps[0]["rows"] == 640 and not torch.equal(steps[0]["ret"], steps[1]["ret"])
    _check_gradients("256x5, two mini-batches", r, steps)


def test_gradients_with_both_cells():
    """100 envs x 5 steps, algorithm.rnn_hidden_size: 128 with algorithm.rnn_critic: the critic's cell regresses onto the standardised returns."""
    from test_gpu_actor_memory import SHORT_EPISODES

    r = _runner(n=100, E=2, **{"algorithm.rnn_hidden_size": 128, "algorithm.rnn_critic": True, **SHORT_EPISODES})
    assert r._cmem_tr is not None and r.value_norm is not None
    r.iteration()
    r.rollout()
    cells, inner = [], r._epoch_gradients_and_step

    def keep(u, v):  # (inside record_steps' wrapper: the critic's state and flags of the step, which the record does not carry)
        cells.append((v.cmem.h0.clone(), v.cmem.resets.clone()))
        inner(u, v)

    r._epoch_gradients_and_step = keep
    with record_steps(r) as steps:
        r.update()
    torch.cuda.synchronize()
    assert len(cells) == len(steps) == 2 and cells[0][0].abs().max().item() > 1e-3
    _check_gradients("100x5, both cells", r, steps, cells)


def _digest(r):
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr, r.value_norm.state, r.value_norm.stats]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_two_iterations_are_deterministic_and_logged():
    digests = []
    for rep in range(2):
        r = _runner(E=2)
        for it in range(2):
            r.train_iteration(it)
        r._flush_log()
        torch.cuda.synchronize()
        digests.append(_digest(r))
        if rep == 0:
            for it in range(2):
                s = r.recorder.stats[it]
                assert s["value_norm/count"] == 640.0 * (it + 1) and s["value_norm/std"] > 0 and math.isfinite(s["value_norm/mean"]) and math.isfinite(s["value_loss"])
            assert r.recorder.stats[1]["value_norm/mean"] == r.value_norm.state.tolist()[0] and r.value_norm.scalars() == {k: v for k, v in r.recorder.stats[1].items() if k.startswith("value_norm/")}
        del r
    print("sha256 after two iterations:", digests)
    assert digests[0] == digests[1]


def test_runner_refuses_a_horizon_above_32():
    from booster_gym_amd.utils.runner import Runner

    with pytest.raises(ValueError, match=r"algorithm\.normalize_value needs runner\.horizon_length of 32 or less, got 33"):
        Runner(cfg=_cfg(n=16, T=33))


# ------------------------------------------------------------------ 5. the launch sequence, key off and on
def _recipe():
    spec = importlib.util.spec_from_file_location("make_launch_sequences", os.path.join(ROOT, "tests", "golden", "make_launch_sequences.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launch_sequence_key_off_and_on(monkeypatch):
    from booster_gym_amd import _lib
    from test_gpu_estimator import _runner as est_runner

    recipe, lib = _recipe(), _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "launch_sequences.json")) as f:
        want = json.load(f)["ppo_default_plan"]
    # key absent: none of the three entry points is reached, and the update's launches are the record's
    with monkeypatch.context() as mp:
        def forbidden(*a):
            raise AssertionError("an entry point of algorithm.normalize_value ran without the key")

        for name in NEW:
            mp.setattr(lib, name, forbidden)
        got, _ = recipe.record("ppo_default_plan", None)
    assert got == want
    # key on: one name per mini-epoch differs, and one bg_value_norm_update per iteration stands behind the last optimiser step
    r = est_runner(1, 128, **recipe.PPO, **{KEY: True})
    E = r.cfg["runner"]["mini_epochs"]
    with recipe.spy() as seq:
        for it in range(recipe.ITERATIONS):
            del seq[:]
            r.train_iteration(it)
            g = list(seq)
            assert g.count("bg_critic_values_gae_norm") == E and g.count("bg_value_norm_update") == 1 and "bg_critic_values_gae" not in g and "bg_value_denormalize" not in g
            at = g.index("bg_value_norm_update")
            assert at > max(k for k, n in enumerate(g) if n in ("bg_update_tail", "bg_critic_values_gae_norm"))
            same = [("bg_critic_values_gae" if n == "bg_critic_values_gae_norm" else n) for n in g[:at] + g[at + 1 :]]
            assert same == want[it], it
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. checkpoints
def test_checkpoint_round_trip_and_mismatches(tmp_path):
    from booster_gym_amd.utils.runner import Runner

    r = _runner(E=2)
    r.train_iteration(0)
    r._flush_log()
    torch.cuda.synchronize()
    ck = r.checkpoint_dict()
    assert sorted(ck["value_normalizer"]) == ["count", "eps", "mean", "var"] and ck["value_normalizer"]["count"] == 640.0 and ck["value_normalizer"]["eps"] == 1.0e-2
    assert not any("value_norm" in k for k in ck["model"])
    state, stats = r.value_norm.state.clone(), r.value_norm.stats.clone()
    on, off = str(tmp_path / "on.pth"), str(tmp_path / "off.pth")
    torch.save(ck, on)
    torch.save({k: v for k, v in ck.items() if k != "value_normalizer"}, off)
    del r
    p = Runner(cfg=_cfg(E=2, **{"basic.checkpoint": on}))
    assert torch.equal(p.value_norm.state, state) and torch.equal(p.value_norm.stats, stats)
    del p
    with pytest.raises(ValueError, match=r"carries a value normaliser but the config has algorithm\.normalize_value: false"):
        Runner(cfg=_cfg(E=2, **{KEY: False, "basic.checkpoint": on}))
    with pytest.raises(ValueError, match=r"has no value normaliser but the config sets algorithm\.normalize_value: true"):
        Runner(cfg=_cfg(E=2, **{"basic.checkpoint": off}))
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value.*algorithm\.normalization_eps = 0\.01, the config has 0\.05"):
        Runner(cfg=_cfg(E=2, **{"algorithm.normalization_eps": 0.05, "basic.checkpoint": on}))
    # a runner that plays never evaluates the critic: either setting loads either checkpoint
    for key, path in ((False, on), (True, on), (True, off)):
        q = Runner(test=True, cfg=_cfg(E=2, **{KEY: key, "basic.checkpoint": path}))
        assert q.value_norm is None
        del q
