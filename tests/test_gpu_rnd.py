"""Random network distillation on the GPU (rnd.enabled): the rollout's launch bg_rnd_reward against the existing single-network launch (bitwise
embeddings) and float64, and a Runner under the section: the key off against the section absent, weight 0 against the key off, the rewards that enter
GAE, the reward normaliser, one predictor step against float64 autograd and Adam, the target, checkpoints, and a composition run."""
import hashlib
import math

import numpy as np
import pytest
import torch

from supervised_grad_ref import net_factory, record_supervised_steps, supervised_gradients_f64
from test_gpu_actor_memory import SHORT_EPISODES
from test_gpu_estimator import _Rec, _descs, _spy_all
from test_gpu_supervised_gradients import LOSS_BOUND
from test_gpu_update_gradients import BOUND, NORM_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 12
GUARD = 16  # sentinel rows behind every output
NEW = ("bg_rnd_reward",)


# ------------------------------------------------------------------ 1. the launch
def _nets(K, target_hidden, pred_hidden=(256, 128), seed=3):
    from booster_gym_amd.utils.model import _mlp

    torch.manual_seed(seed)
    return _mlp(K, target_hidden, A).to(DEV), _mlp(K, pred_hidden, A).to(DEV)


def _embedding(net, rows):
    """The existing launch's mean of `net` on contiguous rows: the reference of both embeddings.  bg_actor_sample_mlp_scan checks that the columns in
    front of its scan_points are 47 H; the arithmetic does not depend on the split, so scan_points = K mod 47: priv_cols for rows of 47 H observations
    and a privileged block of 14, and the one admissible split for the rows of 234 observation columns (47 + 187: no multiple of 47)."""
    from booster_gym_amd import _lib

    n, K = rows.shape
    d, nl = _descs(net)
    mu, act, logstd = torch.empty(n, A, device=DEV), torch.empty(n, A, device=DEV), torch.zeros(A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp_scan(n, _lib.ptr(rows), nl, d, K % 47, _lib.ptr(logstd), 1, 0, _lib.ptr(mu), _lib.ptr(act), _lib.current_stream_ptr()),
               "bg_actor_sample_mlp_scan")
    return mu


def _launch(n, obs, priv, target, pred, dones, stats, weight, rew):
    """One bg_rnd_reward on fresh outputs with GUARD sentinel rows behind row n: (target_out, intrinsic, rewards), whole buffers."""
    from booster_gym_amd import _lib

    td, nt = _descs(target)
    pd, npr = _descs(pred)
    t_out, rho, r = torch.full((n + GUARD, A), 7.0, device=DEV), torch.full((n + GUARD,), 7.0, device=DEV), torch.full((n + GUARD,), 7.0, device=DEV)
    r[:n] = rew
    _lib.check(_lib.load().bg_rnd_reward(n, _lib.ptr(obs), obs.shape[1], _lib.ptr(priv), 0 if priv is None else priv.shape[1], nt, td, npr, pd, _lib.ptr(dones),
                                         _lib.ptr(stats), weight, _lib.ptr(t_out), _lib.ptr(rho), _lib.ptr(r), _lib.current_stream_ptr()), "bg_rnd_reward")
    torch.cuda.synchronize()
    return t_out, rho, r


# (N, obs_cols, priv_cols, the target's hidden widths): a ragged last workgroup, one full workgroup, one row; the critic's and the actor's state;
# the 512 LDS form through a width, and through the 288-column tile of 234 + 14 = 248 columns; the other three wide rows pad to 192 / 144 / 240
CASES = [(37, 47, 14, (256, 128)), (16, 47, 14, (256, 128)), (1, 47, 14, (256, 128)), (37, 47, 0, (256, 128)), (1, 47, 0, (256, 128)),
         (37, 47, 14, (512, 128)), (16, 47, 0, (512, 128)),
         (37, 141, 14, (256, 128)), (37, 141, 0, (256, 128)), (37, 234, 14, (256, 128)), (37, 234, 0, (256, 128))]


@pytest.mark.parametrize("n,oc,pc,target_hidden", CASES)
def test_launch_against_the_single_network_launch_and_float64(n, oc, pc, target_hidden):
    K = oc + pc
    target, pred = _nets(K, target_hidden)
    g = torch.Generator(device="cpu").manual_seed(100 + n + K)
    obs = (torch.randn(n, oc, generator=g) * 0.7).to(DEV)
    priv = (torch.randn(n, pc, generator=g) * 0.7).to(DEV) if pc else None
    rew = torch.randn(n, generator=g).to(DEV)
    rew[0] = -0.0
    dones = (torch.rand(n, generator=g) < 0.3).to(DEV)
    dones[0] = False  # (every case has a live row, N = 1 included; row 0 carries the -0.0)
    if n > 2:
        dones[1], dones[2] = True, False
    dones_u8 = dones.view(torch.uint8)
    stats = torch.tensor([0.3, 0.37, 1.0 / 0.37], dtype=torch.float64).float().to(DEV)
    weight = 0.5
    rows = (torch.cat((obs, priv), dim=1) if pc else obs).contiguous()
    t_ref, p_ref = _embedding(target, rows), _embedding(pred, rows)
    t_out, rho, r = _launch(n, obs, priv, target, pred, dones_u8, stats, weight, rew)
    live = ~dones
    # the target's embedding: the existing launch's mean, bit for bit
    assert torch.equal(t_out[:n], t_ref), "target_out is not bg_actor_sample_mlp_scan's mu of the target on the concatenated rows"
    # rho against float64 on the two bit-exact embeddings: 12 squares and their sum in fp32, 13 roundings of 2^-24 at most, and the root's half ulp
    want = (p_ref.double() - t_ref.double()).pow(2).sum(dim=1).sqrt()
    tiny = want < 1e-30
    assert int(tiny.sum()) == 0, "a row fell under the absolute rule"
    rel = ((rho[:n].double() - want).abs() / want)[live]
    print(f"N {n} K {oc}+{pc} target {target_hidden}: rho in [{want.min().item():.3e}, {want.max().item():.3e}], max relative error "
          f"{rel.max().item() if rel.numel() else 0.0:.3e} (bound 2e-6), {int(dones.sum())} rows done")
    assert bool((rel <= 2e-6).all())
    assert bool((rho[:n][dones] == 0).all()) and bool((rho[:n][live] > 0).all())
    # rewards: untouched bits where done; elsewhere within 1 ulp of the float64 sum, rounded to fp32, on the launch's own fp32 operands
    r_bits, rew_bits = r[:n].view(torch.int32), rew.view(torch.int32)
    assert torch.equal(r_bits[dones], rew_bits[dones])
    exact = rew.double() + float(np.float32(weight)) * stats[2].double() * rho[:n].double()
    want32 = exact.float()
    ulp = torch.from_numpy(np.spacing(np.abs(want32.cpu().numpy()))).to(DEV)
    assert bool(((r[:n] - want32).abs() <= ulp)[live].all()), (r[:n] - want32).abs().max().item()
    assert not torch.equal(r[:n][live], rew[live])
    # guards: nothing behind row n
    assert bool((t_out[n:] == 7.0).all()) and bool((rho[n:] == 7.0).all()) and bool((r[n:] == 7.0).all())
    # weight 0 (of either sign): rewards bit-identical everywhere, the -0.0 included; the other outputs as before
    for w0 in (0.0, -0.0):
        t0, rho0, r0 = _launch(n, obs, priv, target, pred, dones_u8, stats, w0, rew)
        assert torch.equal(r0[:n].view(torch.int32), rew_bits) and torch.equal(t0, t_out) and torch.equal(rho0, rho)
    # reward_stats NULL = the triple (0, 1, 1)
    one = torch.tensor([0.0, 1.0, 1.0], device=DEV)
    a, b = _launch(n, obs, priv, target, pred, dones_u8, None, weight, rew), _launch(n, obs, priv, target, pred, dones_u8, one, weight, rew)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[1], rho)
    # the predictor counts: another predictor, another rho, the same labels
    _, other = _nets(K, target_hidden, seed=4)
    t2, rho2, _ = _launch(n, obs, priv, target, other, dones_u8, stats, weight, rew)
    assert torch.equal(t2, t_out) and not torch.equal(rho2[:n][live], rho[:n][live])


def test_launch_argument_errors():
    from booster_gym_amd import _lib

    lib, p = _lib.load(), _lib.ptr
    n = 16
    target, pred = _nets(61, (256, 128))
    actor_t, actor_p = _nets(47, (256, 128))
    obs, priv, dones = torch.zeros(n, 47, device=DEV), torch.zeros(n, 14, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    outs = [torch.full((n, A), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)]
    td, nt = _descs(target)
    pd, npr = _descs(pred)
    atd, _ = _descs(actor_t)
    apd, _ = _descs(actor_p)

    def call(N=n, obs=obs, oc=47, priv=priv, pc=14, nt=nt, td=td, npr=npr, pd=pd, dones=dones, w=0.5, t_out=outs[0], rho=outs[1], rew=outs[2]):
        return lib.bg_rnd_reward(N, p(obs), oc, p(priv), pc, nt, td, npr, pd, p(dones), None, w, p(t_out), p(rho), p(rew), _lib.current_stream_ptr())

    assert call(N=0) == -1 and call(obs=None) == -1 and call(dones=None) == -1 and call(t_out=None) == -1 and call(rho=None) == -1 and call(rew=None) == -1
    assert call(priv=None) == -1 and b"priv" in lib.bg_last_error()      # priv_cols without priv
    assert call(pc=0) == -1 and b"priv" in lib.bg_last_error()           # priv without priv_cols
    assert call(oc=0) == -1 and call(pc=-1) == -1
    for w in (-0.5, float("inf"), float("nan")):
        assert call(w=w) == -1 and b"weight" in lib.bg_last_error()
    assert call(oc=470) == -4 and b"BG_ACTOR_MAX_INPUT" in lib.bg_last_error()   # 470 + 14 = 484 columns
    assert call(td=atd) == -4 and b"(target)" in lib.bg_last_error()      # a target of 47 inputs on a row of 61
    assert call(pd=apd) == -4 and b"(predictor)" in lib.bg_last_error()
    assert call(nt=2) == -4 and b"(target)" in lib.bg_last_error()        # one hidden layer
    assert call(npr=6) == -4 and b"(predictor)" in lib.bg_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs), "an argument error launched"
    assert call() == 0 and call(priv=None, pc=0, td=atd, pd=apd) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the Runner
T, N = 8, 128
SCHED = {"mode": "linear", "initial_step": 1, "final_step": 5, "final_value": 0.1}


def _cfg(n=N, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": n, "terrain.type": "plane", "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "runner.mini_epochs": 2,
          "basic.seed": 11, "algorithm.learning_rate": 1.0e-3, "rnd.enabled": True, "rnd.weight": 0.5, **SHORT_EPISODES}
    ov.update(over)
    return load_cfg("T1", ov)


def _runner(cfg=None, **over):
    from booster_gym_amd.utils.runner import Runner

    r = Runner(cfg=cfg if cfg is not None else _cfg(**over))
    r.begin_training(recorder=_Rec())
    return r


def _ppo_sha(r):
    """SHA-256 over PPO's parameters and Adam moments (what an iteration without the section leaves)."""
    o, h = r.optimizer, hashlib.sha256()
    for t in [p for k, p in r.model.state_dict().items() if not k.startswith("rnd_")] + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr]:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def key_off():
    """Two iterations with the section off: the SHA the other runs are held to."""
    r = _runner(**{"rnd.enabled": False})
    for it in range(2):
        r.train_iteration(it)
    torch.cuda.synchronize()
    return _ppo_sha(r)


def test_off_means_off(monkeypatch, key_off):
    seq = _spy_all(monkeypatch)
    runs = []
    for absent in (True, False):
        cfg = _cfg(**{"rnd.enabled": False})
        if absent:
            del cfg["rnd"]
        r = _runner(cfg=cfg)
        assert r._rnd is None and r._rnd_trainer is None and "intrinsic_rewards" not in r.buffer and "rnd_targets" not in r.buffer
        del seq[:]
        r.train_iteration(0)
        r.train_iteration(1)
        r._flush_log()
        torch.cuda.synchronize()
        runs.append((list(seq), _ppo_sha(r), sorted(r.checkpoint_dict()), [k for k, _ in r.model.named_parameters()], sorted(r.recorder.stats[1])))
    assert runs[0] == runs[1] and not any(s in runs[0][0] for s in NEW)
    assert runs[0][1] == key_off and "rnd" not in runs[0][2] and not any("rnd" in k for k in runs[0][3] + runs[0][4])
    # ... and with the key on the new launch runs once per env step, behind it
    r = _runner()
    del seq[:]
    r.iteration()
    torch.cuda.synchronize()
    assert seq.count("bg_rnd_reward") == T and seq.count("bg_distill_head_partial") == 1 and seq.count("bg_value_norm_update") == 1
    steps = [k for k, s in enumerate(seq) if s == "bg_env_step_to"]
    assert len(steps) == T and all(seq[k + 1] == "bg_rnd_reward" for k in steps)
    assert seq.index("bg_distill_head_partial") > max(k for k, s in enumerate(seq) if s in ("bg_update_tail", "bg_optimizer_step"))
    assert r._resolve_plan().ahead  # the forward-ahead stays on: it never reads rewards


def test_weight_zero_leaves_ppo_alone(key_off):
    r = _runner(**{"rnd.weight": 0})
    names = [k for k, _ in r.model.named_parameters()]
    assert names[-12:] == [f"rnd_predictor.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")] + [f"rnd_target.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")]
    assert len(r.optimizer.params) == len(names) - 12 and all(p is q for p, q in zip(r.optimizer.params, r.model.ppo_parameters()))
    assert all(p.grad is None for p in r.model.rnd_target.parameters())  # no optimiser, no gradient buffers
    target0 = [p.detach().clone() for p in r.model.rnd_target.parameters()]
    pred0 = [p.detach().clone() for p in r.model.rnd_predictor.parameters()]
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    assert _ppo_sha(r) == key_off
    assert all(torch.equal(a, b) for a, b in zip(target0, r.model.rnd_target.parameters())), "the target moved"
    assert not any(torch.equal(a, b) for a, b in zip(pred0, r.model.rnd_predictor.parameters())), "the predictor did not train"
    s = r.recorder.stats[1]
    assert s["rnd/weight"] == 0.0 and s["rnd/intrinsic_reward"] > 0 and s["rnd/reward_std"] > 0 and s["rnd/loss"] > 0 and all(math.isfinite(v) for v in s.values())


def _rho_f64(r, pred_sd, t):
    """rho of step t in float64 from the state dicts and the buffer's rows t + 1: zero where the step ended an episode."""
    from booster_gym_amd.utils.model import _mlp

    rnd, b = r._rnd, r.buffer
    s = torch.cat((b["obses"][t + 1], b["privileged_obses"][t + 1]), dim=-1).double() if rnd.state == "critic" else b["obses"][t + 1].double()
    tgt, pred = _mlp(rnd.width, rnd.target_hidden, A).to(DEV).double(), _mlp(rnd.width, rnd.predictor_hidden, A).to(DEV).double()
    tgt.load_state_dict({k: v.double() for k, v in r.model.rnd_target.state_dict().items()})
    pred.load_state_dict({k: v.double() for k, v in pred_sd.items()})
    with torch.no_grad():
        rho = (pred(s) - tgt(s)).pow(2).sum(dim=-1).sqrt()
    return torch.where(b["dones"][t], torch.zeros_like(rho), rho)


def test_rewards_entering_gae_normaliser_and_target():
    """Three iterations at weight 0.5.  The env's rewards of iteration 1 are a weight-0 run's on the same seeds (rewards do not reach the rollout before
    the first update), which also checks the copies taken in front of each launch; those copies are the env's rewards of the later iterations, whose
    rollouts a weight-0 run no longer shares.  rho in float64 from the state dicts; sigma from the host's merge of the float64 rho."""
    from booster_gym_amd.utils.rnd import merge_f64

    zero = _runner(**{"rnd.weight": 0})
    zero.rollout()
    torch.cuda.synchronize()
    env_rewards_1 = zero.buffer["rewards"].clone()
    del zero
    r = _runner()
    rt, eps = r._rnd_trainer, 1.0e-2
    assert rt.norm.state.tolist() == [0.0, 1.0, 0.0] and tuple(r.buffer["intrinsic_rewards"].shape) == (T, N) and tuple(r.buffer["rnd_targets"].shape) == (T, N, A)
    target0 = [p.detach().clone() for p in r.model.rnd_target.parameters()]
    taken, inner = [], rt.reward

    def keep(obs, priv, dones, t_out, rho, rew):
        taken.append(rew.clone())
        inner(obs, priv, dones, t_out, rho, rew)

    rt.reward = keep
    state_host, state_dev, worst = (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.0
    for it in range(3):
        pred_sd = {k: v.detach().clone() for k, v in r.model.rnd_predictor.state_dict().items()}
        del taken[:]
        r.rollout()
        torch.cuda.synchronize()
        env_rew, got = torch.stack(taken), r.buffer["rewards"].clone()
        if it == 0:
            assert torch.equal(env_rew, env_rewards_1)
        assert bool(r.buffer["dones"].any()) and not bool(r.buffer["dones"].all())
        rho = torch.stack([_rho_f64(r, pred_sd, t) for t in range(T)])
        sigma = math.sqrt(state_host[1]) + eps
        if it < 2:  # the rewards entering GAE in iterations 1 and 2
            want = env_rew.double() + 0.5 / sigma * rho
            err, top = (got.double() - want).abs().max().item(), want.abs().max().item()
            worst = max(worst, err / top)
            print(f"iteration {it + 1}: rewards entering GAE against float64: {err:.3e}, largest entry {top:.3e} ({err / top:.3e}); sigma {sigma:.6f}")
            assert err <= 1e-5 * top
            assert (got - env_rew)[~r.buffer["dones"]].min().item() > 0 and torch.equal(got[r.buffer["dones"]], env_rew[r.buffer["dones"]])
        logged = r.buffer["intrinsic_rewards"].double()
        assert (logged - rho).abs().max().item() <= 1e-5 * rho.max().item() and bool((logged[r.buffer["dones"]] == 0).all())
        count = float((~r.buffer["dones"]).sum().item())
        state_host = merge_f64(state_host, (rho.sum().item(), (rho * rho).sum().item(), count))
        state_dev = merge_f64(state_dev, (logged.sum().item(), (logged * logged).sum().item(), count))
        r.update()
        r.buffer.roll()
        torch.cuda.synchronize()
    # the normaliser after three iterations: the host's Chan merge of the logged intrinsic rewards
    got_state = rt.norm.state.tolist()
    rel = max(abs(g - w) / abs(w) for g, w in zip(got_state, state_dev))
    print(f"normaliser after three iterations {got_state}, the host's merge {list(state_dev)}: {rel:.3e}; largest reward error / largest entry {worst:.3e}")
    assert rel <= 1e-12 and got_state[2] == state_dev[2] < 3 * T * N
    s = math.sqrt(got_state[1]) + eps
    assert rt.norm.stats.tolist() == np.array([got_state[0], s, 1.0 / s]).astype(np.float32).tolist()
    assert all(torch.equal(a, b) for a, b in zip(target0, r.model.rnd_target.parameters())), "the target moved"


def test_one_predictor_step_is_float64_autograd_and_adam():
    """The gradient in front of bg_adam_step against float64 autograd of 1 / (12 B) sum |pred - tgt|^2 on the same rows, by the bounds
    tests/test_gpu_supervised_gradients.py holds the estimator's steps to; then the parameters behind the step against a float64 Adam step (the
    global-norm clip, lr 1e-3, the first step) on that gradient: fp32 rounding of the moments and the quotient, 1e-5 of the step's lr, and one ulp of
    the parameter."""
    r = _runner()
    rt, b = r._rnd_trainer, r.buffer
    r.rollout()
    torch.cuda.synchronize()
    x = torch.cat((b["obses"][1:], b["privileged_obses"][1:]), dim=-1).reshape(T * N, -1)
    with record_supervised_steps(rt.sup) as steps:
        rt.update(b["obses"][1:], b["privileged_obses"][1:], b["dones"], b["rnd_targets"], b["intrinsic_rewards"])
    torch.cuda.synchronize()
    assert len(steps) == 1
    rec = steps[0]
    assert torch.equal(rec["x"][:, :61], x) and not rec["x"][:, 61:].any() and torch.equal(rec["target"], b["rnd_targets"].reshape(-1, A)) and rec["rows"] == T * N
    aux = {}
    ref = supervised_gradients_f64(rec, net_factory(rt.sup), aux=aux)
    for k, g in ref.items():
        top = g.abs().max().item()
        e = (rec["grads"][k].double() - g).abs().max().item() / top
        print(f"{k}: gradient error / |ref|max {e:.3e} (bound {BOUND})")
        assert top > 0 and e <= BOUND, (k, e)
    norm_ref, used = math.sqrt(sum((g ** 2).sum().item() for g in ref.values())), math.sqrt(rec["clip_sqnorm"].item())
    assert abs(used - norm_ref) <= NORM_BOUND * norm_ref
    got_loss = rec["stats"][0].item() / (A * T * N)
    assert abs(got_loss - aux["cloning_loss"]) <= LOSS_BOUND * aux["cloning_loss"] and abs(rt.loss.item() - got_loss) <= 1e-12 * got_loss
    lr, clip = r._rnd.learning_rate, min(1.0, r._rnd.max_grad_norm / (used + 1e-6))
    for k, p in rec["params"].items():
        now = dict(zip(rec["params"], rt.optimizer.params))[k]
        g = rec["grads"][k].double() * clip
        m, v = 0.1 * g / (1 - 0.9), 0.001 * g * g / (1 - 0.999)
        want = p.double() - lr * m / (v.sqrt() + 1e-8)
        err = (now.double() - want).abs()
        assert bool((err <= 1e-5 * lr + 2.0 ** -23 * want.abs()).all()), (k, err.max().item())
        assert not torch.equal(now, p)


def test_checkpoint_round_trip_schedule_and_mismatches(tmp_path):
    from booster_gym_amd.utils.rnd import weight_at
    from booster_gym_amd.utils.runner import Runner

    over = {"rnd.weight_schedule": SCHED}
    r = _runner(**over)
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    assert [r.recorder.stats[it]["rnd/weight"] for it in range(2)] == [0.5, 0.5] and r._rnd_trainer.iteration == 2
    ck = r.checkpoint_dict()
    assert sorted(ck["rnd"]) == ["iteration", "normalizer", "optimizer", "predictor_hidden", "state", "target_hidden"]
    assert ck["rnd"]["iteration"] == 2 and ck["rnd"]["state"] == "critic" and ck["rnd"]["predictor_hidden"] == [256, 128] and ck["rnd"]["normalizer"]["eps"] == 1.0e-2
    assert sum(k.startswith("rnd_predictor.") for k in ck["model"]) == 6 and sum(k.startswith("rnd_target.") for k in ck["model"]) == 6
    assert len(ck["optimizer"]["state"]) == 17 and len(ck["rnd"]["optimizer"]["state"]) == 6
    on, off = str(tmp_path / "on.pth"), str(tmp_path / "off.pth")
    torch.save(ck, on)
    torch.save({"model": {k: v for k, v in ck["model"].items() if not k.startswith("rnd_")}, **{k: v for k, v in ck.items() if k not in ("model", "rnd")}}, off)
    q = Runner(cfg=_cfg(**over, **{"basic.checkpoint": on}))
    a, b = r._rnd_trainer, q._rnd_trainer
    for net in ("rnd_predictor", "rnd_target"):
        assert all(torch.equal(x, y) for x, y in zip(getattr(r.model, net).parameters(), getattr(q.model, net).parameters())), net
    assert torch.equal(a.optimizer.exp_avg, b.optimizer.exp_avg) and torch.equal(a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq) and b.optimizer.step_count == 2
    assert torch.equal(a.norm.state, b.norm.state) and torch.equal(a.norm.stats, b.norm.stats) and b.iteration == 2
    q.begin_training(recorder=_Rec())
    q.train_iteration(2)  # the schedule continues: iteration 2 of the ramp 0.5 -> 0.1 over iterations 1 .. 5
    q._flush_log()
    torch.cuda.synchronize()
    assert q.recorder.stats[2]["rnd/weight"] == pytest.approx(weight_at(q._rnd, 2), rel=1e-15) == pytest.approx(0.4, rel=1e-12) and b.iteration == 3
    del q
    # a training Runner: checkpoint and config must agree about the key, the state kind and the widths
    with pytest.raises(ValueError, match=r"with random network distillation.*rnd\.enabled: false"):
        Runner(cfg=_cfg(**{"rnd.enabled": False, "basic.checkpoint": on}))
    with pytest.raises(ValueError, match=r"without random network distillation.*rnd\.enabled: true"):
        Runner(cfg=_cfg(**{"basic.checkpoint": off}))
    with pytest.raises(ValueError, match=r"rnd\.state = 'critic' of 61 columns.*rnd\.state = 'actor' has 47"):
        Runner(cfg=_cfg(**{"rnd.state": "actor", "basic.checkpoint": on}))
    with pytest.raises(ValueError, match=r"rnd_predictor hidden widths \[256, 128\].*rnd\.predictor_hidden = \[128, 128\]"):
        Runner(cfg=_cfg(**{"rnd.predictor_hidden": [128, 128], "basic.checkpoint": on}))
    with pytest.raises(ValueError, match=r"rnd_target hidden widths \[256, 128\].*rnd\.target_hidden = \[512, 128\]"):
        Runner(cfg=_cfg(**{"rnd.target_hidden": [512, 128], "basic.checkpoint": on}))
    # a runner that plays never evaluates these networks: either checkpoint under either setting, and with the section absent
    for enabled, path in ((False, on), (True, on), (True, off), (None, on)):
        cfg = _cfg(**{"rnd.enabled": bool(enabled), "basic.checkpoint": path})
        if enabled is None:
            del cfg["rnd"]
        p = Runner(test=True, cfg=cfg)
        assert p._rnd is None and not hasattr(p.model, "rnd_target") and p.play(max_steps=2) == 2


def test_composition_with_mini_batches_value_norm_and_the_height_scan():
    """rnd on state "critic" of 61 + 187 = 248 columns (the 512 LDS form through the 288-column tile) with runner.num_mini_batches: 2 and
    algorithm.normalize_value: two iterations, finite logs."""
    r = _runner(**{"runner.num_mini_batches": 2, "algorithm.normalize_value": True, "terrain.type": "trimesh", "terrain.measure_heights": True,
                   "env.num_privileged_obs": 14 + 187})
    assert r._rnd.width == 248 and r._rnd_trainer.x.shape[1] == 256 and r._mini_batches == 2 and r.value_norm is not None
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    for it in range(2):
        s = r.recorder.stats[it]
        assert all(math.isfinite(v) for v in s.values()) and s["rnd/intrinsic_reward"] > 0 and s["rnd/loss"] > 0 and s["value_norm/count"] == T * N * (it + 1)
    assert r.recorder.stats[1]["rnd/reward_std"] != r.recorder.stats[0]["rnd/reward_std"]
    assert torch.isfinite(r.optimizer.flat).all() and torch.isfinite(r._rnd_trainer.optimizer.flat).all()
