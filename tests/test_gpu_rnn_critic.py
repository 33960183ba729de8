"""algorithm.rnn_critic on the GPU: a recurrent critic beside the recurrent actor of algorithm.rnn_hidden_size.  The grouped recurrences
(bg_gru_sequence_forward_group / _backward_group) bit for bit against the single launches; one update against float64 autograd through time for both
cells and against the reference's loop (oracle/ppo_ref.py, unedited) on a restated model whose est_value walks the critic's cell; the rules of the
critic's carried state; the first step of an env-wise mini-batch against float64 autograd and BG_GRU_GROUP on against off; the key off against today's
calls; training, saving, resuming, evaluating and exporting.

Shapes and bounds are tests/test_gpu_actor_memory.py's: N = 40 envs (two 16-row tiles and a tail of 8), T = 5, plane terrain; forward quantities
2e-5 max(1, |ref|max) (_bound), gradients 1e-4 of the tensor's largest entry (_grad_bound), parameters after an update rtol 1e-3 / atol 2e-6 at the
learning rate 1e-5 with _assert_same_adam_steps, logged losses 2e-4 max(1, |ref|)."""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_actor_memory import CLIP, SHORT_EPISODES, _Restated
from test_gpu_distill import _Rec
from test_gpu_distill_memory import _bound, _grad_bound
from test_gpu_env_mini_batches import _by_envs, _is_permutation
from test_gpu_ppo import _assert_same_adam_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, NO, N, T, H = 12, 47, 40, 5, 128
KEY, RNN, KMB = "algorithm.rnn_critic", "algorithm.rnn_hidden_size", "runner.num_env_mini_batches"
GROUP_ENTRY_POINTS = ("bg_gru_sequence_forward_group", "bg_gru_sequence_backward_group")
CELL = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
FEET = {"env.privileged_extras": ["feet"], "env.num_privileged_obs": 20}  # 47 + 20 = 67 columns: the critic's cell reads rows padded to 128


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "terrain.type": "plane", "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "runner.mini_epochs": 2,
          RNN: H, KEY: True}
    ov.update(over)
    return load_cfg("T1", ov)


def _runner(cfg=None, **over):
    from booster_gym_amd.utils.runner import Runner

    r = Runner(cfg=cfg if cfg is not None else _cfg(**over))
    r.begin_training(recorder=_Rec())
    return r


def _digest(r):
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr, r.model._memory_state, r._last_dones, r._cmem_tr.next_state]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ 1. the grouped recurrences against the single launches
GUARD, SENTINEL = 8, -7.0  # rows behind the last row of every output


class _Problem:
    """One recurrence on random operands: (T, N) steps x envs of width Hc, a state h0 that is not zero, reset flags, weights of its own."""

    def __init__(self, Tp, Np, Hc, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
        self.T, self.N, self.H = Tp, Np, Hc
        self.gi, self.h0, self.dh_ext = rnd(Tp * Np, 3 * Hc), rnd(Np, Hc) * 0.5, rnd(Tp * Np, Hc)
        self.reset = (torch.rand(Tp, Np, device=DEV, generator=g) < 0.3).to(torch.uint8)
        self.reset[0, 0], self.reset[-1, -1] = 1, 1
        self.W, self.b = rnd(3 * Hc, Hc) / Hc ** 0.5, rnd(3 * Hc) * 0.1

    def outputs(self):
        new = lambda rows, w: torch.full((rows + GUARD, w), SENTINEL, device=DEV)
        B, Hc = self.T * self.N, self.H
        return {"h_prev": new(B, Hc), "h": new(B, Hc), "gates": new(B, 4 * Hc), "dgi": new(B, 3 * Hc), "dgh": new(B, 3 * Hc), "dh0": new(self.N, Hc)}


def _single(q, o, bare):
    from booster_gym_amd import _lib

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()
    h0, reset = (None, None) if bare else (p(q.h0), p(q.reset))
    _lib.check(lib.bg_gru_sequence_forward(q.T, q.N, q.H, p(q.gi), h0, reset, p(q.W), p(q.b), p(o["h_prev"]), p(o["h"]), p(o["gates"]), st), "forward")
    _lib.check(lib.bg_gru_sequence_backward(q.T, q.N, q.H, p(q.dh_ext), p(o["gates"]), p(o["h_prev"]), reset, p(q.W), p(o["dgi"]), p(o["dgh"]), p(o["dh0"]), st),
               "backward")


def _forward_problem(q, o, bare):
    from booster_gym_amd import _lib

    p = _lib.ptr
    return _lib.GruForwardProblem(q.T, q.N, p(q.gi), None if bare else p(q.h0), None if bare else p(q.reset), p(q.W), p(q.b), p(o["h_prev"]), p(o["h"]), p(o["gates"]))


def _backward_problem(q, o, bare):
    from booster_gym_amd import _lib

    p = _lib.ptr
    return _lib.GruBackwardProblem(q.T, q.N, p(q.dh_ext), p(o["gates"]), p(o["h_prev"]), None if bare else p(q.reset), p(q.W), p(o["dgi"]), p(o["dgh"]), p(o["dh0"]))


@pytest.mark.parametrize("bare", [(), (1,), (0,)], ids=["states_and_flags", "second_without", "first_without"])
@pytest.mark.parametrize("Hc,shapes", [(128, ((5, 40), (6, 24))), (256, ((3, 17), (3, 17)))])
def test_group_equals_the_single_launches_bit_for_bit(Hc, shapes, bare, monkeypatch):
    """N = 40, 24 and 17 each leave a partly filled 16-row tile; the two problems have 3 + 2 and 2 + 2 workgroups, dealt alternately.  bare: the problems
    whose h0 and reset are NULL."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    qs = [_Problem(Tp, Np, Hc, 1000 * Hc + 10 * Tp + k) for k, (Tp, Np) in enumerate(shapes)]
    want = [q.outputs() for q in qs]
    for k, (q, o) in enumerate(zip(qs, want)):
        _single(q, o, k in bare)
    got = [q.outputs() for q in qs]
    calls = {n: 0 for n in ("bg_gru_sequence_forward", "bg_gru_sequence_backward")}
    for name in calls:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    fw = (_lib.GruForwardProblem * len(qs))(*[_forward_problem(q, o, k in bare) for k, (q, o) in enumerate(zip(qs, got))])
    _lib.check(lib.bg_gru_sequence_forward_group(fw, len(qs), Hc, _lib.current_stream_ptr()), "bg_gru_sequence_forward_group")
    bw = (_lib.GruBackwardProblem * len(qs))(*[_backward_problem(q, o, k in bare) for k, (q, o) in enumerate(zip(qs, got))])
    _lib.check(lib.bg_gru_sequence_backward_group(bw, len(qs), Hc, _lib.current_stream_ptr()), "bg_gru_sequence_backward_group")
    torch.cuda.synchronize()
    assert calls == {"bg_gru_sequence_forward": 0, "bg_gru_sequence_backward": 0}
    for k, (q, w, g) in enumerate(zip(qs, want, got)):
        for name in w:
            rows = q.N if name == "dh0" else q.T * q.N
            assert bool((g[name][rows:] == SENTINEL).all()) and bool((w[name][rows:] == SENTINEL).all()), f"problem {k}: rows behind {name} were written"
            assert bool(torch.isfinite(w[name][:rows]).all()) and not bool((w[name][:rows] == SENTINEL).all())
            assert torch.equal(g[name][:rows], w[name][:rows]), f"problem {k} (T {q.T}, N {q.N}, H {Hc}): {name} differs from the single launch"
        if k in bare:
            assert bool((w["h_prev"][: q.N] == 0).all())  # no h0: the first step enters with a zero state
        else:
            assert bool((w["h_prev"][: q.T * q.N][q.reset.view(-1).bool()] == 0).all()) and w["dh0"][: q.N].abs().max().item() > 0
    # one problem alone, and three: the same bits again
    for sel in ((1,), (0, 1, 0)):
        again = [qs[k].outputs() for k in sel]
        fw = (_lib.GruForwardProblem * len(sel))(*[_forward_problem(qs[k], o, k in bare) for k, o in zip(sel, again)])
        _lib.check(lib.bg_gru_sequence_forward_group(fw, len(sel), Hc, _lib.current_stream_ptr()), "bg_gru_sequence_forward_group")
        bw = (_lib.GruBackwardProblem * len(sel))(*[_backward_problem(qs[k], o, k in bare) for k, o in zip(sel, again)])
        _lib.check(lib.bg_gru_sequence_backward_group(bw, len(sel), Hc, _lib.current_stream_ptr()), "bg_gru_sequence_backward_group")
        torch.cuda.synchronize()
        for k, o in zip(sel, again):
            assert all(torch.equal(o[name], want[k][name]) for name in o), (sel, k)


def test_group_argument_errors_name_the_entry_point():
    from booster_gym_amd import _lib

    lib, q = _lib.load(), _Problem(2, 20, 128, 7)
    o = q.outputs()
    for name, cls, make, optional in (("bg_gru_sequence_forward_group", _lib.GruForwardProblem, _forward_problem, ("h0", "reset")),
                                      ("bg_gru_sequence_backward_group", _lib.GruBackwardProblem, _backward_problem, ("reset", "dh0"))):
        fn, good = getattr(lib, name), make(q, o, False)

        def changed(**kw):
            c = cls.from_buffer_copy(good)
            for k, v in kw.items():
                setattr(c, k, v)
            return c

        cases = [((cls * 1)(good), 0, 128, -1), (None, 1, 128, -1), ((cls * 5)(*[good] * 5), 5, 128, -1), ((cls * 1)(good), 1, 64, -4), ((cls * 1)(good), 1, 512, -4),
                 ((cls * 2)(good, changed(T=0)), 2, 128, -1), ((cls * 2)(good, changed(N=0)), 2, 128, -1), ((cls * 2)(good, changed(W_hh=good.W_hh + 4)), 2, 128, -1)]
        cases += [((cls * 2)(good, changed(**{f: None})), 2, 128, -1) for f, _ in cls._fields_ if f not in ("T", "N") + optional]
        for arr, n, Hc, rc in cases:
            assert fn(arr, n, Hc, None) == rc and name.encode() in lib.bg_last_error(), (name, n, Hc, lib.bg_last_error())
        assert fn((cls * 2)(good, changed(**{f: None for f in optional})), 2, 128, None) == 0  # the optional pointers may be NULL
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. one update against float64
class _RestatedBoth(_Restated):
    """tests/test_gpu_actor_memory.py's restatement with the critic's cell: est_value on the [T][N] rows walks the T steps from the critic's h0 with
    its flags and keeps the last state; the 2-D call (the observation after the last step) takes one more step from it, behind row T's flags."""

    def __init__(self, net, h0, resets, h0_c, resets_c):
        super().__init__(net, h0, resets)
        self.h0_c, self.resets_c, self.hc_last, self.hc_first, self.hc_after = h0_c.double(), resets_c, None, None, None

    def _keep(self, t):
        return (1 - self.resets_c[t].double()).view(-1, 1)

    def est_value(self, obs, privileged_obs):
        x, Tn = torch.cat((obs, privileged_obs), dim=-1), self.resets_c.shape[0] - 1
        if x.dim() == 2:
            h = self.net.critic_memory(x, self.hc_last * self._keep(Tn))
            if self.hc_after is None:
                self.hc_after = h.detach()
            return self.net.critic(h).squeeze(-1)
        h, vs = self.h0_c, []
        for t in range(Tn):
            h = self.net.critic_memory(x[t], h * self._keep(t))
            vs.append(self.net.critic(h).squeeze(-1))
        self.hc_last = h.detach()
        if self.hc_first is None:  # (the first call: the starting parameters)
            self.hc_first = h.detach()
        return torch.stack(vs)


def _float64_copy(r):
    from booster_gym_amd.utils.model import ActorCritic

    ref = ActorCritic(A, NO, r.env.num_privileged_obs, r.actor_hidden, r.critic_hidden, memory_hidden=H, critic_memory_hidden=H).to(DEV)
    ref.load_state_dict(r.model.state_dict())
    return ref.double()


def _values_pass_only(r):
    """The whole-batch values pass of an update's first mini-epoch and nothing behind it: it leaves the critic's carried state as an update would, and
    Adam's moments and the parameters as they were."""
    u = r._update_begin(r._resolve_plan())
    with torch.no_grad():
        r._whole_batch_values(u, None)
    r.invalidate()
    torch.cuda.synchronize()


@pytest.mark.parametrize("extras", [{}, FEET], ids=["61_columns", "feet_67_columns"])
def test_one_update_matches_float64_autograd_through_time(extras):
    """Mini-epoch 0: the gradients of critic_memory.* and critic.* against float64 autograd of the value loss on the update's own returns, those of
    memory.*, actor.* and logstd as tests/test_gpu_actor_memory.py compares them; the norm the clip sees covers all of them.  The whole update of 2
    mini-epochs at the learning rate 1e-5 against the reference's loop in float64 on the restated model; the critic's last state and the values of
    all (T + 1) N rows against float64.  Figures measured on an MI355X are printed by the run."""
    from oracle.ppo_ref import ppo_update_reference, surrogate_loss

    r = _runner(**{"algorithm.learning_rate": 1.0e-5, **SHORT_EPISODES, **extras})
    mt, cm, alg = r._mem_tr, r._cmem_tr, r.cfg["algorithm"]
    width = NO + r.env.num_privileged_obs
    assert cm is not None and cm.bias_partial and (cm.T, cm.TF, cm.N) == (T, T + 1, N) and cm.kin == r._critic_in.shape[-1] == (128 if extras else 64)
    assert r.model.critic_memory.input_size == width and r.model.critic[0].in_features == H
    r._fused_opt = False  # the tail as separate launches: the optimiser's step is a Python call a spy can stand in front of
    with torch.no_grad():
        r.model.logstd.zero_()  # (the head kernel's KL of a row is then exactly 0 where dmu is: tests/test_gpu_actor_memory.py)
    r.invalidate()
    r.optimizer.max_grad_norm = CLIP
    # two rollouts, and between them the first's values pass (no optimiser step: Adam's moments start with the restatement's): both states are not zero
    r.rollout()
    _values_pass_only(r)
    r.buffer.roll()
    r.rollout()
    torch.cuda.synchronize()
    plan = r._resolve_plan()
    assert not plan.ahead and not plan.one_tail and not plan.one_stream and not plan.chain_values and plan.defer
    assert (plan.critic.fwd, plan.critic.bwd, plan.actor.fwd, plan.actor.bwd) == ("layer",) * 4
    b = r.buffer
    assert mt.h0.abs().max().item() > 1e-3 and cm.h0.abs().max().item() > 1e-3 and torch.equal(cm.h0, cm.next_state)
    assert torch.equal(cm.resets[1:].bool(), b["dones"]) and torch.equal(cm.resets[:T], mt.resets)
    if not bool(b["dones"][: T - 1].any()):  # (no env ended inside the horizon: force one, and the flags the update reads with it)
        b["dones"][1, ::3] = True
    last = b["dones"][T - 1]
    if not bool(last.any()) or bool(last.all()):  # the last step too: row T enters with a zero state for some envs and not for others
        last[:] = False
        last[1::3] = True
    mt.resets[1:].copy_(b["dones"][: T - 1])
    cm.resets[1:].copy_(b["dones"])
    assert bool(cm.resets[1:T].any()) and not bool(cm.resets[1:T].all()) and bool(cm.resets[T].any()) and not bool(cm.resets[T].all())
    obses, priv = b["obses"][:T].double(), b["privileged_obses"][:T].double()
    actions = b["actions"].double()

    # (a) the reference's loop in float64 on the restated model
    ref = _float64_copy(r)
    restated, rec = _RestatedBoth(ref, mt.h0, mt.resets, cm.h0, cm.resets), {}
    stats_ref, lr_ref = ppo_update_reference(restated, torch.optim.Adam(restated.parameters(), lr=1.0e-5), obses, priv, actions, b["rewards"].double().clone(),
                                             b["dones"].clone(), b["time_outs"].clone(), b["obses"][T].double(), b["privileged_obses"][T].double(), mini_epochs=2,
                                             gamma=alg["gamma"], lam=alg["lam"], bound_coef=alg["bound_coef"], entropy_coef=alg["entropy_coef"],
                                             desired_kl=alg["desired_kl"], learning_rate=1.0e-5, max_grad_norm=CLIP, record=rec)
    norm_ref = torch.sqrt(sum((g.double() ** 2).sum() for g in rec["grads"].values())).item()
    share = {n: torch.sqrt(sum((g.double() ** 2).sum() for k, g in rec["grads"].items() if k.startswith(n))).item() for n in ("memory.", "critic_memory.", "critic.")}
    print(f"restatement: gradient norm of the first step {norm_ref:.4f}, shares {share}, max_grad_norm {CLIP}")
    assert norm_ref > CLIP and all(v > 0 for v in share.values())

    # (b) the update, its first mini-epoch read in front of the first optimiser step
    first, norms, clip_sq, step = {}, [], [], r.optimizer.step

    def spy():
        norms.append(r.optimizer.grad.double().norm().item())
        if not first:
            first.update({k: p.grad.clone() for k, p in r.model.named_parameters()}, adv=r._adv.clone(), ret=r._ret.clone(), stats=r._stats.clone(),
                         values=r._values_all.clone(), hc=cm.h.clone(), carried=cm.next_state.clone())
        step()
        clip_sq.append(r.optimizer._gnorm.clone())

    r.optimizer.step = spy
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    acc = r.update()
    summ = r._summarize(acc)
    torch.cuda.synchronize()
    assert len(norms) == 2
    clip_norm = [float(v.sqrt()) for v in clip_sq]
    print(f"update: gradient norms {norms}, the norms the clip used {clip_norm}, restatement's first {norm_ref:.6f}; without critic_memory.* the first "
          f"would be {(norm_ref ** 2 - share['critic_memory.'] ** 2) ** 0.5:.6f}")
    assert abs(norms[0] - norm_ref) <= 1e-3 * norm_ref and abs(clip_norm[0] - norm_ref) <= 1e-3 * norm_ref and min(clip_norm) > CLIP
    # the clip's norm is the whole flat gradient's, and that buffer holds every parameter's gradient, the critic's cell's included
    assert all(abs(c - g) <= 1e-6 * g for c, g in zip(clip_norm, norms)) and sum(p.numel() for p in r.model.parameters()) == sum(r.optimizer.sizes)
    assert all(p.grad.data_ptr() >= r.optimizer.grad.data_ptr() for k, p in r.model.named_parameters() if k.startswith("critic_memory."))
    assert first["stats"][4].item() == 0.0, "the first mini-epoch's KL is not exactly 0: old mu did not come from the update's own launches"

    # (c) float64 on the starting parameters: the critic's states and values, then autograd of the loss on the update's own advantages and returns
    fresh = _float64_copy(r)
    fresh.load_state_dict({k: v.double() for k, v in p_start.items()})
    pol = _RestatedBoth(fresh, mt.h0, mt.resets, cm.h0, cm.resets)
    with torch.no_grad():
        old_logp = pol.act(obses).log_prob(actions).sum(-1)
    values = pol.est_value(obses, priv)
    with torch.no_grad():
        last_values = pol.est_value(b["obses"][T].double(), b["privileged_obses"][T].double())
    hc = first.pop("hc")
    _bound(first["carried"], pol.hc_first, "the critic's state behind step T - 1 (what the next iteration starts from) against float64")
    assert torch.equal(first.pop("carried"), hc[(T - 1) * N : T * N])
    _bound(hc[T * N :], pol.hc_after, "the critic's last state (row T) against float64")
    _bound(first.pop("values"), torch.cat((values.detach().reshape(-1), last_values)), "the values of all (T + 1) N rows against float64")
    assert torch.equal(cm.next_state, hc[(T - 1) * N : T * N]), "a later mini-epoch changed the carried state"
    adv = first.pop("adv").double()
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    dist = pol.act(obses)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    loss = (torch.nn.functional.mse_loss(values, first.pop("ret").double()) + surrogate_loss(old_logp, dist.log_prob(actions).sum(-1), adv)
            + alg["bound_coef"] * bound_loss + alg["entropy_coef"] * dist.entropy().sum(-1).mean())
    loss.backward()
    first.pop("stats")
    for k, q in fresh.named_parameters():
        _grad_bound(first.pop(k), q.grad, f"grad {k}")
    assert not first  # every parameter: 4 + 4 of the cells, 8 + 8 of the trunks, logstd

    # (d) after 2 mini-epochs: parameters, losses, learning rate against the reference's loop
    for (k, p), (k2, q) in zip(r.model.named_parameters(), ref.named_parameters()):
        assert k == k2 and not torch.equal(p, p_start[k]), k
        print(k, "max |p - restatement|", (p.double() - q).abs().max().item(), "moved", (q - p_start[k].double()).abs().max().item())
        assert torch.allclose(p.double(), q, rtol=1e-3, atol=2e-6), (k, (p.double() - q).abs().max().item())
        _assert_same_adam_steps(k, p.double(), q, p_start[k].double())
    for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean"):
        print(k, summ[k], stats_ref[k])
        assert abs(summ[k] - stats_ref[k]) <= 2e-4 * max(1.0, abs(stats_ref[k])), (k, summ[k], stats_ref[k])
    assert abs(summ["lr"] - lr_ref) < 1e-9


# ------------------------------------------------------------------ 3. the rules of the critic's carried state
def _walk_f64(cell, x, h0, resets):
    """The float64 walk of a cell over x [steps][N][in] from h0 with the flags: the state behind every step."""
    cell, h, out = cell.double(), h0.double(), []
    with torch.no_grad():
        for t in range(x.shape[0]):
            h = cell(x[t].double(), h * (1 - resets[t].double()).view(-1, 1))
            out.append(h)
    return torch.stack(out)


def test_state_rules_and_reproducibility():
    import copy

    shas = []
    for run in range(2):
        r = _runner(**SHORT_EPISODES)
        cm = r._cmem_tr
        assert torch.all(cm.next_state == 0) and torch.all(cm.h0 == 0) and cm.next_state.shape == (N, H)
        any_reset = False
        for it in range(3):
            carried, last = cm.next_state.clone(), r._last_dones.clone()
            r.rollout()
            before = copy.deepcopy(r.model.critic_memory)  # the parameters the rollout ran on
            dones = r.buffer["dones"].clone()
            rows = torch.cat((r.buffer["obses"], r.buffer["privileged_obses"]), dim=-1).clone()
            assert torch.equal(cm.h0, carried) and torch.equal(cm.resets[0], last) and torch.equal(cm.resets[1:].bool(), dones), it
            seen, carry = [], cm.carry_state

            def spy():
                carry()
                seen.append(cm.next_state.clone())

            cm.carry_state = spy
            r.update()
            del cm.carry_state
            r.buffer.roll()
            torch.cuda.synchronize()
            # once per update, behind mini-epoch 0's pass; mini-epoch 1 runs on other parameters and leaves it alone
            assert len(seen) == 1 and torch.equal(cm.next_state, seen[0]) and not torch.equal(cm.next_state, cm.h[(T - 1) * N : T * N]), it
            walk = _walk_f64(before, rows, carried, cm.resets)
            _bound(cm.next_state, walk[T - 1], f"iteration {it}: the carried state against a float64 walk on the parameters from before the update")
            assert torch.all(cm.h_prev[cm.resets.bool().view(-1)] == 0.0)  # an env that reset enters its next step with a zero state
            any_reset = any_reset or bool(cm.resets[1:].any())
            assert "critic_memory_state" not in r.checkpoint_dict() and not any("state" in k for k in r.checkpoint_dict()["model"] if k.startswith("critic_memory"))
        assert any_reset, "no reset fell inside a horizon"
        r.begin_training(recorder=_Rec())
        assert torch.all(cm.next_state == 0)  # zero again at begin_training
        shas.append(_digest(r))
        del r
    assert shas[0] == shas[1]


# ------------------------------------------------------------------ 4. env mini-batches
def test_first_step_of_an_env_mini_batch_matches_float64_autograd():
    """N = 64, T = 8, K = 2: b = 256 rows.  The gradients of both cells and both trunks in front of the first optimiser step against float64 autograd on
    the envs Runner.env_permutation names, from their gathered states and flags, on the update's own advantages and returns."""
    from oracle.ppo_ref import surrogate_loss

    Nn, Tt, K = 64, 8, 2
    n = Nn // K
    r = _runner(**{"env.num_envs": Nn, "runner.horizon_length": Tt, KMB: K, "algorithm.learning_rate": 1.0e-5, **SHORT_EPISODES})
    mt, cm, alg = r._mem_tr, r._cmem_tr, r.cfg["algorithm"]
    assert r._mb_rows == Tt * n == 256 and (r._cmem_mb.T, r._cmem_mb.TF, r._cmem_mb.N) == (Tt, Tt, n) and r._gru_group == 1
    r._fused_opt = False
    with torch.no_grad():
        r.model.logstd.zero_()
    r.invalidate()
    r.rollout()
    _values_pass_only(r)
    r.buffer.roll()
    r.rollout()
    torch.cuda.synchronize()
    assert r._resolve_plan().gru_group == 1 and r._mb_plan.gru_group == 1 and not r._mb_plan.one_stream
    b = r.buffer
    assert mt.h0.abs().max().item() > 1e-3 and cm.h0.abs().max().item() > 1e-3 and bool(mt.resets[1:].any()) and not bool(mt.resets[1:].all())
    sigma = r.env_permutation(r._mb_updates, 0)
    assert _is_permutation(sigma, Nn)
    first, step = {}, r.optimizer.step

    def spy():
        if not first:
            first.update({k: p.grad.clone() for k, p in r.model.named_parameters()}, adv=r._adv.clone(), ret=r._ret.clone(), h0=r._mb.h0.clone(),
                         h0_c=r._mb.h0_c.clone(), resets=r._mb.resets.clone())
        step()

    r.optimizer.step = spy
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    r.update()
    torch.cuda.synchronize()
    assert r.optimizer.step_count == 2 * K
    # the gathered states and flags of the first mini-epoch are the whole batch's by its permutation: ten streams, the critic's state the tenth
    assert torch.equal(first["h0"], mt.h0[sigma.long()]) and torch.equal(first["h0_c"], cm.h0[sigma.long()])
    assert torch.equal(first["resets"].view(K, Tt, n), _by_envs(mt.resets, sigma, K)) and torch.equal(cm.resets[:Tt], mt.resets)
    envs = sigma[:n].long()
    fresh = _float64_copy(r)
    fresh.load_state_dict({k: v.double() for k, v in p_start.items()})
    pol = _RestatedBoth(fresh, first["h0"][:n], first["resets"].view(K, Tt, n)[0], first["h0_c"][:n],
                        torch.cat((first["resets"].view(K, Tt, n)[0], torch.zeros(1, n, dtype=torch.uint8, device=DEV))))
    obses, priv, actions = b["obses"][:Tt, envs].double(), b["privileged_obses"][:Tt, envs].double(), b["actions"][:, envs].double()
    with torch.no_grad():
        old_logp = pol.act(obses).log_prob(actions).sum(-1)
    adv = first["adv"].double()
    adv = ((adv - adv.mean()) / (adv.std() + 1e-8))[:, envs]  # the whole batch's moments
    dist, values = pol.act(obses), pol.est_value(obses, priv)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    loss = (torch.nn.functional.mse_loss(values, first["ret"].double()[:, envs]) + surrogate_loss(old_logp, dist.log_prob(actions).sum(-1), adv)
            + alg["bound_coef"] * bound_loss + alg["entropy_coef"] * dist.entropy().sum(-1).mean())
    loss.backward()
    for k, q in fresh.named_parameters():
        _grad_bound(first[k], q.grad, f"grad {k}")


def _child(group):
    env = dict(os.environ, BG_GRU_GROUP=group, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rnn_critic_child.py")], env=env, check=True, timeout=300, capture_output=True, text=True).stdout
    lines = {l.split()[0]: l.split()[1:] for l in out.splitlines() if l.startswith(("counts", "sha256"))}
    return [int(c) for c in lines["counts"]], lines["sha256"][0]


def test_group_on_and_off_leave_the_same_bits():
    """Two iterations at N = 64, T = 8, K = 2, each side in a fresh process.  Per update: old mu's pass (the actor's cell alone), 2 whole-batch values
    passes (the critic's alone), then 2 x 2 steps with both cells each way: as one grouped launch or as two single ones.  BG_GRU_GROUP = 1, the
    default, groups the forward recurrences, 2 the backward ones too, 0 none."""
    on, both, off = _child("1"), _child("2"), _child("0")
    assert on[0] == [2 * 3, 2 * 8, 2 * 4, 0] and both[0] == [2 * 3, 0, 2 * 4, 2 * 4] and off[0] == [2 * (3 + 8), 2 * 8, 0, 0], (on[0], both[0], off[0])
    assert on[1] == off[1] == both[1], "BG_GRU_GROUP=1, =2 and =0 leave different parameters or moments"


# ------------------------------------------------------------------ 5. the key off
def test_key_off_runs_todays_calls_alone(monkeypatch):
    import importlib.util

    from booster_gym_amd import _lib

    lib = _lib.load()

    def forbidden(*a):
        raise AssertionError("a grouped recurrence ran outside a one-stream step with both cells")

    for name in GROUP_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, forbidden)
    today = ["logstd"] + [f"{n}.{i}.{w}" for n in ("critic", "actor") for i in (0, 2, 4, 6) for w in ("weight", "bias")]
    for over, names in (({RNN: 0, KEY: False}, today), ({KEY: None}, today + [f"memory.{w}" for w in CELL]), ({KEY: False, KMB: 2, "env.num_envs": 64, "runner.horizon_length": 8}, None),
                        ({}, today + [f"memory.{w}" for w in CELL] + [f"critic_memory.{w}" for w in CELL])):  # (the last: the key on at K = 1)
        cfg = _cfg(**over)
        if not over.get(KEY, True):
            del cfg["algorithm"]["rnn_critic"]  # absent, as in the shipped yaml
        r = _runner(cfg=cfg)
        if over:
            assert r._cmem_tr is None and not hasattr(r.model, "critic_memory") and r.model.critic[0].in_features == 61 and not r._resolve_plan().gru_group
        assert names is None or [k for k, _ in r.model.named_parameters()] == names
        for it in range(2):
            r.train_iteration(it)
        r._flush_log()
        torch.cuda.synchronize()
        assert torch.isfinite(r.optimizer.flat).all()
        del r
    # the launch sequence of an rnn_hidden_size: 128 run without the key is the committed record's, call by call
    spec = importlib.util.spec_from_file_location("make_launch_sequences", os.path.join(ROOT, "tests", "golden", "make_launch_sequences.py"))
    recipe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recipe)
    import json

    with open(os.path.join(ROOT, "tests", "golden", "launch_sequences.json")) as f:
        want = json.load(f)["ppo_rnn_hidden_size_128"]
    got, _ = recipe.record("ppo_rnn_hidden_size_128", None)
    assert got == want


# ------------------------------------------------------------------ 6. life cycle
def test_training_saves_resumes_evaluates_and_exports(tmp_path):
    from booster_gym_amd.utils.evaluate import Evaluator
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import Runner, checkpoint_memory_overrides

    big = {"env.num_envs": 128}
    r = _runner(**big)
    names = [k for k, _ in r.model.named_parameters()]
    assert names[-8:] == [f"{c}.{w}" for c in ("memory", "critic_memory") for w in CELL]
    assert [id(p) for p in r.optimizer.params] == [id(p) for p in r.model.parameters()]
    start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    for it in range(2):
        s = r.recorder.stats[it]
        assert all(torch.isfinite(torch.tensor(float(v))) for v in s.values()) and not any("memory" in k or "rnn" in k for k in s)  # no log name is added
    assert torch.isfinite(r.optimizer.flat).all() and all(not torch.equal(p, start[k]) for k, p in r.model.named_parameters())
    ck = r.checkpoint_dict()
    assert {f"critic_memory.{w}" for w in CELL} <= set(ck["model"]) and len(ck["optimizer"]["state"]) == len(names)
    assert sum(v["exp_avg"].numel() for v in ck["optimizer"]["state"].values()) == sum(r.optimizer.sizes)
    assert checkpoint_memory_overrides(ck) == {RNN: H, KEY: True} and not any(k for k in ck if "state" in k and "critic" in k)
    path = str(tmp_path / "both_cells.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r
    # resume: the parameters and Adam's moments are the checkpoint's, the critic's state is zero again, and training continues
    r = _runner(**big, **{"basic.checkpoint": path})
    assert all(torch.equal(v, sd[k]) for k, v in r.model.state_dict().items()) and torch.all(r._cmem_tr.next_state == 0)
    assert r.optimizer.step_count == 4 and r.optimizer.exp_avg.abs().max().item() > 0
    r.train_iteration(0)
    r._flush_log()
    torch.cuda.synchronize()
    assert torch.isfinite(r.optimizer.flat).all() and not torch.equal(r.model.critic_memory.weight_hh, sd["critic_memory.weight_hh"])
    del r
    # a checkpoint and a config that disagree about the key, either way
    with pytest.raises(ValueError, match=r"algorithm\.rnn_critic"):
        Runner(cfg=_cfg(**big, **{KEY: False, "basic.checkpoint": path}))
    plain_model = ActorCritic(A, NO, 14, memory_hidden=H)
    plain_model.load_state_dict({k: v.cpu() for k, v in sd.items() if not k.startswith(("critic_memory.", "critic."))}, strict=False)
    plain = str(tmp_path / "actor_cell_only.pth")
    torch.save({"model": plain_model.state_dict(), "curriculum": ck["curriculum"]}, plain)
    with pytest.raises(ValueError, match=r"algorithm\.rnn_critic"):
        Runner(cfg=_cfg(**big, **{"basic.checkpoint": plain}))
    # evaluate.py's way in: both keys from the checkpoint, reported
    bare = _cfg(**big)
    del bare["algorithm"]["rnn_critic"], bare["algorithm"]["rnn_hidden_size"]
    ev = Evaluator(checkpoint=path, cfg=bare)
    assert ev.applied[KEY] is True and ev.applied[RNN] == H and ev.model.critic_memory_hidden == H
    rep = ev.run(steps=8)
    assert rep["steps"] == 8 and rep["overrides"][KEY] is True
    del ev
    # export_model.py: the module is the actor's, and equals the one exported from the same actor without the critic's cell
    envv = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    mods = []
    for k, p in enumerate((path, plain)):
        cwd = tmp_path / f"export{k}"
        cwd.mkdir()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={p}"], cwd=str(cwd), env=envv, check=True, timeout=300,
                             capture_output=True, text=True)
        assert "STATEFUL" in out.stdout
        mods.append(torch.jit.load(str(cwd / "deploy" / "models" / "T1.pt"), map_location="cpu"))
    x = torch.randn(3, 7, NO, generator=torch.Generator().manual_seed(5))
    for t in range(3):
        ya, yb = mods[0](x[t]), mods[1](x[t])
        assert tuple(ya.shape) == (7, A) and torch.equal(ya, yb) and ya.abs().max().item() > 0
    assert not any("critic" in k for k in mods[0].state_dict())
