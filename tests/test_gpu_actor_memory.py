"""algorithm.rnn_hidden_size on the GPU: PPO on a recurrent (GRU) actor.  The one new launch, bg_gru_bias_partial with its finish, against float64
column sums; one update against float64 autograd through the iteration's steps (the cell from the stored state with the resets, the trunk, the PPO
loss as oracle/ppo_ref.py states it) and the reference's own loop on that restated model; the rules of the carried state; training, saving,
resuming, evaluating, playing and exporting; fine-tuning a distilled recurrent student; one composition; and the key off against today's calls.

Shapes and bounds are tests/test_gpu_distill_memory.py's: N = 40 envs (two 16-row tiles of the recurrence and a tail of 8), T = 5 (B = 200: one
128-row block and a ragged one), plane terrain; forward quantities 2e-5 max(1, |ref|max) (_bound), gradients 1e-4 of the tensor's largest entry
(_grad_bound), parameters after an update rtol 1e-3 / atol 2e-6 at the learning rate 1e-5 and test_gpu_ppo's _assert_same_adam_steps, logged losses
test_full_update_matches_reference_loop's 2e-4 max(1, |ref|)."""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_distill import GRID_5x3, _Rec
from test_gpu_distill import _cfg as _distill_cfg
from test_gpu_distill_memory import MEM, _bound, _distiller, _grad_bound, teacher_ck  # noqa: F401  (teacher_ck: the module's fixture)
from test_gpu_ppo import _assert_same_adam_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, N, T, H = 12, 40, 5, 128
KEY = "algorithm.rnn_hidden_size"
GRU_ENTRY_POINTS = ("bg_actor_sample_gru", "bg_distill_act_gru", "bg_gru_sequence_forward", "bg_gru_sequence_backward", "bg_gru_bias_partial")
# an episode of 7 control steps of 0.02 s: every env times out (and resets) on its 8th step, inside the second horizon of 5
SHORT_EPISODES = {"rewards.episode_length_s": 0.13}
CLIP = 0.25  # max_grad_norm of the gradient test, on both of its sides


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "terrain.type": "plane", "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "runner.mini_epochs": 2,
          KEY: H}
    ov.update(over)
    return load_cfg("T1", ov)


def _runner(cfg=None, **over):
    from booster_gym_amd.utils.runner import Runner

    r = Runner(cfg=cfg if cfg is not None else _cfg(**over))
    r.begin_training(recorder=_Rec())
    return r


def _sha(r):
    h = hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [r.model._memory_state]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ 1. bg_gru_bias_partial + its finish
def _bias_finish(records, nb, Hc, out_i, out_h):
    from booster_gym_amd import _lib

    fin = _lib.ReduceProblem()
    fin.partial, fin.groups, fin.record, fin.n_out = records.data_ptr(), nb, 6 * Hc, 6 * Hc
    fin.out[0], fin.out[1], fin.n[0], fin.n[1] = out_i.data_ptr(), out_h.data_ptr(), 3 * Hc, 3 * Hc
    return fin


@pytest.mark.parametrize("Hc", [128, 256])
@pytest.mark.parametrize("B", [129, 200, 384])
def test_gru_bias_partial_and_its_finish(B, Hc):
    """B = 129: a block of one row; 200: a ragged block; 384: whole blocks only.  Rows behind B hold NaN: a row read past B poisons a sum."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import reduce_group

    g = torch.Generator(device="cpu").manual_seed(B + Hc)
    C, nb, p = 3 * Hc, (B + 127) // 128, _lib.ptr
    dgi, dgh = (torch.full((B + 130, C), float("nan"), device=DEV) for _ in range(2))
    dgi[:B], dgh[:B] = torch.randn(B, C, generator=g).to(DEV), (torch.randn(B, C, generator=g) * 3.0).to(DEV)

    def run():
        records = torch.full((nb + 2, 6 * Hc), 7.0, device=DEV)
        out_i, out_h = torch.full((C + 8,), 7.0, device=DEV), torch.full((C + 8,), 7.0, device=DEV)
        _lib.check(_lib.load().bg_gru_bias_partial(B, Hc, p(dgi), p(dgh), p(records), _lib.current_stream_ptr()), "bg_gru_bias_partial")
        reduce_group([_bias_finish(records, nb, Hc, out_i, out_h)])
        torch.cuda.synchronize()
        assert torch.all(records[nb:] == 7.0), "records past the last block were written"
        assert torch.all(out_i[C:] == 7.0) and torch.all(out_h[C:] == 7.0)
        return records[:nb], out_i[:C], out_h[:C]

    rec, out_i, out_h = run()
    assert torch.isfinite(rec).all() and torch.isfinite(out_i).all() and torch.isfinite(out_h).all(), "a row at or beyond B was read"
    for k in range(nb):  # record k = the column sums of rows [128 k, min(128 k + 128, B)): dgi's | dgh's
        rows = slice(128 * k, min(128 * k + 128, B))
        _grad_bound(rec[k], torch.cat((dgi[rows].double().sum(0), dgh[rows].double().sum(0))), f"B {B} H {Hc} record {k}")
    _grad_bound(out_i, dgi[:B].double().sum(0), f"B {B} H {Hc} bias_ih gradient")
    _grad_bound(out_h, dgh[:B].double().sum(0), f"B {B} H {Hc} bias_hh gradient")
    for x, y in zip((rec, out_i, out_h), run()):
        assert torch.equal(x, y), "two calls differ"


def test_gru_bias_partial_argument_errors_name_the_entry_point():
    from booster_gym_amd import _lib

    lib, o = _lib.load(), torch.zeros(4096, device=DEV)
    p, name = o.data_ptr(), b"bg_gru_bias_partial"
    for args, rc in (((0, 128, p, p, p), -1), ((4, 64, p, p, p), -4), ((4, 512, p, p, p), -4), ((4, 128, None, p, p), -1), ((4, 128, p, None, p), -1),
                     ((4, 128, p, p, None), -1), ((4, 128, p + 4, p, p), -1), ((4, 128, p, p + 8, p), -1), ((4, 128, p, p, p + 4), -1)):
        assert lib.bg_gru_bias_partial(*args, None) == rc and name in lib.bg_last_error(), (args, lib.bg_last_error())


# ------------------------------------------------------------------ 2. one update against float64 autograd through time
class _Restated:
    """What oracle/ppo_ref.ppo_update_reference asks of a model, on a float64 ActorCritic with memory: the cell over the T steps from h0 (a zero
    state behind a reset), the trunk on every state."""

    def __init__(self, net, h0, resets):
        self.net, self.h0, self.resets, self.h_first = net, h0.double(), resets, None

    def parameters(self):
        return list(self.net.parameters())

    def named_parameters(self):
        return self.net.named_parameters()

    def act(self, obses):
        h, mus = self.h0, []
        for t in range(obses.shape[0]):
            h = self.net.memory(obses[t], h * (1 - self.resets[t].double()).view(-1, 1))
            mus.append(self.net.actor(h))
        if self.h_first is None:  # (the first call: the starting parameters)
            self.h_first = h.detach()
        mean = torch.stack(mus)
        return torch.distributions.Normal(mean, torch.exp(self.net.logstd).expand_as(mean))

    def est_value(self, obs, privileged_obs):
        return self.net.critic(torch.cat((obs, privileged_obs), dim=-1)).squeeze(-1)


def _float64_copy(r):
    from booster_gym_amd.utils.model import ActorCritic

    ref = ActorCritic(A, 47, r.env.num_privileged_obs, r.actor_hidden, r.critic_hidden, memory_hidden=H).to(DEV)
    ref.load_state_dict(r.model.state_dict())
    return ref.double()


def test_one_update_matches_float64_autograd_through_time():
    """First mini-epoch: the gradients of memory.*, actor.* and logstd against float64 autograd of the actor's loss on the update's own advantages.
    The whole update of 2 mini-epochs at the learning rate 1e-5: parameters, logged losses and the learning rate against the reference's loop
    (oracle/ppo_ref.py, unedited) run in float64 on the restated model.  Figures measured on an MI355X are printed by the run."""
    from oracle.ppo_ref import ppo_update_reference, surrogate_loss

    r = _runner(**{"algorithm.learning_rate": 1.0e-5, **SHORT_EPISODES})
    mt, alg = r._mem_tr, r.cfg["algorithm"]
    assert mt is not None and mt.bias_partial and r.model.memory_hidden == H and r.model.actor[0].in_features == H
    r._fused_opt = False  # the tail as separate launches: the optimiser's step is a Python call a spy can stand in front of
    # log-std 0: the head kernel's KL of a row, sum_a logstd - old_logstd + 0.5 (old_sigma^2 + dmu^2) / sigma^2 - 0.5 in fp32, is then exactly 0 where
    # dmu is (sigma^2 = 1 / sigma^2 = 1; at the initial -2 the rounded reciprocal leaves -1.2e-8 a row whatever mu is), so "exactly 0" below says dmu = 0
    with torch.no_grad():
        r.model.logstd.zero_()
    r.invalidate()
    # ... and, the actor's gradients being 1 / sigma^2 smaller for it, a clip at 0.25 on both sides, so that the steps are clipped (asserted below)
    r.optimizer.max_grad_norm = CLIP
    r.rollout()  # a rollout first: the one below starts from a state that is not zero (no update: Adam's moments start with the restatement's)
    r.buffer.roll()
    r.rollout()
    torch.cuda.synchronize()
    plan = r._resolve_plan()
    assert not plan.ahead and not plan.one_tail and (plan.actor.fwd, plan.actor.bwd) == ("layer", "layer") and plan.defer
    b = r.buffer
    assert mt.h0.abs().max().item() > 1e-3 and torch.equal(mt.resets[1:].bool(), b["dones"][: T - 1])
    forced = not bool(b["dones"][: T - 1].any())
    if forced:  # (no env ended inside the horizon: force one, and the flags the update reads with it; the rollout's own state then is another's)
        b["dones"][1, ::3] = True
        mt.resets[2].copy_(b["dones"][1])
    assert bool(mt.resets[1:].any()) and not bool(mt.resets[1:].all())
    rollout_state = r.model._memory_state.clone()
    obses, priv = b["obses"][:T].double(), b["privileged_obses"][:T].double()
    actions = b["actions"].double()

    # (a) the reference's loop in float64 on the restated model
    ref = _float64_copy(r)
    restated, rec = _Restated(ref, mt.h0, mt.resets), {}
    stats_ref, lr_ref = ppo_update_reference(restated, torch.optim.Adam(restated.parameters(), lr=1.0e-5), obses, priv, actions, b["rewards"].double().clone(),
                                             b["dones"].clone(), b["time_outs"].clone(), b["obses"][T].double(), b["privileged_obses"][T].double(), mini_epochs=2,
                                             gamma=alg["gamma"], lam=alg["lam"], bound_coef=alg["bound_coef"], entropy_coef=alg["entropy_coef"],
                                             desired_kl=alg["desired_kl"], learning_rate=1.0e-5, max_grad_norm=CLIP, record=rec)
    norm_ref = torch.sqrt(sum((g.double() ** 2).sum() for g in rec["grads"].values())).item()
    cell_share = torch.sqrt(sum((g.double() ** 2).sum() for k, g in rec["grads"].items() if k.startswith("memory."))).item()
    print(f"restatement: gradient norm of the first step {norm_ref:.4f} (memory.* alone {cell_share:.4f}), max_grad_norm {r.optimizer.max_grad_norm}")
    assert norm_ref > r.optimizer.max_grad_norm and cell_share > 0  # the first step is clipped: a norm without the cell's gradients scales it otherwise

    # (b) the update, its first mini-epoch read in front of the first optimiser step
    first, norms, clip_sq, step = {}, [], [], r.optimizer.step

    def spy():
        norms.append(r.optimizer.grad.double().norm().item())
        if not first:
            first.update({k: p.grad.clone() for k, p in r.model.named_parameters()}, h=mt.h[-N:].clone(), adv=r._adv.clone(), stats=r._stats.clone())
        step()
        clip_sq.append(r.optimizer._gnorm.clone())  # bg_adam_step's own squared norm: what its clip divided by

    r.optimizer.step = spy
    p_start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    acc = r.update()
    summ = r._summarize(acc)
    torch.cuda.synchronize()
    assert len(norms) == 2
    print(f"update: gradient norms {norms}, restatement's first {norm_ref:.6f}")
    clip_norm = [float(v.sqrt()) for v in clip_sq]
    print(f"update: the norms the clip used {clip_norm}; without memory.* the first would be {(norm_ref ** 2 - cell_share ** 2) ** 0.5:.6f}")
    # the clip's norm is over every gradient, the cell's four included (leaving them out moves it by 2 %: 0.5060 against 0.5166)
    assert abs(norms[0] - norm_ref) <= 1e-3 * norm_ref and abs(clip_norm[0] - norm_ref) <= 1e-3 * norm_ref and min(clip_norm) > CLIP
    assert first["stats"][4].item() == 0.0, "the first mini-epoch's KL is not exactly 0: old mu did not come from the update's own launches"
    _bound(first.pop("h"), restated.h_first, "the update's last state against float64")
    if not forced:  # (the rollout and the update walk the same steps from the same h0)
        _bound(rollout_state, restated.h_first, "the rollout's state against float64")

    # (c) float64 autograd of the actor's loss on the update's own advantages (oracle/ppo_ref.py's statement of it), from the starting parameters
    fresh = _float64_copy(r)
    fresh.load_state_dict({k: v.double() for k, v in p_start.items()})
    pol = _Restated(fresh, mt.h0, mt.resets)
    with torch.no_grad():
        old_logp = pol.act(obses).log_prob(actions).sum(-1)
    adv = first.pop("adv").double()
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    dist = pol.act(obses)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    loss = surrogate_loss(old_logp, dist.log_prob(actions).sum(-1), adv) + alg["bound_coef"] * bound_loss + alg["entropy_coef"] * dist.entropy().sum(-1).mean()
    loss.backward()
    first.pop("stats")
    compared = 0
    for k, q in fresh.named_parameters():
        if k.startswith(("memory.", "actor.")) or k == "logstd":
            _grad_bound(first[k], q.grad, f"grad {k}")
            compared += 1
    assert compared == 4 + 8 + 1

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


# ------------------------------------------------------------------ 3. the rules of the carried state
def test_state_rules_and_reproducibility():
    """One mini-epoch per update: the update's one forward pass then runs on the parameters the rollout acted with."""
    shas = []
    for run in range(2):
        r = _runner(**{"runner.mini_epochs": 1, **SHORT_EPISODES})
        mt, model, resets_seen = r._mem_tr, r.model, []
        assert model._memory_state is not None and torch.all(model._memory_state == 0) and torch.all(r._last_dones == 0)
        sample = model.sample_actions

        def spy(*a, reset=None, **kw):
            resets_seen.append(reset.clone().view(-1).to(torch.uint8))
            return sample(*a, reset=reset, **kw)

        model.sample_actions = spy
        any_reset = False
        for it in range(3):
            state, last = model._memory_state.clone(), r._last_dones.clone()
            del resets_seen[:]
            r.rollout()
            after = model._memory_state.clone()
            dones = r.buffer["dones"].clone()
            r.update()
            r.buffer.roll()
            torch.cuda.synchronize()
            # h0 of this iteration = the state the one before ended in (zero at first), bit for bit; the reset flags are the done flags one step on
            assert torch.equal(mt.h0, state) and torch.equal(mt.resets[0], last) and torch.equal(mt.resets[1:].bool(), dones[: T - 1]), it
            assert len(resets_seen) == T and torch.equal(torch.stack(resets_seen), mt.resets), it
            assert torch.equal(r._last_dones.bool(), dones[T - 1]) and not torch.equal(after, state)
            # an env that reset enters its next step with a zero state, in the update's recurrence and (the states agree) in the rollout's
            on = mt.resets.bool().view(-1)
            assert torch.all(mt.h_prev[on] == 0.0)
            _bound(after, mt.h[-N:].double(), f"iteration {it}: the rollout's state against the update's last h")
            any_reset = any_reset or bool(mt.resets[1:].any())
        assert any_reset, "no reset fell inside a horizon"
        shas.append(_sha(r))
        del r
    assert shas[0] == shas[1]


# ------------------------------------------------------------------ 4. training runs, saves, resumes, evaluates, plays and exports
def test_training_runs_saves_resumes_evaluates_and_exports(tmp_path):
    """Fails on the parent commit, where Runner(test=False) refuses a model with memory."""
    from booster_gym_amd.utils.distill import checkpoint_student_overrides
    from booster_gym_amd.utils.evaluate import Evaluator
    from booster_gym_amd.utils.runner import Runner, checkpoint_memory_overrides

    r = _runner()
    names = [k for k, _ in r.model.named_parameters()]
    assert names[-4:] == ["memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"]
    assert [id(p) for p in r.optimizer.params] == [id(p) for p in r.model.parameters()]
    start = {k: p.detach().clone() for k, p in r.model.named_parameters()}
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    for it in range(2):
        s = r.recorder.stats[it]
        assert all(torch.isfinite(torch.tensor(float(s[k]))) for k in ("value_loss", "actor_loss", "bound_loss", "entropy", "kl_mean", "lr")), s
        assert not any("memory" in k or "rnn" in k for k in s)  # no log name is added
    assert torch.isfinite(r.optimizer.flat).all()
    for k, p in r.model.named_parameters():
        assert not torch.equal(p, start[k]), f"{k} did not move"
    ck = r.checkpoint_dict()
    assert {"memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"} <= set(ck["model"]) and "distillation" not in ck
    assert len(ck["optimizer"]["state"]) == len(names) and sum(v["exp_avg"].numel() for v in ck["optimizer"]["state"].values()) == sum(r.optimizer.sizes)
    assert checkpoint_student_overrides(ck) is None and checkpoint_memory_overrides(ck) == {KEY: H}
    path = str(tmp_path / "recurrent.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in r.model.state_dict().items()}
    del r
    # resume: the parameters and Adam's moments are the checkpoint's, the state is zero again, and training continues
    r = _runner(**{"basic.checkpoint": path})
    assert all(torch.equal(v, sd[k]) for k, v in r.model.state_dict().items()) and torch.all(r.model._memory_state == 0)
    assert r.optimizer.step_count == 4 and r.optimizer.exp_avg.abs().max().item() > 0
    r.train_iteration(0)
    r._flush_log()
    torch.cuda.synchronize()
    assert torch.isfinite(r.optimizer.flat).all() and not torch.equal(r.model.memory.weight_hh, sd["memory.weight_hh"])
    del r
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory"):  # a config without the key against this checkpoint
        Runner(cfg=_cfg(**{KEY: 0, "basic.checkpoint": path}))
    # evaluate.py's way in: the width from the checkpoint, reported
    plain = _cfg(**{KEY: 0})
    del plain["algorithm"]["rnn_hidden_size"]
    ev = Evaluator(checkpoint=path, cfg=plain)
    assert ev.applied[KEY] == H and ev.model.memory_hidden == H
    rep = ev.run(steps=8)
    assert rep["steps"] == 8 and rep["overrides"][KEY] == H and ev.model._memory_state.abs().max().item() > 0
    del ev
    # play under the yaml the run trained with, then the exported stateful module on the rows play saw
    p = Runner(test=True, cfg=_cfg(**{"basic.checkpoint": path}))
    obs_seen, act_seen, done_seen, env = [], [], [], p.env
    reset, step = env.reset, env.step

    def spy_reset():
        out = reset()
        obs_seen.append(out[0].clone())
        return out

    def spy_step(act):
        act_seen.append(act.clone())
        out = step(act)
        obs_seen.append(out[0].clone())
        done_seen.append(out[2].clone())
        return out

    env.reset, env.step = spy_reset, spy_step
    assert p.play(max_steps=4) == 4 and len(act_seen) == 4
    del p
    envv = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={path}"], cwd=str(tmp_path), env=envv, check=True,
                         timeout=300, capture_output=True, text=True)
    assert "STATEFUL" in out.stdout
    mod = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    for t in range(4):
        y = mod(obs_seen[t].cpu())
        err = (y - act_seen[t].cpu()).abs().max().item()
        print(f"step {t}: TorchScript against play {err:.3e}")
        assert tuple(y.shape) == (N, A) and err <= 1e-5
        if bool(done_seen[t].any()):
            h = mod.h.clone()
            h[done_seen[t].cpu().bool()] = 0.0
            mod.h = h


# ------------------------------------------------------------------ 5. fine-tuning a distilled recurrent student
def test_a_recurrent_student_fine_tunes_under_ppo(teacher_ck, tmp_path):  # noqa: F811
    from booster_gym_amd.utils.distill import student_cfg_overrides
    from booster_gym_amd.utils.runner import Runner

    d = _distiller(teacher_ck)
    d.train_iteration(0)
    path = str(tmp_path / "student.pth")
    torch.save(d.checkpoint_dict(), path)
    over, sd = student_cfg_overrides(d.cfg), {k: v.clone() for k, v in d.student.state_dict().items()}
    del d
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory.*out of scope.*algorithm\.rnn_hidden_size"):  # the re-entry overrides alone do not train
        Runner(cfg=_distill_cfg(None, 1, **over, **{"basic.checkpoint": path}))
    r = _runner(cfg=_distill_cfg(None, 1, **over, **{KEY: MEM, "basic.checkpoint": path, "runner.mini_epochs": 2}))
    assert all(torch.equal(v, sd[k]) for k, v in r.model.state_dict().items())
    assert r.optimizer.step_count == 0 and float(r.optimizer.exp_avg.abs().sum()) == 0.0  # fresh Adam moments
    r.train_iteration(0)
    r._flush_log()
    torch.cuda.synchronize()
    assert torch.isfinite(r.optimizer.flat).all() and all(torch.isfinite(torch.tensor(float(v))) for v in r.recorder.stats[0].values())
    assert not torch.equal(r.model.memory.weight_ih, sd["memory.weight_ih"]) and not torch.equal(r.model.actor[0].weight, sd["actor.0.weight"])


# ------------------------------------------------------------------ 6. one composition
def test_terrain_curriculum_height_scan_critic_and_a_two_layer_trunk():
    over = {"terrain.type": "trimesh", "terrain.curriculum": True, "terrain.num_levels": 3, "terrain.max_init_level": 2, "terrain.measure_heights": True,
            "env.num_privileged_obs": 14 + 15, "algorithm.actor_hidden": [128, 128], **GRID_5x3}
    r = _runner(**over)
    assert r.model.actor[0].in_features == H and r.model.actor[0].out_features == 128 and r.model.critic[0].in_features == 47 + 29
    r.train_iteration(0)
    r._flush_log()
    torch.cuda.synchronize()
    s = r.recorder.stats[0]
    assert torch.isfinite(r.optimizer.flat).all() and all(torch.isfinite(torch.tensor(float(v))) for v in s.values()) and "terrain/mean_level" in s


# ------------------------------------------------------------------ 7. the key off
def test_key_off_runs_todays_calls_alone(monkeypatch, teacher_ck):  # noqa: F811
    from booster_gym_amd import _lib

    lib = _lib.load()

    def forbidden(*a):
        raise AssertionError("a recurrent actor's entry point ran with the key off")

    for name in GRU_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, forbidden)
    for cfg in (_cfg(**{KEY: 0}), _cfg()):
        if cfg["algorithm"]["rnn_hidden_size"]:
            del cfg["algorithm"]["rnn_hidden_size"]  # absent, as in the shipped yaml
        r = _runner(cfg=cfg)
        assert r._mem_tr is None and not hasattr(r.model, "memory") and not hasattr(r, "_last_dones")
        assert [k for k, _ in r.model.named_parameters()] == ["logstd"] + [f"{n}.{i}.{w}" for n in ("critic", "actor") for i in (0, 2, 4, 6) for w in ("weight", "bias")]
        for it in range(2):
            r.train_iteration(it)
        r._flush_log()
        torch.cuda.synchronize()
        del r
    # a distillation iteration with a recurrent student keeps its four launches: two column sums per epoch, never the new entry
    monkeypatch.undo()
    counts = {"bg_elu_backward_colsum": 0, "bg_gru_bias_partial": 0}
    for name in counts:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    d = _distiller(teacher_ck)
    d.train_iteration(0)
    torch.cuda.synchronize()
    assert counts == {"bg_elu_backward_colsum": 2 * d.dcfg.num_epochs, "bg_gru_bias_partial": 0}, counts
