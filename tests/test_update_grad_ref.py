"""tests/update_grad_ref.step_gradients_f64 against the oracle it restates (oracle/ppo_ref.ppo_update_reference, pinned by tests/golden/ppo_*.npz): a
hand-built record of a tiny float64 batch gives the gradients of the reference loop's first step to 1e-12 of each tensor's largest entry -- plain, and
with the mirror-symmetry term against a copy of tests/test_gpu_symmetry.ppo_update_sym_reference's loss; and the recurrent form (a record with h0 and
resets) against the same loop on tests/test_gpu_actor_memory._Restated's model, a GRU cell of 128 in front of the trunk, with resets.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.ppo_ref import discount_values, ppo_update_reference, surrogate_loss
from update_grad_ref import step_gradients_f64

T, N, A, NO, NP = 3, 8, 4, 10, 5
WIDTHS = (32, 32, 16)
ALG = {"bound_coef": 1.0, "entropy_coef": -0.01}


def _make_model():
    from booster_gym_amd.utils.model import ActorCritic

    return ActorCritic(A, NO, NP, WIDTHS, WIDTHS)


def _batch(seed=3):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    torch.manual_seed(seed)
    model = _make_model().double()
    with torch.no_grad():
        model.logstd.copy_(torch.linspace(-1.0, 0.2, A).view(1, A))
        model.actor[-1].bias.add_(1.2)  # (some means beyond +-1: the bound loss has a gradient)
    obses, priv, last_obs, last_priv = rn(T, N, NO), rn(T, N, NP), rn(N, NO), rn(N, NP)
    actions, rewards = rn(T, N, A), rn(T, N)
    dones, time_outs = torch.zeros(T, N, dtype=torch.bool), torch.zeros(T, N, dtype=torch.bool)
    dones[1, 2] = dones[0, 5] = time_outs[1, 6] = time_outs[2, 0] = True
    return model, obses, priv, actions, rewards, dones, time_outs, last_obs, last_priv


def _padded(x, width):
    out = torch.zeros(x.shape[0], width, dtype=x.dtype)
    out[:, : x.shape[1]] = x
    return out


def _record(model, params, obses, priv, actions, raw_adv, returns, partners=None):
    """What record_steps clones in front of a step, built by hand: the rows padded with zero columns as the runner pads them (15 -> 16, 10 -> 16)."""
    B = T * N
    with torch.no_grad():
        old_logp = model.act(obses).log_prob(actions).sum(-1).reshape(B)
    x_a = obses.reshape(B, NO) if partners is None else torch.cat((obses.reshape(B, NO), partners.reshape(B, NO)))
    return dict(params=params, x_c=_padded(torch.cat((obses, priv), -1).reshape(B, NO + NP), 16), x_a=_padded(x_a, 16), actions=actions.reshape(B, A),
                old_logp=old_logp, adv=raw_adv.reshape(B), ret=returns.reshape(B), rows=B, adv_all=raw_adv.clone())


def _assert_same(got, want):
    assert list(got) == list(want)
    for k in want:
        err, top = (got[k] - want[k]).abs().max().item(), want[k].abs().max().item()
        assert got[k].dtype == torch.float64 and top > 0 and err <= 1e-12 * top, (k, err, top)


def test_step_gradients_reproduce_the_reference_loops_first_step():
    model, obses, priv, actions, rewards, dones, time_outs, last_obs, last_priv = _batch()
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    rec = {}
    ppo_update_reference(model, torch.optim.Adam(model.parameters(), lr=1e-5), obses, priv, actions, rewards.clone(), dones, time_outs, last_obs, last_priv,
                         mini_epochs=1, record=rec)
    assert any(not torch.equal(p, params[k]) for k, p in model.named_parameters())  # (the loop has stepped: the record below starts from the clones)
    start = _make_model().double()
    start.load_state_dict(params)
    record = _record(start, params, obses, priv, actions, rec["raw_adv"], rec["returns"])
    aux = {}
    _assert_same(step_gradients_f64(record, _make_model, ALG, aux=aux), rec["grads"])
    assert aux["bound_loss"] > 0 and np.allclose((aux["value_loss"], aux["actor_loss"], aux["bound_loss"], aux["entropy"]), rec["losses"], rtol=1e-12, atol=0)
    # the normalisation is the whole batch's, with the unbiased std: the population std is another gradient (1 / (2B) in the actor's tensors)
    wrong = step_gradients_f64(record, _make_model, ALG, unbiased=False)
    k = "actor.0.weight"
    assert (wrong[k] - rec["grads"][k]).abs().max().item() > 1e-3 * rec["grads"][k].abs().max().item()
    assert torch.equal(wrong["critic.0.weight"], step_gradients_f64(record, _make_model, ALG)["critic.0.weight"])
    # a non-zero padding column is refused
    record["x_a"][3, 12] = 1.0
    try:
        step_gradients_f64(record, _make_model, ALG)
    except AssertionError as e:
        assert "padding" in str(e)
    else:
        raise AssertionError("a non-zero padding column went through")


def test_step_gradients_with_the_symmetry_term_reproduce_the_symmetric_loops_first_step():
    model, obses, priv, actions, rewards, dones, time_outs, last_obs, last_priv = _batch(seed=4)
    g = torch.Generator().manual_seed(1)
    obs_src, act_src = torch.randperm(NO, generator=g), torch.tensor([1, 0, 3, 2])
    obs_sign = torch.where(torch.rand(NO, generator=g) < 0.5, -1.0, 1.0).double()
    act_sign = torch.tensor([1.0, 1.0, -1.0, -1.0], dtype=torch.float64)
    coef = 10.0
    # --- a copy of the first mini-epoch of tests/test_gpu_symmetry.ppo_update_sym_reference's loop, up to loss.backward()
    obses_m = obses[..., obs_src.long()] * obs_sign
    with torch.no_grad():
        old_dist = model.act(obses)
        old_actions_log_prob = old_dist.log_prob(actions).sum(dim=-1)
    values = model.est_value(obses, priv)
    last_values = model.est_value(last_obs, last_priv)
    with torch.no_grad():
        rewards[time_outs] = values[time_outs]
        advantages = discount_values(rewards, dones | time_outs, values, last_values, 0.995, 0.95)
        returns = values + advantages
        raw_adv = advantages.clone()
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    value_loss = F.mse_loss(values, returns)
    dist = model.act(obses)
    actions_log_prob = dist.log_prob(actions).sum(dim=-1)
    actor_loss = surrogate_loss(old_actions_log_prob, actions_log_prob, advantages)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    entropy = dist.entropy().sum(dim=-1)
    sym_loss = (model.actor(obses_m) - dist.loc[..., act_src.long()] * act_sign).square().mean()
    loss = value_loss + actor_loss + 1.0 * bound_loss + -0.01 * entropy.mean() + coef * sym_loss
    loss.backward()
    # ---
    want = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    record = _record(model, params, obses, priv, actions, raw_adv, returns.detach(), partners=obses_m)
    maps = (obs_src.numpy(), obs_sign.numpy(), act_src.numpy(), act_sign.numpy())
    aux = {}
    _assert_same(step_gradients_f64(record, _make_model, ALG, extra=("symmetry", coef, maps), aux=aux), want)
    assert aux["pair_loss"] > 0 and abs(aux["pair_loss"] - sym_loss.item()) <= 1e-12 * sym_loss.item()
    # the smoothness term is the same pair term on the identity action map
    ident = (obs_src.numpy(), obs_sign.numpy(), np.arange(A), np.ones(A))
    _assert_same(step_gradients_f64(record, _make_model, ALG, extra=("smoothness", coef)), step_gradients_f64(record, _make_model, ALG, extra=("symmetry", coef, ident)))


def test_recurrent_step_gradients_reproduce_the_reference_loop_on_the_restated_model():
    """The reference's loop (oracle/ppo_ref.py, unedited) on _Restated -- the cell over the T steps from h0, a zero state behind a reset, the trunk on
    every state -- against step_gradients_f64 on a hand-built record with h0 and resets.  Without back-propagation through time the cell's recurrent
    weights get another gradient."""
    from booster_gym_amd.utils.model import ActorCritic
    from test_gpu_actor_memory import _Restated

    H = 128
    make = lambda: ActorCritic(A, NO, NP, WIDTHS, WIDTHS, memory_hidden=H)
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    torch.manual_seed(5)
    model = make().double()
    with torch.no_grad():
        model.logstd.copy_(torch.linspace(-1.0, 0.2, A).view(1, A))
        model.actor[-1].bias.add_(1.2)
    obses, priv, last_obs, last_priv, actions, rewards = rn(T, N, NO), rn(T, N, NP), rn(N, NO), rn(N, NP), rn(T, N, A), rn(T, N)
    h0 = rn(N, H) * 0.5
    dones, time_outs = torch.zeros(T, N, dtype=torch.bool), torch.zeros(T, N, dtype=torch.bool)
    dones[1, 2] = dones[0, 5] = time_outs[1, 6] = time_outs[2, 0] = True
    resets = torch.zeros(T, N, dtype=torch.uint8)
    resets[0, 3] = resets[0, 4] = 1                      # (step 0: the done flags of the iteration before)
    resets[1:] = (dones | time_outs)[: T - 1].to(torch.uint8)  # an env that ended enters its next step with a zero state
    assert bool(resets[1:].any()) and not bool(resets.all())
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    rec = {}
    ppo_update_reference(_Restated(model, h0, resets), torch.optim.Adam(model.parameters(), lr=1e-5), obses, priv, actions, rewards.clone(), dones, time_outs, last_obs,
                         last_priv, mini_epochs=1, record=rec)
    assert any(not torch.equal(p, params[k]) for k, p in model.named_parameters())
    start = make().double()
    start.load_state_dict(params)
    B = T * N
    with torch.no_grad():
        old_logp = _Restated(start, h0, resets).act(obses).log_prob(actions).sum(-1).reshape(B)
    record = dict(params=params, x_c=_padded(torch.cat((obses, priv), -1).reshape(B, NO + NP), 16), x_a=_padded(obses.reshape(B, NO), 16), actions=actions.reshape(B, A),
                  old_logp=old_logp, adv=rec["raw_adv"].reshape(B), ret=rec["returns"].reshape(B), rows=B, adv_all=rec["raw_adv"].clone(), h0=h0, resets=resets)
    aux = {}
    got = step_gradients_f64(record, make, ALG, aux=aux)
    assert {"memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"} <= set(got)
    _assert_same(got, rec["grads"])
    assert np.allclose((aux["value_loss"], aux["actor_loss"], aux["bound_loss"], aux["entropy"]), rec["losses"], rtol=1e-12, atol=0)
    # no back-propagation through time is another gradient of the recurrent weights (and the same one of the critic)
    cut = step_gradients_f64(record, make, ALG, bptt=False)
    k = "memory.weight_hh"
    assert (cut[k] - rec["grads"][k]).abs().max().item() > 1e-2 * rec["grads"][k].abs().max().item()
    assert torch.equal(cut["critic.0.weight"], got["critic.0.weight"])
    # a recurrent record against a feed-forward model is refused (the parameters do not load)
    try:
        step_gradients_f64(record, _make_model, ALG)
    except (AssertionError, RuntimeError):
        pass
    else:
        raise AssertionError("a recurrent record went through a feed-forward model")
