"""The gradient of one optimiser step of Runner.update(), restated in float64 autograd on the step's own inputs -- TEST INFRASTRUCTURE, not a test file.

record_steps(runner)      records, around every call of Runner._epoch_gradients_and_step (the one seam every optimiser step of every plan goes through:
                          the whole batch on one stream or two, a row mini-batch), what the step's gradient is a function of and the gradient the
                          step left in FlatAdam.grad.  It changes no switch and no plan: the update runs the launches it would run without it.
step_gradients_f64(...)   evaluates oracle/ppo_ref.py:52-58's loss on such a record with torch autograd and returns {name: gradient}.

Because the record holds the update's own rows -- padded, stacked, normalised, mirrored as the networks read them -- the one function serves every
feature key; that those rows are the right ones is what each feature's own tests assert."""
import contextlib

import torch
import torch.nn.functional as F

from oracle.ppo_ref import surrogate_loss


@contextlib.contextmanager
def record_steps(runner):
    """`with record_steps(r) as steps: r.update()` -- steps: one dict per optimiser step, in order:
      params    {name: clone} of runner.model.named_parameters() in front of the step
      x_c, x_a  the critic's rows [rows][padded width], the actor's rows (2 x rows with a pair loss: the batch, then the partners)
      actions, old_logp, adv, ret, rows   the step's per-row streams (adv: raw) and the number of rows its loss is a mean over
      adv_all   the whole batch's raw advantages (the moments the step normalises with are the whole batch's)
      h0, resets   a recurrent actor only (v.mem is not None): the state [envs][H] the step's recurrence starts from and its reset flags uint8 [T][envs]
                   (an env-wise mini-batch: the gathered ones of its envs); x_a then holds the cell's padded rows [T envs][64], step-major
      grads     {name: clone} of the parameters' .grad views of FlatAdam.grad behind the step: the fused tails finish the weight gradients and write
                the log-std slice inside the launch, and no form of the step stores the clipped gradient back, so this is the complete unclipped one
      clip_sqnorm   the squared norm the clip divided by where the form leaves it readable (the separate launches: FlatAdam._gnorm; bg_update_tail:
                    its slots of FlatAdam._tail_norm + the log-std's squares, which that launch adds itself), None for bg_optimizer_step, which keeps
                    it in registers
      form      "separate" / "tail" / "fused": the form of FlatAdam the step ran
      plan      the UpdatePlan the step ran under (v.plan)."""
    steps, inner = [], runner._epoch_gradients_and_step
    named = lambda: list(runner.model.named_parameters())

    def recorded(u, v):
        # the side stream may still be writing what is cloned here (two-stream plans: the critic's half of the mini-epoch); the step itself starts
        # with this same hand-over
        torch.cuda.current_stream().wait_stream(runner._side_stream)
        B, plan, opt = v.rows, v.plan, runner.optimizer
        rec = dict(params={k: p.detach().clone() for k, p in named()}, x_c=v.x_c[:B].clone(), x_a=v.x_a.clone(), actions=v.actions.clone(),
                   old_logp=v.old_logp.clone(), adv=v.adv.clone(), ret=v.ret.clone(), rows=B, adv_all=runner._adv.clone(), plan=plan)
        if v.mem is not None:
            rec.update(h0=v.mem.h0.clone(), resets=v.mem.resets.clone())
        fused, one_tail = plan.fused_opt and not runner._lr_restart, plan.one_tail and not runner._lr_restart
        inner(u, v)
        rec["grads"] = {k: p.grad.clone() for k, p in named()}
        if not fused:
            rec["form"], rec["clip_sqnorm"] = "separate", opt._gnorm.clone().sum()
        elif one_tail and not plan.ranks:
            rec["form"] = "tail"
            # (every slot: the launch writes the same number of slots in every step of a runner under one plan, the rest are zero since allocation;
            #  a stale slot would make the norm too LARGE and fail the comparison, not hide anything)
            rec["clip_sqnorm"] = opt._tail_norm.sum() + sum((g.double() ** 2).sum() for k, g in rec["grads"].items() if k == "logstd")
        else:
            rec["form"], rec["clip_sqnorm"] = "fused", None
        steps.append(rec)

    runner._epoch_gradients_and_step = recorded
    try:
        yield steps
    finally:
        del runner._epoch_gradients_and_step  # (the instance attribute: the class's method is back)


def model_factory(runner):
    """make_model for a runner's ActorCritic, with the cell of a recurrent actor: the constructor call Runner.__init__ makes."""
    from booster_gym_amd.utils.model import ActorCritic

    env, memory = runner.env, getattr(runner, "_memory", 0)
    return lambda: ActorCritic(env.num_actions, env.num_obs, env.num_privileged_obs, runner.actor_hidden, runner.critic_hidden, memory_hidden=memory)


def recurrent_means(model, x_a, h0, resets, bptt=True):
    """The actor's means [T envs][12] of a recurrent model on the cell's rows x_a [T envs][47], step-major: the cell over the T steps from h0 [envs][H]
    with a zero state behind a reset (resets [T][envs]), the trunk on every state.  bptt = False detaches the state between steps: no
    back-propagation through time, a WRONG gradient for sensitivity controls."""
    T, n = resets.shape
    x, h, mus = x_a.reshape(T, n, -1), h0, []
    for t in range(T):
        h = model.memory(x[t], h * (1 - resets[t].to(h0.dtype)).view(n, 1))
        mus.append(model.actor(h))
        if not bptt:
            h = h.detach()
    return torch.cat(mus)


def step_gradients_f64(record, make_model, alg, extra=None, *, dtype=torch.float64, unbiased=True, aux=None, bptt=True):
    """The gradient of the step's loss at the recorded parameters, by torch autograd: the loss written out as oracle/ppo_ref.py:52-58 writes it.
      value term      mse(critic(x_c[:, :k_c]), ret)
      surrogate term  surrogate_loss on exp(logp - old_logp) with the recorded fp32 old_logp and the advantages (adv - mean) / (std + 1e-8), the
                      moments those of the whole batch's raw advantages in float64 with torch's unbiased std (a row mini-batch's rows too)
      + alg["bound_coef"] * bound loss + alg["entropy_coef"] * mean entropy
      extra           ("symmetry", coef, mirror_maps): + coef * mean |actor(x_a[B:]) - M_a mu(x_a[:B])|^2  (mirror_maps: env.mirror_maps())
                      ("smoothness", coef):            + coef * mean |actor(x_a[B:]) - mu(x_a[:B])|^2
                      -- tests/test_gpu_symmetry.ppo_update_sym_reference's and tests/test_gpu_smoothness.ppo_update_smooth_reference's terms on the
                      rows the actor trained on.
    The networks read the first in_features columns of x_c / x_a; the padding columns must be zero.  make_model() builds the ActorCritic, which
    is cast to `dtype` and loaded with the recorded parameters.  dtype = torch.float32: the same loss as torch's own fp32 autograd computes it (the
    moments still in float64).  unbiased = False: the population std, a WRONG reference for sensitivity controls.  aux: a dict that receives
    "ratio" (the rows' probability ratios) and the loss terms.  Returns {name: gradient} in `dtype`.
    A record with h0 / resets (a recurrent actor): x_a is read as [T][envs][padded 64], the means are recurrent_means' -- the cell over the T steps from
    h0, a zero state behind a reset, the trunk on every state -- and every loss line is the same (bptt: recurrent_means').  A feed-forward record
    takes the path it always took."""
    B, dev = record["rows"], record["x_c"].device
    model = make_model().to(device=dev, dtype=dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in record["params"].items()})
    recurrent = "h0" in record
    assert recurrent == bool(getattr(model, "memory_hidden", 0)) and not (recurrent and extra is not None)
    k_c, k_a = model.critic[0].in_features, model.memory.input_size if recurrent else model.actor[0].in_features
    x_c, x_a = record["x_c"], record["x_a"]
    assert x_c.shape[0] == B and x_a.shape[0] == (2 * B if extra is not None else B), (tuple(x_c.shape), tuple(x_a.shape), B)
    assert not x_c[:, k_c:].any() and not x_a[:, k_a:].any(), "the padding columns of the network inputs must be zero"
    x_c, x_a = x_c[:, :k_c].to(dtype), x_a[:, :k_a].to(dtype)
    actions, old_logp, ret = record["actions"].to(dtype), record["old_logp"].to(dtype), record["ret"].to(dtype)
    with torch.no_grad():
        adv_all = record["adv_all"].double().reshape(-1)
        advantages = ((record["adv"].double() - adv_all.mean()) / (adv_all.std(unbiased=unbiased) + 1e-8)).to(dtype)
    values = model.critic(x_c).squeeze(-1)
    value_loss = F.mse_loss(values, ret)
    mean = recurrent_means(model, x_a, record["h0"].to(dtype), record["resets"], bptt) if recurrent else model.actor(x_a[:B])
    dist = torch.distributions.Normal(mean, torch.exp(model.logstd).expand_as(mean))
    actions_log_prob = dist.log_prob(actions).sum(dim=-1)
    actor_loss = surrogate_loss(old_logp, actions_log_prob, advantages)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    entropy = dist.entropy().sum(dim=-1)
    loss = value_loss + actor_loss + alg["bound_coef"] * bound_loss + alg["entropy_coef"] * entropy.mean()
    pair_loss = None
    if extra is not None:
        kind, coef = extra[0], extra[1]
        if kind == "symmetry":
            act_src, act_sign = (torch.as_tensor(v, device=dev) for v in extra[2][2:])
            target = dist.loc[..., act_src.long()] * act_sign.to(dtype)
        elif kind == "smoothness":
            target = dist.loc
        else:
            raise ValueError(f"extra: {kind!r}")
        pair_loss = (model.actor(x_a[B:]) - target).square().mean()
        loss = loss + coef * pair_loss
    loss.backward()
    if aux is not None:
        aux.update(ratio=torch.exp(actions_log_prob - old_logp).detach(), value_loss=value_loss.item(), actor_loss=actor_loss.item(),
                   bound_loss=bound_loss.item(), entropy=entropy.mean().item(), pair_loss=None if pair_loss is None else pair_loss.item())
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}
