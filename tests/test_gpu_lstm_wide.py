"""The LSTM's launches at H = 512 (algorithm.rnn_hidden_size: 512 with rnn_cell: "lstm") and the 2,048-wide GEMMs under them, on the helpers, reference
and bounds of tests/test_gpu_lstm_shapes.py (tests/test_lstm_wide.py holds the fp32 twin at this width to a tenth of the bounds)."""
import copy

import pytest
import torch

from test_gpu_actor_memory import CLIP, SHORT_EPISODES, _cfg, _runner
from test_gpu_distill_memory import _bound, _grad_bound
from test_gpu_lstm import _Policy64
from test_gpu_lstm_shapes import (FORWARD, GRADS, _backward, _case, _cell_launch, _check_forward, _check_gradient, _cut, _forward, _lstm_model, _state_stores,
                                  test_bias_partial_at_and_around_its_record_size as _bias_partial)
from test_lstm_wide import WIDE_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 512
WIDE = {"algorithm.rnn_hidden_size": H, "algorithm.rnn_cell": "lstm"}


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_sequence_launches_match_float64(name):
    T, N, scale, reset, h0, c0 = WIDE_CASES[name]
    c = _case(T, N, H, scale, reset, h0, c0)
    out = _forward(T, N, H, c["gi"], c["h0"], c["c0"], c["reset"], c["cell"])
    for x, k in zip(out, FORWARD):
        _check_forward(x, c, k, name)
    grads = _backward(T, N, H, c["dh_ext"], out[4], out[1], c["reset"], c["cell"])
    for x, k in zip(grads, GRADS):
        _check_gradient(x, c, k, name)
    again = _backward(T, N, H, c["dh_ext"], out[4], out[1], c["reset"], c["cell"], want_dh0=False, want_dc0=False)  # LSTMTrainer.backward's call
    assert torch.equal(again[0], grads[0]) and again[1] is None and again[2] is None
    assert N != 40 or c["reset"] is None or 0 < int(c["reset"][1:].sum()) < 4 * N  # resets inside the horizon


def test_a_forward_launch_split_in_time_reproduces_the_single_launch():
    T, N, T1 = 5, 40, 2
    c = _case(T, N, H)
    whole = _forward(T, N, H, c["gi"], c["h0"], c["c0"], c["reset"], c["cell"])
    first = _forward(T1, N, H, _cut(c["gi"], 0, T1), c["h0"], c["c0"], _cut(c["reset"], 0, T1), c["cell"])
    second = _forward(T - T1, N, H, _cut(c["gi"], T1, T), first[2][T1 - 1].contiguous(), first[3][T1 - 1].contiguous(), _cut(c["reset"], T1, T), c["cell"])
    for a, b, w, k in zip(first, second, whole, FORWARD):
        assert torch.equal(torch.cat((a, b)), w), k


@pytest.mark.parametrize("B", [1, 127, 129, 516])
def test_bias_partial(B):
    _bias_partial(B, H)


@pytest.mark.parametrize("N", [1, 16, 17, 40])
@pytest.mark.parametrize("trunk", [(256, 128, 128), (512, 128)])
def test_rollout_launch(trunk, N):
    """Against the float64 cell + trunk, in place and out of place; h' / c' against step 0 of the update's recurrence (gi: bg_mlp_layer_forward, 2,048 columns)."""
    from booster_gym_amd import _lib
    model = _lstm_model(H, trunk)
    g = torch.Generator(device="cpu").manual_seed(1000 * H + N)
    obs = torch.cat((torch.randn(N, 47, generator=g), torch.full((1, 47), float("nan")))).to(DEV)
    h, c = (torch.randn(N, H, generator=g) * 0.5).to(DEV), (torch.randn(N, H, generator=g) * 0.5).to(DEV)
    reset = (torch.rand(N, generator=g) < 0.3).to(torch.uint8).to(DEV)
    keep = (1 - reset.double()).view(N, 1)
    with torch.no_grad():
        h_ref, c_ref = copy.deepcopy(model.memory).double()(obs[:N].double(), (h.double() * keep, c.double() * keep))
        mu_ref = copy.deepcopy(model.actor).double()(h_ref)
    stores = _state_stores(h, c)
    h_out, c_out, mu, act = got = _cell_launch("bg_actor_sample_lstm", model, reset, stores, N, False, obs=obs)
    for x, ref, k in ((h_out, h_ref, "h'"), (c_out, c_ref, "c'"), (mu, mu_ref, "mu")):
        _bound(x, ref, f"trunk {trunk} N {N} {k}")
    assert torch.isfinite(act).all() and not torch.equal(act, mu)
    for x, y, k in zip(_cell_launch("bg_actor_sample_lstm", model, reset, stores, N, True, obs=obs), got, ("h'", "c'", "mu", "actions")):
        assert torch.equal(x, y), ("in place against out of place", k)
    x, w_pad, gi = torch.zeros(N, 64, device=DEV), torch.zeros(4 * H, 64, device=DEV), torch.empty(N, 4 * H, device=DEV)
    x[:, :47], w_pad[:, :47] = obs[:N], model.memory.weight_ih.detach()
    _lib.check(_lib.load().bg_mlp_layer_forward(N, 64, 4 * H, _lib.ptr(x), _lib.ptr(w_pad), _lib.ptr(model.memory.bias_ih), _lib.ptr(gi), 0, _lib.current_stream_ptr()),
               "bg_mlp_layer_forward")
    torch.cuda.synchronize()
    _, _, upd_h, upd_c, _ = _forward(1, N, H, gi.view(1, N, 4 * H), h, c, reset.view(1, N), model.memory)
    _bound(upd_h[0], h_out.double(), f"trunk {trunk} N {N}: the update's h of step 0 against the rollout's")
    _bound(upd_c[0], c_out.double(), f"trunk {trunk} N {N}: the update's c of step 0 against the rollout's")


def test_one_update_matches_float64_autograd_and_the_checkpoint_plays(tmp_path):
    """tests/test_gpu_lstm.py's gradient test at 128 envs, T = 5, H = 512 (the 2,048-row weight gradients and bias sums); then the checkpoint plays."""
    from booster_gym_amd.utils.model import ActorCritic, LSTMTrainer
    from booster_gym_amd.utils.runner import Runner, checkpoint_memory_overrides
    from oracle.ppo_ref import surrogate_loss

    over = {"env.num_envs": 128, **WIDE}
    r = _runner(**{"algorithm.learning_rate": 1.0e-5, **SHORT_EPISODES, **over})
    mt, alg, T = r._mem_tr, r.cfg["algorithm"], r.cfg["runner"]["horizon_length"]
    assert isinstance(mt, LSTMTrainer) and tuple(r.model._memory_state.shape) == (2, 128, H) and tuple(r.model.memory.weight_hh.shape) == (4 * H, H)
    r._fused_opt = False
    with torch.no_grad():
        r.model.logstd.zero_()
    r.invalidate(); r.optimizer.max_grad_norm = CLIP
    r.rollout(); r.buffer.roll(); r.rollout()
    b = r.buffer
    b["dones"][1, ::3] = True  # (an env ends inside the horizon, and the flags the update reads with it)
    mt.resets[2].copy_(b["dones"][1])
    torch.cuda.synchronize()
    assert mt.h0.abs().max().item() > 1e-3 and bool(mt.resets[1:].any()) and not bool(mt.resets[1:].all())
    first, step = {}, r.optimizer.step

    def spy():
        if not first:
            first.update({k: q.grad.clone() for k, q in r.model.named_parameters()}, adv=r._adv.clone())
        step()

    r.optimizer.step, start = spy, {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    r.update(); torch.cuda.synchronize()
    net = ActorCritic(12, 47, r.env.num_privileged_obs, r.actor_hidden, r.critic_hidden, memory_hidden=H, memory_cell="lstm").to(DEV)
    net.load_state_dict(start)
    pol = _Policy64(net.double(), mt.h0, mt.resets)
    obses, actions = b["obses"][:T].double(), b["actions"].double()
    with torch.no_grad():
        old_logp = pol.dist(obses).log_prob(actions).sum(-1)
    adv = first["adv"].double()
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    dist = pol.dist(obses)
    bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
    (surrogate_loss(old_logp, dist.log_prob(actions).sum(-1), adv) + alg["bound_coef"] * bound_loss + alg["entropy_coef"] * dist.entropy().sum(-1).mean()).backward()
    for k, q in net.named_parameters():
        if k.startswith(("memory.", "actor.")):
            _grad_bound(first[k], q.grad, f"grad {k}")
    r.optimizer.step = step
    ck, path = r.checkpoint_dict(), str(tmp_path / "wide.pth")
    assert checkpoint_memory_overrides(ck) == WIDE
    torch.save(ck, path)
    play = Runner(test=True, cfg=_cfg(**{"basic.checkpoint": path, **over}))
    obs = torch.randn(128, 47, generator=torch.Generator().manual_seed(3)).to(DEV)
    mus = []
    for m in (r.model, play.model):
        m.reset_memory()
        act, mu = torch.zeros(128, 12, device=DEV), torch.zeros(128, 12, device=DEV)
        for t in range(2):
            m.sample_actions(obs, act, 1, t, mu_out=mu)
        mus.append(mu.clone())
    assert torch.isfinite(mus[0]).all() and mus[0].abs().max().item() > 0 and torch.equal(mus[0], mus[1])
