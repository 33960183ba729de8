"""algorithm.rnn_input: "row" on the GPU: bg_actor_sample_gru_row / _lstm_row against float64 torch.nn.GRUCell / LSTMCell and the trunk on the CPU, against
the 47-input launches at K = 47, their argument checks, and one update of an LSTM actor on the stacked / perceptive row against float64 autograd
through the steps.  Bounds: tests/test_gpu_lstm.py's (forward 2e-5 max(1, |ref|max), gradients 1e-4 of the tensor's largest entry)."""
import copy

import pytest
import torch

from test_gpu_actor_memory import CLIP, SHORT_EPISODES, _cfg, _runner
from test_gpu_distill_memory import _bound, _grad_bound
from test_gpu_lstm import FILL, _guarded, _Policy64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELLS = [("gru", 128, (256, 128, 128)), ("gru", 256, (512, 128)), ("lstm", 128, (256, 128, 128)), ("lstm", 256, (512, 128)), ("lstm", 512, (512, 256, 128))]


def _actor(cell, H, trunk, K):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(H + K)
    m = ActorCritic(12, K, 14, actor_hidden=trunk, memory_hidden=H, memory_cell=cell, memory_input=K).to(DEV)
    with torch.no_grad():
        m.memory.bias_ih.normal_(0.0, 0.1); m.memory.bias_hh.normal_(0.0, 0.1)
    return m


def _sample(m, obs, reset, s_in, s_out, mu, row=True, desc=None):
    """The cell's launch (its _row form, or the 47-input one) on the rows of obs; s_in / s_out: the state tensors, [N][H] or the LSTM's [2][N][H]."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import layer_descriptors

    lin, p, N = [l for l in m.actor if isinstance(l, torch.nn.Linear)], _lib.ptr, obs.shape[0]
    states = (s_in[0], s_out[0], s_in[1], s_out[1]) if m.memory_cell == "lstm" else (s_in, s_out)
    act = torch.zeros(N, 12, device=DEV)
    rc = getattr(_lib.load(), f"bg_actor_sample_{m.memory_cell}" + ("_row" if row else ""))(
        N, p(obs), obs.stride(0), desc or m.gru_descriptor(), len(lin), layer_descriptors(lin), p(m.logstd), 11, 3, p(reset), *[p(s) for s in states], p(mu), p(act),
        _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, act


@pytest.mark.parametrize("K", [47, 94, 234, 256])
@pytest.mark.parametrize("cell, H, trunk", CELLS)
def test_row_launches_against_float64(cell, H, trunk, K):
    """Rows K + 5 floats apart with NaN in the 5 columns behind the cell's K: nothing of them may reach an output.  The second call runs in place."""
    m = _actor(cell, H, trunk, K)
    m64, S = copy.deepcopy(m).double().cpu(), (2 if cell == "lstm" else 1)
    for N in (1, 17, 40):
        g = torch.Generator().manual_seed(N)
        rows = torch.full((N, K + 5), float("nan"), device=DEV)
        rows[:, :K] = torch.randn(N, K, generator=g).to(DEV)
        state = torch.randn(S, N, H, generator=g).to(DEV)
        reset = torch.zeros(N, dtype=torch.uint8, device=DEV)
        reset[1::3] = 1
        out, mu = torch.stack([_guarded(N, H) for _ in range(S)]), _guarded(N, 12)
        s_in, s_out = (state, out) if cell == "lstm" else (state[0], out[0])
        rc, act = _sample(m, rows[:, :K], reset, s_in, s_out, mu)
        assert rc == 0
        with torch.no_grad():
            kept = state.double().cpu() * (1 - reset.cpu().double()).view(1, N, 1)
            new = m64.memory(rows[:, :K].double().cpu(), (kept[0], kept[1]) if cell == "lstm" else kept[0])
            new = torch.stack(new) if cell == "lstm" else new[None]
            mu64 = m64.actor(new[0])
        assert torch.all(out[:, N] == FILL) and torch.all(mu[N] == FILL), "a row at or beyond N was written"
        _bound(out[:, :N].cpu(), new, f"{cell} {H} K {K} N {N} state")
        _bound(mu[:N].cpu(), mu64, f"{cell} {H} K {K} N {N} mu")
        assert bool(torch.isfinite(act).all())
        io, mu_io = state.clone(), _guarded(N, 12)
        _sample(m, rows[:, :K], reset, io if cell == "lstm" else io[0], io if cell == "lstm" else io[0], mu_io)
        assert torch.equal(io, out[:, :N]) and torch.equal(mu_io, mu)


@pytest.mark.parametrize("cell, H, trunk", CELLS)
def test_47_inputs_equal_the_existing_launch_bit_for_bit(cell, H, trunk):
    m, N, S = _actor(cell, H, trunk, 47), 40, (2 if cell == "lstm" else 1)
    g = torch.Generator().manual_seed(7)
    obs, state = torch.randn(N, 47, generator=g).to(DEV), torch.randn(S, N, H, generator=g).to(DEV)
    reset = (torch.arange(N, device=DEV) % 4 == 1).to(torch.uint8)
    got = []
    for row in (False, True):
        out, mu = torch.zeros(S, N, H, device=DEV), torch.zeros(N, 12, device=DEV)
        rc, act = _sample(m, obs, reset, state if cell == "lstm" else state[0], out if cell == "lstm" else out[0], mu, row=row)
        assert rc == 0
        got.append((out, mu, act))
    assert all(torch.equal(a, b) for a, b in zip(*got))


@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("K, stride, want", [(46, 64, -4), (257, 260, -4), (94, 93, -1)])
def test_argument_checks_return_before_any_launch(cell, K, stride, want):
    from booster_gym_amd import _lib

    m, N = _actor(cell, 128, (256, 128, 128), 94), 4
    d = m.gru_descriptor()
    d = type(d)(d.W_ih, d.W_hh, d.b_ih, d.b_hh, K, 128)
    obs = torch.zeros(N, stride, device=DEV)
    state, mu = torch.full((2, N, 128), FILL, device=DEV), torch.full((N, 12), FILL, device=DEV)
    rc, act = _sample(m, obs, None, state if cell == "lstm" else state[0], state if cell == "lstm" else state[0], mu, desc=d)
    assert rc == want and f"bg_actor_sample_{cell}_row" in _lib.load().bg_last_error().decode()
    assert torch.all(state == FILL) and torch.all(mu == FILL) and torch.all(act == 0)


SCAN = {"terrain.type": "trimesh", "terrain.measure_heights": True, "terrain.actor_heights": True, "terrain.measured_points_x": [-0.2, 0.0, 0.2],
        "terrain.measured_points_y": [-0.1, 0.1], "env.num_observations": 53, "env.num_privileged_obs": 20}


@pytest.mark.parametrize("over, K", [({"env.frame_stack": 2, "env.num_observations": 94}, 94), (SCAN, 53)])
def test_one_update_and_the_checkpoint(over, K, tmp_path):
    """test_gpu_lstm's gradient test on the row: the first mini-epoch's gradients against float64 autograd through the T steps from the rollout's state;
    then the checkpoint in a runner that plays gives the training runner's mean, bit for bit."""
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import Runner, checkpoint_memory_overrides
    from oracle.ppo_ref import surrogate_loss

    keys = {"env.num_envs": 128, "algorithm.rnn_cell": "lstm", "algorithm.rnn_input": "row", **over}
    r = _runner(**{"algorithm.learning_rate": 1.0e-5, **SHORT_EPISODES, **keys})
    mt, alg, T = r._mem_tr, r.cfg["algorithm"], r.cfg["runner"]["horizon_length"]
    assert tuple(r.model.memory.weight_ih.shape) == (512, K) and mt.kin == r._actor_in.shape[-1] >= K
    r._fused_opt = False
    with torch.no_grad():
        r.model.logstd.zero_()
    r.invalidate()
    r.optimizer.max_grad_norm = CLIP
    r.rollout()  # a rollout first: the one below starts from a state that is not zero
    r.buffer.roll()
    r.rollout()
    b = r.buffer
    if not bool(b["dones"][: T - 1].any()):  # (no env ended inside the horizon: force one, and the flags the update reads with it)
        b["dones"][1, ::3] = True
        mt.resets[2].copy_(b["dones"][1])
    first, step = {}, r.optimizer.step

    def spy():
        if not first:
            first.update({k: q.grad.clone() for k, q in r.model.named_parameters()}, adv=r._adv.clone())
        step()

    r.optimizer.step = spy
    start = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    r.update()
    torch.cuda.synchronize()
    net = ActorCritic(12, K, r.env.num_privileged_obs, r.actor_hidden, r.critic_hidden, memory_hidden=128, memory_cell="lstm", memory_input=K).to(DEV)
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
            _grad_bound(first[k], q.grad, f"K {K} grad {k}")

    ck, path = r.checkpoint_dict(), str(tmp_path / "row.pth")
    assert checkpoint_memory_overrides(ck) == {"algorithm.rnn_hidden_size": 128, "algorithm.rnn_cell": "lstm", "algorithm.rnn_input": "row"}
    torch.save(ck, path)
    with pytest.raises(ValueError, match=r"algorithm\.rnn_input"):  # the 47-input cell's config against this checkpoint
        Runner(test=True, cfg=_cfg(**{"basic.checkpoint": path, "algorithm.rnn_cell": "lstm", "env.num_envs": 128}))
    player = Runner(test=True, cfg=_cfg(**{"basic.checkpoint": path, **keys})).model
    obs, reset, means = b["obses"][0].contiguous(), torch.ones(128, dtype=torch.uint8, device=DEV), []
    for model in (r.model, player):
        mu, act = torch.zeros(128, 12, device=DEV), torch.zeros(128, 12, device=DEV)
        model.sample_actions(obs, act, 1, 0, mu_out=mu, reset=reset, scan=K % 47)
        means.append(mu)
    torch.cuda.synchronize()
    assert torch.equal(*means) and bool(means[0].abs().max() > 0)
