"""The rollout's actor launch on packed weights (bg_actor_pack + bg_actor_sample, csrc/bg_ppo.hip): the mean against a float64 evaluation of the same
layers, the sample against mu + exp(logstd) n with n recovered from a second call, determinism in (seed, counter), guard rows around the outputs, a
NaN behind the last observation row, the zero column that pads the first layer, and what a packed copy does when the parameters change under it."""
import copy

import pytest
import torch

from booster_gym_amd import _lib
from booster_gym_amd.utils.model import ActorCritic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 15, 16, 17, 33, 250)  # one partial tile, exact tiles, one row past a tile, one past a pair of tiles, several workgroups with a ragged last one
ATOL = 2e-5  # tests/test_gpu_ppo.py:101 (test_actor_sample_kernel_matches_torch_actor): the fused rollout actor's bound on mu
CANARY, GUARD = -12345.5, 64


def _model(seed=0):
    """random weights and biases at 1 / sqrt(fan-in), logstd in [-1, 0]"""
    torch.manual_seed(seed)
    m = ActorCritic(12, 47, 14).to(DEV)
    with torch.no_grad():
        for l in m.actor:
            if isinstance(l, torch.nn.Linear):
                l.weight.copy_(torch.randn_like(l.weight) / l.in_features ** 0.5)
                l.bias.copy_(torch.randn_like(l.bias) / l.in_features ** 0.5)
        m.logstd.copy_(-torch.rand_like(m.logstd))
    return m


def _mu64(m, obs):
    x = obs.double()
    lin = [l for l in m.actor if isinstance(l, torch.nn.Linear)]
    for i, l in enumerate(lin):
        x = x @ l.weight.detach().double().t() + l.bias.detach().double()
        if i + 1 < len(lin):
            x = torch.nn.functional.elu(x)
    return x


def _guarded(n):
    full = torch.full((n + 2 * GUARD, 12), CANARY, device=DEV)
    return full, full[GUARD : GUARD + n]


def _sample(m, obs, seed, counter, packed=None):
    """(mu, actions) in buffers with guard rows on both sides, which must come back untouched"""
    n = obs.shape[0]
    (mu_full, mu), (act_full, act) = _guarded(n), _guarded(n)
    m.sample_actions(obs, act, seed, counter, mu_out=mu, packed=packed)
    for full in (mu_full, act_full):
        assert (full[:GUARD] == CANARY).all() and (full[GUARD + n :] == CANARY).all(), "a guard row was written"
        assert (full[GUARD : GUARD + n] != CANARY).all()
    return mu.clone(), act.clone()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def observations():
    """[251][47]: row N of a test's rows is NaN in that test's own copy"""
    torch.manual_seed(1)
    return torch.randn(max(ROWS) + 1, 47, device=DEV)


@pytest.mark.parametrize("n", ROWS)
def test_mean_sample_determinism_and_guards(model, observations, n):
    store = observations[: n + 1].clone()
    store[n] = float("nan")  # just past the valid rows: must reach no output
    obs = store[:n]
    mu, act = _sample(model, obs, 5, 3)
    assert torch.isfinite(mu).all() and torch.isfinite(act).all()
    err = (mu.double() - _mu64(model, obs)).abs().max().item()
    print(f"N = {n}: max |mu - float64| = {err:.3e}")
    assert err <= ATOL, (n, err)
    # the noise, from a second call with logstd = 0: actions = mu + 1 * n
    zero = copy.deepcopy(model)
    with torch.no_grad():
        zero.logstd.zero_()
    mu0, act0 = _sample(zero, obs, 5, 3)
    assert torch.equal(mu0, mu)
    noise = act0 - mu0
    want = mu + torch.exp(model.logstd.detach()) * noise
    assert torch.allclose(act, want, rtol=0, atol=4 * torch.finfo(torch.float32).eps * max(1.0, act.abs().max().item())), (act - want).abs().max()
    assert noise.abs().max() < 7 and (noise != 0).any()  # (act0 - mu0 rounds: the comparison above allows a few ulps of the largest action)
    mu2, act2 = _sample(model, obs, 5, 3)
    assert torch.equal(mu2, mu) and torch.equal(act2, act), "the same (seed, counter) gave other bits"
    mu3, act3 = _sample(model, obs, 5, 4)
    assert torch.equal(mu3, mu) and not torch.equal(act3, act), "another counter must move the noise and nothing else"


def test_packed_first_layer_pads_column_47_with_zeros(model):
    packed = model.pack_actor()
    assert packed.numel() == _lib.ACTOR_PACKED_FLOATS and packed.data_ptr() % 16 == 0
    l0 = packed[: 4 * 4 * 3 * 64 * 4].view(4, 4, 3, 64, 4)  # [wave][j][q][lane][c] = W0[16 (wave + 4 j) + (lane & 15)][4 (4 q + c) + (lane >> 4)]
    assert (l0[:, :, 2, 48:, 3] == 0).all(), "column 47 of the packed first layer"
    w0 = model.actor[0].weight.detach()
    for wave, j, q, lane, c in ((0, 0, 0, 0, 0), (3, 2, 1, 37, 2), (1, 3, 2, 63, 2), (2, 1, 2, 47, 3)):
        assert l0[wave, j, q, lane, c] == w0[16 * (wave + 4 * j) + (lane & 15), 4 * (4 * q + c) + (lane >> 4)]


def test_a_packed_copy_is_a_snapshot_and_packing_again_follows_the_weights(observations):
    m = _model(2)
    obs = observations[:33].contiguous()
    packed = m.pack_actor()
    mu_a, act_a = _sample(m, obs, 9, 1, packed=packed)
    with torch.no_grad():
        for l in m.actor:
            if isinstance(l, torch.nn.Linear):
                l.weight[3, 5] += 0.25
    # documented (include/booster_gym_amd.h, ActorCritic.pack_actor): without packing again the launch still computes the packed snapshot
    mu_stale, act_stale = _sample(m, obs, 9, 1, packed=packed)
    assert torch.equal(mu_stale, mu_a) and torch.equal(act_stale, act_a)
    mu_b, act_b = _sample(m, obs, 9, 1, packed=m.pack_actor())
    assert not torch.equal(mu_b, mu_a)
    assert (mu_b.double() - _mu64(m, obs)).abs().max().item() <= ATOL
    fresh = ActorCritic(12, 47, 14).to(DEV)
    fresh.load_state_dict(m.state_dict())
    mu_f, act_f = _sample(fresh, obs, 9, 1)  # packs by itself
    assert torch.equal(mu_f, mu_b) and torch.equal(act_f, act_b), "a re-packed model and a fresh one differ"
