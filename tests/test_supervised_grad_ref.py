"""tests/supervised_grad_ref.supervised_gradients_f64 against the loops it restates: a hand-built float64 record of a tiny network gives, to 1e-12 of
each tensor's largest entry, the gradients of the first step of tests/test_gpu_distill._check_one_iteration's loop (plain), of
tests/test_gpu_distill_symmetry._check_one_symmetric_iteration's (with the symmetric term, under the model's own action mirror) and of
tests/test_gpu_distill_memory._loss_f64 (a GRU cell of 128 in front of the network, with resets); the switches that produce the WRONG references of the
GPU file's controls move what they say they move and nothing else.  No GPU."""
import torch

from supervised_grad_ref import supervised_gradients_f64

T, N, A, NO, KIN = 3, 8, 12, 10, 16
WIDTHS = (32, 32, 16)
B = T * N


def _actor_critic(memory=0):
    from booster_gym_amd.utils.model import ActorCritic

    return ActorCritic(A, NO, 5, WIDTHS, WIDTHS, **({"memory_hidden": memory} if memory else {}))


def _make_net(n_in=NO):
    from booster_gym_amd.utils.model import _mlp

    return lambda: _mlp(n_in, WIDTHS, A)


def _data(seed, memory=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    torch.manual_seed(seed)
    model = _actor_critic(memory).double()
    return model, rn(T, N, NO), rn(T, N, A), rn


def _padded(x):
    out = torch.zeros(x.shape[0], KIN, dtype=x.dtype)
    out[:, : x.shape[1]] = x
    return out


def _params(model):
    """The record's names of a model's trained tensors in the order of Distiller's optimiser: memory.* as they are, then actor.* as net.*."""
    named = dict(model.named_parameters())
    return {**{k: p for k, p in named.items() if k.startswith("memory.")}, **{"net." + k[len("actor."):]: p for k, p in named.items() if k.startswith("actor.")}}


def _assert_same(got, want):
    assert list(got) == list(want)
    for k in want:
        err, top = (got[k] - want[k]).abs().max().item(), want[k].abs().max().item()
        assert got[k].dtype == torch.float64 and top > 0 and err <= 1e-12 * top, (k, err, top)


def _refused(fn, word):
    try:
        fn()
    except AssertionError as e:
        assert word in str(e), e
    else:
        raise AssertionError(f"{word}: went through")


def test_plain_gradients_reproduce_the_cloning_loops_first_step():
    model, obses, labels, _ = _data(3)
    rows, y = obses.reshape(B, NO), labels.reshape(B, A)
    params = {k: p.detach().clone() for k, p in _params(model).items()}
    # --- tests/test_gpu_distill._check_one_iteration's loop, up to loss.backward()
    loss = ((model.actor(rows) - y) ** 2).mean()
    loss.backward()
    # ---
    want = {k: p.grad.detach().clone() for k, p in _params(model).items()}
    record = dict(params=params, x=_padded(rows), target=y, rows=B, symmetry=None)
    aux = {}
    got = supervised_gradients_f64(record, _make_net(), aux=aux)
    _assert_same(got, want)
    assert abs(aux["cloning_loss"] - loss.item()) <= 1e-12 * loss.item() and aux["loss"] == aux["cloning_loss"] and aux["symmetric_loss"] is None
    # the fp32 twin: the same loss in torch's own fp32, close to and not equal to float64's
    twin = supervised_gradients_f64(record, _make_net(), dtype=torch.float32)
    for k in want:
        err = (twin[k].double() - want[k]).abs().max().item() / want[k].abs().max().item()
        assert twin[k].dtype == torch.float32 and 0 < err < 1e-5, (k, err)
    # the controls' wrong references: the padded row count scales every tensor by B / padded; the doubled column sums move the hidden biases alone
    scaled = supervised_gradients_f64(record, _make_net(), mean_rows=32)
    _assert_same({k: g * (32 / B) for k, g in scaled.items()}, want)
    doubled = supervised_gradients_f64(record, _make_net(), hidden_bias_scale=2.0)
    hidden_biases = {"net.0.bias", "net.2.bias", "net.4.bias"}
    assert all(torch.equal(doubled[k], (2.0 if k in hidden_biases else 1.0) * got[k]) for k in want) and hidden_biases < set(want) and "net.6.bias" in want
    # a non-zero padding column is refused, and so are rows that are not the targets'
    bad = dict(record, x=record["x"].clone())
    bad["x"][3, 12] = 1.0
    _refused(lambda: supervised_gradients_f64(bad, _make_net()), "padding")
    _refused(lambda: supervised_gradients_f64(dict(record, x=torch.cat((record["x"], record["x"]))), _make_net()), str(B))


def test_symmetric_gradients_reproduce_the_symmetric_loops_first_step():
    from test_gpu_distill_symmetry import _maps, _mirror_actions

    _, _, act_src, act_sign = _maps()
    assert len(act_src) == A and list(act_src) != list(range(A)) and (act_sign < 0).any()  # a non-trivial M_a: the model's own
    model, obses, labels, rn = _data(4)
    coef = 10.0
    rows, y = obses.reshape(B, NO), labels.reshape(B, A)
    g = torch.Generator().manual_seed(1)
    obs_src, obs_sign = torch.randperm(NO, generator=g), torch.where(torch.rand(NO, generator=g) < 0.5, -1.0, 1.0).double()
    mrows = rows[:, obs_src] * obs_sign
    params = {k: p.detach().clone() for k, p in _params(model).items()}
    # --- tests/test_gpu_distill_symmetry._check_one_symmetric_iteration's loop, up to backward()
    mu = model.actor(rows)
    bc, sym = ((mu - y) ** 2).mean(), ((model.actor(mrows) - _mirror_actions(mu, act_src, act_sign)) ** 2).mean()
    (bc + coef * sym).backward()
    # ---
    want = {k: p.grad.detach().clone() for k, p in _params(model).items()}
    record = dict(params=params, x=_padded(torch.cat((rows, mrows))), target=y, rows=B,
                  symmetry=(coef, torch.as_tensor(act_src, dtype=torch.long), torch.as_tensor(act_sign, dtype=torch.float64)))
    aux = {}
    got = supervised_gradients_f64(record, _make_net(), aux=aux)
    _assert_same(got, want)
    assert abs(aux["cloning_loss"] - bc.item()) <= 1e-12 * bc.item() and abs(aux["symmetric_loss"] - sym.item()) <= 1e-12 * sym.item() and sym.item() > 0
    assert abs(aux["loss"] - (bc.item() + coef * sym.item())) <= 1e-12 * aux["loss"]
    # each term's gradient alone: they add up to the whole, the cloning one is the gradient of the record without the term
    _assert_same({k: aux["cloning_grads"][k] + aux["symmetric_grads"][k] for k in want}, want)
    alone = supervised_gradients_f64(dict(record, x=record["x"][:B], symmetry=None), _make_net())
    _assert_same(aux["cloning_grads"], alone)
    assert all(aux["symmetric_grads"][k].abs().max().item() > 0 for k in want)
    # the control: with M_a net(x[:B]) detached the original half carries the cloning term alone -- another gradient in every tensor
    cut = supervised_gradients_f64(record, _make_net(), detach_mirrored_original=True)
    for k in want:
        assert (cut[k] - want[k]).abs().max().item() > 1e-3 * want[k].abs().max().item(), k
    # a record with the term needs 2B rows
    _refused(lambda: supervised_gradients_f64(dict(record, x=record["x"][:B]), _make_net()), str(B))


def test_recurrent_gradients_reproduce_the_loss_through_time():
    from test_gpu_distill_memory import _loss_f64

    H = 128
    model, obses, labels, rn = _data(5, memory=H)
    h0 = rn(N, H) * 0.5
    resets = torch.zeros(T, N, dtype=torch.uint8)
    resets[0, 3] = resets[0, 4] = resets[1, 2] = resets[2, 6] = resets[2, 0] = 1
    params = {k: p.detach().clone() for k, p in _params(model).items()}
    assert list(params)[:4] == ["memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"] and len(params) == 12
    loss, _ = _loss_f64(model, obses, labels, h0, resets)  # (tests/test_gpu_distill_memory's restatement, unedited)
    loss.backward()
    want = {k: p.grad.detach().clone() for k, p in _params(model).items()}
    record = dict(params=params, x=_padded(obses.reshape(B, NO)), target=labels.reshape(B, A), rows=B, symmetry=None, h0=h0, resets=resets)
    make_cell = lambda: torch.nn.GRUCell(NO, H)
    aux = {}
    got = supervised_gradients_f64(record, _make_net(H), make_cell, aux=aux)
    _assert_same(got, want)
    assert abs(aux["cloning_loss"] - loss.item()) <= 1e-12 * loss.item()
    # no back-propagation through time is another gradient of the recurrent weights, and the same one of the output layer
    cut = supervised_gradients_f64(record, _make_net(H), make_cell, bptt=False)
    k = "memory.weight_hh"
    assert (cut[k] - want[k]).abs().max().item() > 1e-2 * want[k].abs().max().item()
    assert torch.equal(cut["net.6.weight"], got["net.6.weight"])
    # the resets count: without them the gradient is another one
    other = supervised_gradients_f64(dict(record, resets=torch.zeros_like(resets)), _make_net(H), make_cell)
    assert (other[k] - want[k]).abs().max().item() > 1e-3 * want[k].abs().max().item()
    # a recurrent record without a cell, and a feed-forward one with a cell, are refused
    for rec, cell in ((record, None), ({k: v for k, v in record.items() if k not in ("h0", "resets")}, make_cell)):
        try:
            supervised_gradients_f64(rec, _make_net(H), cell)
        except AssertionError:
            pass
        else:
            raise AssertionError("a record and a cell that do not belong together went through")
