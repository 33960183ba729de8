"""estimator.enabled without a GPU: the section's rules (every refusal names its key), the key off, the regression target built from a privileged row,
the model with and without the third network, and the exported composition."""
import pytest
import torch


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", {"estimator.enabled": True, **over})


def test_defaults_and_key_off():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.estimator import DEFAULTS, EST_WIDTH, EstimatorCfg, estimator_cfg, estimator_enabled

    shipped = load_cfg("T1")
    assert shipped["estimator"] == DEFAULTS and DEFAULTS["enabled"] is False and EST_WIDTH == 12  # the shipped yaml names every key, at its default: off
    assert estimator_cfg(shipped) is None and not estimator_enabled(shipped)
    absent = load_cfg("T1")
    del absent["estimator"]
    assert estimator_cfg(absent) is None  # a yaml written before the section existed
    # off: nothing else of the section is read, nor what the key does not compose with
    assert estimator_cfg(load_cfg("T1", {"estimator.targets": "nonsense", "estimator.hidden": [7], "algorithm.symmetry_loss": True}), world_size=8) is None
    assert estimator_cfg(load_cfg("T1", {"estimator.enabled": None})) is None
    on = estimator_cfg(_cfg())
    assert on == EstimatorCfg((4, 5, 6, 7), (256, 128), 2, 1.0e-3, 1.0)
    sparse = _cfg()
    sparse["estimator"] = {"enabled": True}
    assert estimator_cfg(sparse) == on  # absent keys: the defaults
    got = estimator_cfg(_cfg(**{"estimator.targets": [13, 0], "estimator.hidden": [512, 256, 128], "estimator.num_epochs": 5, "estimator.learning_rate": 1,
                                "estimator.max_grad_norm": 0.5}))
    assert got == ((13, 0), (512, 256, 128), 5, 1.0, 0.5)
    # with the critic's height scan its columns are legal targets; 47 x 10 + 10 = 480 is the widest actor row
    scan = {"terrain.measure_heights": True, "env.num_privileged_obs": 14 + 187}
    assert estimator_cfg(_cfg(**{"estimator.targets": [4, 200], **scan})).targets == (4, 200)
    assert len(estimator_cfg(_cfg(**{"env.frame_stack": 10, "env.num_observations": 470, "estimator.targets": list(range(10))})).targets) == 10


@pytest.mark.parametrize("over,match", [
    ({"estimator.enabled": 1}, r"estimator\.enabled must be true or false"),
    ({"estimator.enabled": "yes"}, r"estimator\.enabled must be true or false"),
    ({"estimator.targets": []}, r"estimator\.targets"),
    ({"estimator.targets": list(range(13))}, r"estimator\.targets"),
    ({"estimator.targets": [4, 4]}, r"estimator\.targets.*distinct"),
    ({"estimator.targets": [4, 14]}, r"estimator\.targets.*env\.num_privileged_obs - 1 = 13"),
    ({"estimator.targets": [-1]}, r"estimator\.targets"),
    ({"estimator.targets": [4.0]}, r"estimator\.targets"),
    ({"estimator.targets": [True]}, r"estimator\.targets"),
    ({"estimator.targets": 4}, r"estimator\.targets"),
    ({"estimator.hidden": [256]}, r"estimator\.hidden"),
    ({"estimator.hidden": [256, 256]}, r"estimator\.hidden"),
    ({"estimator.hidden": [128, 100, 128]}, r"estimator\.hidden"),
    ({"estimator.hidden": [128] * 5}, r"estimator\.hidden"),
    ({"estimator.hidden": [512, 128], "parallel.gemm_split": 9}, r"gemm_split.*estimator\.hidden"),
    ({"estimator.num_epochs": 0}, r"estimator\.num_epochs"),
    ({"estimator.num_epochs": 1.5}, r"estimator\.num_epochs"),
    ({"estimator.learning_rate": 0}, r"estimator\.learning_rate"),
    ({"estimator.learning_rate": float("nan")}, r"estimator\.learning_rate"),
    ({"estimator.max_grad_norm": -1.0}, r"estimator\.max_grad_norm"),
    ({"estimator.max_grad_norm": True}, r"estimator\.max_grad_norm"),
    ({"estimator.momentum": 0.9}, r"estimator\.momentum is not a key"),
    ({"env.frame_stack": 10, "env.num_observations": 470, "estimator.targets": list(range(11))}, r"estimator\.targets.*481 exceeds 480"),
    ({"algorithm.symmetry_loss": True}, r"estimator\.enabled.*algorithm\.symmetry_loss"),
    ({"algorithm.empirical_normalization": True}, r"estimator\.enabled.*algorithm\.empirical_normalization"),
    ({"terrain.actor_heights": True, "terrain.measure_heights": True}, r"estimator\.enabled.*terrain\.actor_heights"),
    ({"runner.num_mini_batches": 2}, r"estimator\.enabled.*runner\.num_mini_batches"),
])
def test_refusals_name_their_key(over, match):
    from booster_gym_amd.utils.estimator import estimator_cfg

    with pytest.raises(ValueError, match=match):
        estimator_cfg(_cfg(**over))


def test_more_than_one_rank_and_distillation_are_refused():
    from booster_gym_amd.utils.distill import distillation_cfg
    from booster_gym_amd.utils.estimator import estimator_cfg

    with pytest.raises(ValueError, match=r"estimator\.enabled.*one rank \(WORLD_SIZE = 2\)"):
        estimator_cfg(_cfg(), world_size=2)
    section = _cfg()
    section["estimator"] = [1, 2]
    with pytest.raises(ValueError, match=r"estimator must be a mapping"):
        estimator_cfg(section)
    dist = {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 + 187, "env.num_privileged_obs": 14 + 187}
    with pytest.raises(ValueError, match=r"estimator\.enabled.*distillation"):
        distillation_cfg(_cfg(**dist))
    assert distillation_cfg(_cfg(**{"estimator.enabled": False, **dist})) is not None


def test_target_row():
    from booster_gym_amd.utils.estimator import estimator_targets

    priv = torch.arange(3 * 5 * 14, dtype=torch.float32).reshape(3, 5, 14) + 0.5
    y = estimator_targets(priv, (4, 5, 6, 7))
    assert tuple(y.shape) == (3, 5, 12) and torch.equal(y[..., :4], priv[..., 4:8]) and not y[..., 4:].any()
    y = estimator_targets(priv.reshape(15, 14), (13, 0, 7))  # the order of `targets`
    assert torch.equal(y[:, 0], priv.reshape(15, 14)[:, 13]) and torch.equal(y[:, 1], priv.reshape(15, 14)[:, 0]) and torch.equal(y[:, 2], priv.reshape(15, 14)[:, 7])
    assert not y[:, 3:].any()
    out = torch.full((15, 12), 9.0)
    assert estimator_targets(priv.reshape(15, 14), tuple(range(12)), out=out) is out and torch.equal(out, priv.reshape(15, 14)[:, :12])
    out.fill_(9.0)
    estimator_targets(priv.reshape(15, 14), (1,), out=out)
    assert torch.equal(out[:, 0], priv.reshape(15, 14)[:, 1]) and not out[:, 1:].any()  # the tail is zeroed, whatever the buffer held


def test_model_without_an_estimator_is_todays():
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(0)
    m = ActorCritic(12, 47, 14)
    names = [k for k, _ in m.named_parameters()]
    want = ["logstd"] + [f"{net}.{i}.{t}" for net in ("critic", "actor") for i in (0, 2, 4, 6) for t in ("weight", "bias")]
    assert names == want and list(m.state_dict()) == want and not m.has_estimator and m.estimator_cols == 0 and not hasattr(m, "estimator")
    assert len(m.ppo_parameters()) == len(list(m.parameters())) and all(p is q for p, q in zip(m.ppo_parameters(), m.parameters()))
    torch.manual_seed(0)
    twin = ActorCritic(12, 47, 14, estimator_hidden=None, estimator_cols=4)  # (without widths there is no estimator, whatever the count)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), twin.state_dict().values())) and twin.actor[0].in_features == 47
    x = torch.randn(5, 47)
    assert torch.equal(m.act(x).loc, m.actor(x)) and m.actor_input(x) is x


@pytest.mark.parametrize("H,E,hidden", [(1, 4, (256, 128)), (3, 12, (128, 128, 128)), (2, 1, (512, 128))])
def test_model_with_an_estimator_and_the_export_wrapper(H, E, hidden, tmp_path):
    from booster_gym_amd.utils.model import ActorCritic, EstimatorActor, hidden_of

    torch.manual_seed(1)
    F = 47 * H
    m = ActorCritic(12, F, 14, estimator_hidden=hidden, estimator_cols=E)
    names = [k for k, _ in m.named_parameters()]
    assert names[:17] == [k for k, _ in ActorCritic(12, F, 14).named_parameters()]  # today's parameters first, in today's order
    assert all(k.startswith("estimator.") for k in names[17:]) and len(names) == 17 + 2 * (len(hidden) + 1)
    assert [k for k, _ in zip(names, m.ppo_parameters())] == names[:17] and len(m.ppo_parameters()) == 17
    assert (m.actor[0].in_features, m.critic[0].in_features, m.estimator[0].in_features, m.estimator[-1].out_features) == (F + E, F + 14, F, 12)
    assert hidden_of(m.state_dict(), "estimator") == hidden and m.has_estimator and m.estimator_cols == E
    with torch.no_grad():
        for p in m.estimator[-1].parameters():
            p.mul_(5.0)
    x = torch.randn(9, F)

    def elu_mlp(seq, v):  # the hand-written composition, float64
        lin = [l for l in seq if isinstance(l, torch.nn.Linear)]
        for k, l in enumerate(lin):
            v = v @ l.weight.double().t() + l.bias.double()
            if k + 1 < len(lin):
                v = torch.where(v > 0, v, torch.expm1(v))
        return v

    with torch.no_grad():
        e = elu_mlp(m.estimator, x.double())
        want = elu_mlp(m.actor, torch.cat((x.double(), e[:, :E]), dim=1))
        dist = m.act(x)
        assert (dist.loc.double() - want).abs().max().item() < 1e-5 and torch.allclose(dist.scale, torch.full((9, 12), float(torch.exp(torch.tensor(-2.0)))))
        assert torch.equal(m.actor_input(x)[:, :F], x) and (m.actor_input(x)[:, F:].double() - e[:, :E]).abs().max().item() < 1e-5
        m64 = ActorCritic(12, F, 14, estimator_hidden=hidden, estimator_cols=E)
        m64.load_state_dict(m.state_dict())
        assert (m64.double().act(x.double()).loc - want).abs().max().item() < 1e-12
        # columns [E, 12) of the estimator are never read by the actor
        if E < 12:
            before = m.act(x).loc.clone()
            m.estimator[-1].bias[E:] += 3.0
            assert torch.equal(m.act(x).loc, before)
        # the export wrapper: 47 H floats in, 12 out, through TorchScript and back
        path = str(tmp_path / "actor.pt")
        torch.jit.script(EstimatorActor(m.actor, m.estimator, E)).save(path)
        got = torch.jit.load(path, map_location="cpu")(x)
        assert tuple(got.shape) == (9, 12) and (got.double() - want).abs().max().item() < 1e-5
    with pytest.raises(ValueError, match="estimator_cols"):
        ActorCritic(12, F, 14, estimator_hidden=hidden, estimator_cols=13)
    with pytest.raises(ValueError, match="estimator_cols"):
        ActorCritic(12, F, 14, estimator_hidden=hidden, estimator_cols=0)
