"""rnd.enabled without a GPU: the section's rules (every refusal names its key), the key off, the weight's schedule, the defaults of the other
sections with the section present, the host restatement of the reward normaliser's merge, and the model with and without the two networks."""
import numpy as np
import pytest
import torch


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", {"rnd.enabled": True, "rnd.weight": 0.5, **over})


def test_defaults_and_key_off():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.rnd import DEFAULTS, RND_WIDTH, RndCfg, RndSchedule, rnd_cfg, rnd_enabled

    shipped = load_cfg("T1")
    assert shipped["rnd"] == DEFAULTS and DEFAULTS["enabled"] is False and DEFAULTS["weight"] is None and RND_WIDTH == 12  # every key, at its default: off
    assert rnd_cfg(shipped) is None and not rnd_enabled(shipped)
    absent = load_cfg("T1")
    del absent["rnd"]
    assert rnd_cfg(absent) is None  # a yaml written before the section existed
    null = load_cfg("T1")
    null["rnd"] = None
    assert rnd_cfg(null) is None
    assert rnd_cfg(load_cfg("T1", {"rnd.enabled": None})) is None
    sparse = load_cfg("T1")
    sparse["rnd"] = {}
    assert rnd_cfg(sparse) is None  # `enabled` absent
    # off: nothing else of the section is read, nor the rank count
    assert rnd_cfg(load_cfg("T1", {"rnd.weight": "nonsense", "rnd.state": 7, "rnd.target_hidden": [7], "rnd.momentum": 1}), world_size=8) is None
    on = rnd_cfg(_cfg())
    assert on == RndCfg(0.5, None, "critic", 61, (256, 128), (256, 128), 1, 1.0e-3, 1.0, True)
    sparse["rnd"] = {"enabled": True, "weight": 0.5}
    assert rnd_cfg(sparse) == on  # absent keys: the defaults
    got = rnd_cfg(_cfg(**{"rnd.weight": 0, "rnd.state": "actor", "rnd.predictor_hidden": [512, 256, 128], "rnd.target_hidden": [512, 128], "rnd.num_epochs": 3,
                          "rnd.learning_rate": 1, "rnd.max_grad_norm": 0.5, "rnd.reward_normalization": False,
                          "rnd.weight_schedule": {"mode": "linear", "initial_step": 0, "final_step": 10, "final_value": 0}}))
    assert got == (0.0, RndSchedule(0, 10, 0.0), "actor", 47, (512, 256, 128), (512, 128), 3, 1.0, 0.5, False)
    # the widest rows: the critic's with the height scan (61 + 187), a frame stack of ten for the actor (470)
    scan = {"terrain.measure_heights": True, "env.num_privileged_obs": 14 + 187}
    assert rnd_cfg(_cfg(**scan)).width == 248
    assert rnd_cfg(_cfg(**{"env.frame_stack": 10, "env.num_observations": 470, "rnd.state": "actor"})).width == 470


SCHED = {"mode": "linear", "initial_step": 2, "final_step": 6, "final_value": 0.1}


@pytest.mark.parametrize("over,match", [
    ({"rnd.enabled": 1}, r"rnd\.enabled must be true or false"),
    ({"rnd.enabled": "yes"}, r"rnd\.enabled must be true or false"),
    ({"rnd.weight": None}, r"rnd\.weight must be a finite number >= 0.*no default"),
    ({"rnd.weight": -0.1}, r"rnd\.weight"),
    ({"rnd.weight": float("inf")}, r"rnd\.weight"),
    ({"rnd.weight": float("nan")}, r"rnd\.weight"),
    ({"rnd.weight": True}, r"rnd\.weight"),
    ({"rnd.weight": "1"}, r"rnd\.weight"),
    ({"rnd.weight_schedule": "linear"}, r"rnd\.weight_schedule must be null or a mapping"),
    ({"rnd.weight_schedule": dict(SCHED, mode="step")}, r"rnd\.weight_schedule\.mode"),
    ({"rnd.weight_schedule": {k: v for k, v in SCHED.items() if k != "mode"}}, r"rnd\.weight_schedule\.mode"),
    ({"rnd.weight_schedule": dict(SCHED, initial_step=-1)}, r"rnd\.weight_schedule\.initial_step"),
    ({"rnd.weight_schedule": dict(SCHED, final_step=2.5)}, r"rnd\.weight_schedule\.final_step"),
    ({"rnd.weight_schedule": dict(SCHED, final_step=2)}, r"rnd\.weight_schedule\.final_step = 2 must be above rnd\.weight_schedule\.initial_step = 2"),
    ({"rnd.weight_schedule": dict(SCHED, final_value=-1)}, r"rnd\.weight_schedule\.final_value"),
    ({"rnd.weight_schedule": {k: v for k, v in SCHED.items() if k != "final_value"}}, r"rnd\.weight_schedule\.final_value"),
    ({"rnd.weight_schedule": dict(SCHED, power=2)}, r"rnd\.weight_schedule\.power is not a key"),
    ({"rnd.state": "privileged"}, r"rnd\.state must be"),
    ({"rnd.state": 1}, r"rnd\.state must be"),
    ({"rnd.predictor_hidden": [256]}, r"rnd\.predictor_hidden"),
    ({"rnd.predictor_hidden": [256, 256]}, r"rnd\.predictor_hidden"),
    ({"rnd.target_hidden": [128, 100, 128]}, r"rnd\.target_hidden"),
    ({"rnd.target_hidden": [128] * 5}, r"rnd\.target_hidden"),
    ({"rnd.predictor_hidden": [512, 128], "parallel.gemm_split": 9}, r"gemm_split.*rnd\.predictor_hidden"),
    ({"rnd.num_epochs": 0}, r"rnd\.num_epochs"),
    ({"rnd.num_epochs": 1.5}, r"rnd\.num_epochs"),
    ({"rnd.learning_rate": 0}, r"rnd\.learning_rate"),
    ({"rnd.learning_rate": float("nan")}, r"rnd\.learning_rate"),
    ({"rnd.max_grad_norm": -1.0}, r"rnd\.max_grad_norm"),
    ({"rnd.max_grad_norm": True}, r"rnd\.max_grad_norm"),
    ({"rnd.reward_normalization": 1}, r"rnd\.reward_normalization must be true or false"),
    ({"rnd.num_outputs": 16}, r"rnd\.num_outputs is not a key"),
    # 47 x 10 + 14 = 484 columns for the critic's row; the actor's 470 fit
    ({"env.frame_stack": 10, "env.num_observations": 470}, r"rnd\.state = 'critic'.*484 columns, above 480"),
    ({"env.frame_stack": 10, "env.num_observations": 481, "rnd.state": "actor"}, r"rnd\.state = 'actor'.*481 columns, above 480"),
])
def test_refusals_name_their_key(over, match):
    from booster_gym_amd.utils.rnd import rnd_cfg

    with pytest.raises(ValueError, match=match):
        rnd_cfg(_cfg(**over))


def test_missing_weight_and_more_than_one_rank_are_refused():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.rnd import rnd_cfg

    with pytest.raises(ValueError, match=r"rnd\.weight must be a finite number >= 0 when rnd\.enabled is on"):
        rnd_cfg(load_cfg("T1", {"rnd.enabled": True}))  # the shipped section, switched on: there is no default weight
    cfg = load_cfg("T1")
    cfg["rnd"] = {"enabled": True}
    with pytest.raises(ValueError, match=r"rnd\.weight"):
        rnd_cfg(cfg)
    with pytest.raises(ValueError, match=r"rnd\.enabled.*one rank \(WORLD_SIZE = 2\)"):
        rnd_cfg(_cfg(), world_size=2)
    with pytest.raises(ValueError, match=r"rnd must be a mapping"):
        rnd_cfg({"rnd": [1]})


def test_weight_schedule():
    from booster_gym_amd.utils.rnd import rnd_cfg, weight_at

    const = rnd_cfg(_cfg())
    assert [weight_at(const, i) for i in (0, 1, 1000)] == [0.5, 0.5, 0.5]
    lin = rnd_cfg(_cfg(**{"rnd.weight_schedule": SCHED}))  # 0.5 up to iteration 2, linear to 0.1 at 6, 0.1 behind it
    assert [weight_at(lin, i) for i in (0, 1, 2)] == [0.5, 0.5, 0.5]
    assert [weight_at(lin, i) for i in (3, 4, 5)] == pytest.approx([0.4, 0.3, 0.2], rel=1e-15)
    assert [weight_at(lin, i) for i in (6, 7, 10 ** 6)] == [0.1, 0.1, 0.1]
    up = rnd_cfg(_cfg(**{"rnd.weight": 0, "rnd.weight_schedule": {"mode": "linear", "initial_step": 0, "final_step": 4, "final_value": 2.0}}))
    assert [weight_at(up, i) for i in range(6)] == [0.0, 0.5, 1.0, 1.5, 2.0, 2.0]


def test_other_sections_defaults_are_unchanged_by_the_section():
    """The section's presence with enabled false changes nothing another section's reader returns, nor a value of the shipped yaml."""
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.estimator import DEFAULTS as EST_DEFAULTS, estimator_cfg
    from booster_gym_amd.utils.runner import env_mini_batches, hidden_widths, mini_batches, rnn_critic_of, rnn_hidden_size_of, smoothness_loss, symmetry_loss
    from booster_gym_amd.utils.value_norm import normalize_value_of

    with_sec, without = load_cfg("T1"), load_cfg("T1")
    del without["rnd"]
    assert with_sec["rnd"]["enabled"] is False
    assert {k: v for k, v in with_sec.items() if k != "rnd"} == without
    assert with_sec["estimator"] == EST_DEFAULTS and with_sec["algorithm"]["learning_rate"] == 1.0e-5 and with_sec["runner"]["horizon_length"] == 24
    for f in (rnn_hidden_size_of, estimator_cfg, rnn_critic_of, hidden_widths, mini_batches, env_mini_batches, smoothness_loss, symmetry_loss, normalize_value_of):
        assert f(with_sec) == f(without), f.__name__
    assert rnn_hidden_size_of(with_sec) == 0 and estimator_cfg(with_sec) is None
    on = {"algorithm.rnn_hidden_size": 128, "estimator.enabled": False}
    assert rnn_hidden_size_of(load_cfg("T1", on)) == 128
    assert estimator_cfg(load_cfg("T1", {"estimator.enabled": True})) == estimator_cfg(load_cfg("T1", {"estimator.enabled": True, "rnd.enabled": False}))


def test_merge_restatement_is_the_variance_of_the_concatenation():
    """merge_f64 (what tests/test_gpu_rnd.py holds the device state to) over batches of very different means and scales against numpy's mean and
    population variance of all samples: 1e-12 relative."""
    from booster_gym_amd.utils.rnd import merge_f64

    rng = np.random.default_rng(5)
    batches = [np.abs(rng.normal(0.05, 0.02, 640)), np.abs(rng.normal(1.5, 0.7, 3072)), np.abs(rng.normal(9.0, 2.5, 1000)), np.zeros(0), np.array([3.25])]
    state = (0.0, 1.0, 0.0)
    for b in batches:
        state = merge_f64(state, (b.sum(), (b * b).sum(), float(b.size)))
    allx = np.concatenate(batches)
    assert state[2] == allx.size
    assert abs(state[0] - allx.mean()) <= 1e-12 * abs(allx.mean()) and abs(state[1] - allx.var()) <= 1e-12 * allx.var()
    assert merge_f64((0.3, 2.0, 7.0), (0.0, 0.0, 0.0)) == (0.3, 2.0, 7.0)  # an empty batch leaves the state


def test_model_with_and_without_the_networks():
    """The two modules are registered last, drawn from a generator of their own: the other parameters and the global generator's next draw are as
    without them; PPO's optimiser would hold what it holds without the key; the target takes no gradient."""
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.rnd import module_seed

    torch.manual_seed(3)
    plain = ActorCritic(12, 47, 14)
    after_plain = torch.rand(4)
    torch.manual_seed(3)
    m = ActorCritic(12, 47, 14, rnd=(61, (256, 128), (512, 128), module_seed(3)))
    after = torch.rand(4)
    assert torch.equal(after, after_plain)
    names = [n for n, _ in m.named_parameters()]
    k = len(list(plain.named_parameters()))
    assert names[:k] == [n for n, _ in plain.named_parameters()] and all(n.startswith("rnd_predictor.") for n in names[k : k + 6]) and all(n.startswith("rnd_target.") for n in names[k + 6 :])
    assert all(torch.equal(p, q) for p, q in zip(plain.parameters(), m.parameters()))
    assert [n for n, p in m.named_parameters() if any(p is q for q in m.ppo_parameters())] == names[:k]
    assert all(p.requires_grad for p in m.rnd_predictor.parameters()) and not any(p.requires_grad for p in m.rnd_target.parameters())
    assert m.rnd_predictor[0].weight.shape == (256, 61) and m.rnd_target[0].weight.shape == (512, 61) and m.rnd_predictor[-1].out_features == m.rnd_target[-1].out_features == 12
    for net in (m.rnd_predictor, m.rnd_target):  # torch.nn.Linear's range
        for l in (x for x in net if isinstance(x, torch.nn.Linear)):
            b = 1.0 / np.sqrt(l.in_features)
            assert l.weight.abs().max().item() <= b and l.bias.abs().max().item() <= b and l.weight.std().item() > 0.4 * b
    again = ActorCritic(12, 47, 14, rnd=(61, (256, 128), (512, 128), module_seed(3)))  # whatever the global generator's state
    assert all(torch.equal(p, q) for p, q in zip(m.rnd_target.parameters(), again.rnd_target.parameters()))
    other = ActorCritic(12, 47, 14, rnd=(61, (256, 128), (512, 128), module_seed(4)))
    assert not torch.equal(other.rnd_target[0].weight, m.rnd_target[0].weight) and module_seed(3) != module_seed(4)
