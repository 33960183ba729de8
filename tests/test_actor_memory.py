"""algorithm.rnn_hidden_size without a GPU: the key's rules (runner.rnn_hidden_size_of), its agreement with algorithm.actor_memory, the refused
combinations, the shipped yaml, the checkpoint rule of evaluate.py on plain dicts, the plan of an update on a recurrent actor, the new entry point
in header, bindings and library, and tools/play_oracle.py's host GRU step against torch.nn.GRUCell in float64."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "algorithm.rnn_hidden_size"


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", over)


def test_rnn_hidden_size_values():
    from booster_gym_amd.utils.runner import rnn_hidden_size_of

    assert rnn_hidden_size_of(_cfg()) == 0 and rnn_hidden_size_of(_cfg(**{KEY: 0})) == 0
    assert rnn_hidden_size_of(_cfg(**{KEY: 128})) == 128 and rnn_hidden_size_of(_cfg(**{KEY: 256})) == 256
    assert rnn_hidden_size_of(_cfg(**{KEY: 128, "algorithm.rnn_type": "gru"})) == 128
    for bad in (64, True, 128.0, "128", -128, 512):
        with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size"):
            rnn_hidden_size_of(_cfg(**{KEY: bad}))
    for kind in ("lstm", "GRU", 1):
        with pytest.raises(ValueError, match=r"algorithm\.rnn_type.*algorithm\.rnn_hidden_size"):
            rnn_hidden_size_of(_cfg(**{KEY: 128, "algorithm.rnn_type": kind}))
    with pytest.raises(ValueError, match=r"algorithm\.rnn_type"):  # (also with the cell off: there is one cell type)
        rnn_hidden_size_of(_cfg(**{"algorithm.rnn_type": "lstm"}))


def test_agreement_with_actor_memory():
    from booster_gym_amd.utils.runner import actor_memory_of, rnn_hidden_size_of

    both = _cfg(**{KEY: 128, "algorithm.actor_memory": 128})
    assert rnn_hidden_size_of(both) == actor_memory_of(both) == 128
    assert rnn_hidden_size_of(_cfg(**{"algorithm.actor_memory": 128})) == 0  # the re-entry key alone is not the training key
    assert actor_memory_of(_cfg(**{KEY: 128})) == 0
    for a, b in ((128, 256), (256, 128)):
        with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*algorithm\.actor_memory"):
            rnn_hidden_size_of(_cfg(**{KEY: a, "algorithm.actor_memory": b}))


REFUSED = {"estimator.enabled": ({"estimator.enabled": True}, r"estimator\.enabled"),
           "env.frame_stack": ({"env.frame_stack": 3, "env.num_observations": 141}, r"env\.frame_stack"),
           "terrain.actor_heights": ({"terrain.actor_heights": True, "terrain.measure_heights": True}, r"terrain\.actor_heights"),
           "algorithm.symmetry_loss": ({"algorithm.symmetry_loss": True}, r"algorithm\.symmetry_loss"),
           "algorithm.empirical_normalization": ({"algorithm.empirical_normalization": True}, r"algorithm\.empirical_normalization"),
           "runner.num_mini_batches": ({"runner.num_mini_batches": 4}, r"runner\.num_mini_batches")}


@pytest.mark.parametrize("other", sorted(REFUSED))
def test_refused_combinations_name_both_keys(other):
    from booster_gym_amd.utils.runner import rnn_hidden_size_of

    over, pattern = REFUSED[other]
    with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*" + pattern):
        rnn_hidden_size_of(_cfg(**{KEY: 128, **over}))
    assert rnn_hidden_size_of(_cfg(**over)) == 0  # ... and the other key alone is none of this function's business


def test_more_than_one_rank_is_refused_and_the_rest_composes():
    from booster_gym_amd.utils.runner import rnn_hidden_size_of

    with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*rank"):
        rnn_hidden_size_of(_cfg(**{KEY: 128}), world_size=2)
    assert rnn_hidden_size_of(_cfg(**{KEY: 128}), world_size=1) == 128
    composes = {"terrain.curriculum": True, "terrain.measure_heights": True, "commands.curriculum": True, "algorithm.actor_hidden": [128, 128],
                "algorithm.critic_hidden": [512, 256, 128], "env.frame_stack": 1, "runner.num_mini_batches": 1}
    assert rnn_hidden_size_of(_cfg(**{KEY: 256, **composes})) == 256


def test_shipped_config_lists_neither_key():
    alg = _cfg()["algorithm"]
    assert "rnn_hidden_size" not in alg and "rnn_type" not in alg and "actor_memory" not in alg
    text = open(os.path.join(ROOT, "booster_gym_amd", "envs", "T1.yaml")).read()
    assert "rnn_hidden_size" in text  # (the comment block describes it)


def test_checkpoint_rule_on_plain_dicts():
    from booster_gym_amd.utils.distill import checkpoint_student_overrides
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import checkpoint_memory_overrides

    for H in (128, 256):
        sd = ActorCritic(12, 47, 14, memory_hidden=H).state_dict()
        trained = {"model": sd, "optimizer": {}, "curriculum": None}
        assert checkpoint_memory_overrides(trained) == {KEY: H} and checkpoint_student_overrides(trained) is None
        student = {"model": sd, "distillation": {"teacher": "t.pth", "iteration": 1, "loss": 0.1, "student_memory": H}}
        assert checkpoint_memory_overrides(student) is None  # a student re-enters under its own overrides
        assert checkpoint_student_overrides(student)["algorithm.actor_memory"] == H
    plain = {"model": ActorCritic(12, 47, 14).state_dict()}
    assert checkpoint_memory_overrides(plain) is None and checkpoint_student_overrides(plain) is None
    assert checkpoint_memory_overrides({}) is None


def test_plan_of_an_update_on_a_recurrent_actor():
    """The trunk behind the cell runs the per-layer kernels beside the critic's chains, nothing runs ahead in the rollout, and the tail is the
    separate launches; memory = 0 is today's plan, field by field."""
    from booster_gym_amd.utils.runner import plan_update

    sw = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
              defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
    critic, actor = ((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64)
    today = plan_update(critic, actor, 24 * 4096, **sw)
    assert plan_update(critic, actor, 24 * 4096, memory=0, **sw) == today and today.one_tail and today.ahead
    for H in (128, 256):
        plan = plan_update(critic, ((H, 256, 128, 128, 12), H), 24 * 4096, memory=H, **sw)
        assert (plan.actor.fwd, plan.actor.bwd, plan.critic.fwd, plan.critic.bwd) == ("layer", "layer", "chain_split", "chain_split")
        assert all(plan.actor.grouped[:-1]) and plan.defer and plan.fused_opt and not plan.one_tail and not plan.ahead and not plan.one_stream and plan.wgrad == 0
    for bad in ({"split": 9}, {"fused_head": False}, {"defer_finish": False}, {"fused": False}):
        with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size"):
            plan_update(critic, ((128, 256, 128, 128, 12), 128), 24 * 4096, memory=128, **{**sw, **bad})
    with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*rows"):
        plan_update(critic, ((128, 256, 128, 128, 12), 128), 35, memory=128, **sw)


def test_new_entry_point_is_declared_bound_and_exported():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    m = re.search(r"\bint bg_gru_bias_partial\(([^;]*)\);", header)
    assert m and "bg_gru_bias_partial" in _lib.SYMBOLS
    fn = _lib.load().bg_gru_bias_partial
    assert len(fn.argtypes) == len(m.group(1).split(",")) == 6
    src = open(os.path.join(ROOT, "booster_gym_amd", "csrc", "bg_gru.hip")).read()
    kernel = src[src.index("gru_bias_partial_kernel"):]
    assert "atomic" not in kernel[: kernel.index("int check_shape")]  # a fixed order: no atomics in the new kernel


def _play_oracle():
    spec = importlib.util.spec_from_file_location("play_oracle", os.path.join(ROOT, "tools", "play_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("H", [128, 256])
def test_play_oracle_gru_step_matches_grucell_in_float64(H, tmp_path):
    from booster_gym_amd.utils.model import ActorCritic

    mod = _play_oracle()
    torch.manual_seed(H)
    model = ActorCritic(12, 47, 14, memory_hidden=H)
    path = str(tmp_path / "recurrent.pth")
    torch.save({"model": model.state_dict()}, path)
    mem, layers = mod.load_memory(path), mod.load_actor(path, memory=True)
    assert mem.hidden == H and np.all(mem.h == 0) and layers[0][0].shape == (256, H)
    cell, trunk = model.memory.double(), model.actor.double()
    xs = torch.randn(7, 47, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    h = torch.zeros(1, H, dtype=torch.float64)
    for t in range(7):
        if t == 4:  # an episode ends: both sides start again from a zero state
            mem.reset()
            h = torch.zeros_like(h)
            assert np.all(mem.h == 0)
        with torch.no_grad():
            h = cell(xs[t : t + 1], h)
            mu = trunk(h)[0].numpy()
        got = mem.step(xs[t].numpy())
        assert got.dtype == np.float64 and np.abs(got - h[0].numpy()).max() <= 1e-12, t
        assert np.abs(mod.mlp(layers, got) - mu).max() <= 1e-5  # (the trunk's weights are the checkpoint's fp32 values on both sides)
    plain = str(tmp_path / "plain.pth")
    torch.save({"model": ActorCritic(12, 47, 14).state_dict()}, plain)
    assert mod.load_memory(plain) is None and len(mod.load_actor(plain)) == 4


def test_messages_point_to_the_training_key():
    from booster_gym_amd.utils.model import ActorCritic

    with pytest.raises(ValueError, match=r"stateful.*algorithm\.rnn_hidden_size"):
        ActorCritic(12, 47, 14, memory_hidden=128).act(torch.zeros(2, 47))
