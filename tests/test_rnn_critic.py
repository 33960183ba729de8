"""algorithm.rnn_critic without a GPU: the key's values and errors (runner.rnn_critic_of), the shipped yaml, the model with a second cell
(critic_memory.* last, the critic's first layer on the cell's state, today's parameter order with the key off), the checkpoint rule of evaluate.py on
plain dicts, the plan of an update with both cells, the cell trainer's shape rules, and the two grouped entry points in header, bindings and library."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, RNN = "algorithm.rnn_critic", "algorithm.rnn_hidden_size"
TODAY = ["logstd"] + [f"{n}.{i}.{w}" for n in ("critic", "actor") for i in (0, 2, 4, 6) for w in ("weight", "bias")]
CELL = ["weight_ih", "weight_hh", "bias_ih", "bias_hh"]


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", over)


def test_rnn_critic_values():
    from booster_gym_amd.utils.runner import rnn_critic_of

    assert rnn_critic_of(_cfg()) == 0
    for off in (False, None):
        assert rnn_critic_of(_cfg(**{KEY: off})) == 0 and rnn_critic_of(_cfg(**{KEY: off, RNN: 128})) == 0
    assert rnn_critic_of(_cfg(**{RNN: 256})) == 0  # a recurrent actor alone keeps its feed-forward critic
    assert rnn_critic_of(_cfg(**{KEY: True, RNN: 128})) == 128 and rnn_critic_of(_cfg(**{KEY: True, RNN: 256})) == 256
    assert rnn_critic_of(_cfg(**{KEY: True, RNN: 128, "runner.num_env_mini_batches": 4, "algorithm.rnn_type": "gru"})) == 128


def test_rnn_critic_errors_name_the_keys():
    from booster_gym_amd.utils.runner import rnn_critic_of

    for bad in (1, 0, "true", 128, 1.0, [True]):
        with pytest.raises(ValueError, match=r"algorithm\.rnn_critic"):
            rnn_critic_of(_cfg(**{KEY: bad, RNN: 128}))
    for without in ({}, {RNN: 0}, {RNN: None}):  # true without a cell in front of the actor: both keys named
        with pytest.raises(ValueError, match=r"algorithm\.rnn_critic.*algorithm\.rnn_hidden_size"):
            rnn_critic_of(_cfg(**{KEY: True, **without}))
    # everything a recurrent actor does not compose with is rnn_hidden_size_of's to refuse, in its words
    with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*algorithm\.symmetry_loss"):
        rnn_critic_of(_cfg(**{KEY: True, RNN: 128, "algorithm.symmetry_loss": True}))
    with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*rank"):
        rnn_critic_of(_cfg(**{KEY: True, RNN: 128}), world_size=2)
    with pytest.raises(ValueError, match=r"algorithm\.rnn_type"):
        rnn_critic_of(_cfg(**{KEY: True, RNN: 128, "algorithm.rnn_type": "lstm"}))


def test_rnn_hidden_size_of_is_unaffected_by_the_key():
    from booster_gym_amd.utils.runner import rnn_hidden_size_of

    for value in (True, False, None, "nonsense"):
        assert rnn_hidden_size_of(_cfg(**{KEY: value, RNN: 128})) == 128 and rnn_hidden_size_of(_cfg(**{KEY: value})) == 0


def test_shipped_config_lists_the_key_in_no_mapping():
    import yaml

    path = os.path.join(ROOT, "booster_gym_amd", "envs", "T1.yaml")
    text = open(path).read()

    def keys(node):
        if isinstance(node, dict):
            for k, v in node.items():
                yield k
                yield from keys(v)

    assert "rnn_critic" not in set(keys(yaml.safe_load(text))) and "rnn_critic" not in _cfg()["algorithm"]
    assert any("rnn_critic" in line and line.lstrip().startswith("#") for line in text.splitlines())  # (the comment block describes it)


@pytest.mark.parametrize("H", [128, 256])
def test_model_with_a_critic_cell(H):
    from booster_gym_amd.utils.model import ActorCritic

    m = ActorCritic(12, 47, 14, memory_hidden=H, critic_memory_hidden=H)
    names = [k for k, _ in m.named_parameters()]
    assert names == [k for k, _ in ActorCritic(12, 47, 14, memory_hidden=H).named_parameters()] + [f"critic_memory.{w}" for w in CELL]
    assert isinstance(m.critic_memory, torch.nn.GRUCell) and (m.critic_memory.input_size, m.critic_memory.hidden_size) == (47 + 14, H)
    assert m.critic[0].in_features == H and m.actor[0].in_features == H and m.memory.input_size == 47
    assert [id(p) for p in m.ppo_parameters()] == [id(p) for p in m.parameters()]
    with pytest.raises(ValueError, match=r"est_value.*algorithm\.rnn_critic"):
        m.est_value(torch.zeros(3, 47), torch.zeros(3, 14))
    with pytest.raises(ValueError, match="act"):
        m.act(torch.zeros(3, 47))
    wide = ActorCritic(12, 47, 20, memory_hidden=H, critic_memory_hidden=H)  # env.privileged_extras: the cell reads the wider row
    assert wide.critic_memory.input_size == 67 and wide.critic[0].in_features == H


def test_parameter_order_with_the_key_off_is_todays():
    from booster_gym_amd.utils.model import ActorCritic

    for kw in ({}, {"critic_memory_hidden": 0}, {"critic_memory_hidden": None}):
        m = ActorCritic(12, 47, 14, **kw)
        assert [k for k, _ in m.named_parameters()] == TODAY and not hasattr(m, "critic_memory") and m.critic[0].in_features == 61
        assert m.est_value(torch.zeros(3, 47), torch.zeros(3, 14)).shape == (3,)
    m = ActorCritic(12, 47, 14, memory_hidden=128)
    assert [k for k, _ in m.named_parameters()] == TODAY + [f"memory.{w}" for w in CELL] and m.critic[0].in_features == 61
    # ... and the same draws: the key off changes no initial weight
    torch.manual_seed(3)
    a = ActorCritic(12, 47, 14, memory_hidden=128).state_dict()
    torch.manual_seed(3)
    b = ActorCritic(12, 47, 14, memory_hidden=128, critic_memory_hidden=0).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_checkpoint_rule_on_plain_dicts():
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import checkpoint_memory_overrides

    for H in (128, 256):
        both = {"model": ActorCritic(12, 47, 14, memory_hidden=H, critic_memory_hidden=H).state_dict(), "optimizer": {}, "curriculum": None}
        assert checkpoint_memory_overrides(both) == {RNN: H, KEY: True}
        actor_only = {"model": ActorCritic(12, 47, 14, memory_hidden=H).state_dict(), "optimizer": {}}
        assert checkpoint_memory_overrides(actor_only) == {RNN: H}  # today's checkpoints: unchanged
        student = {"model": actor_only["model"], "distillation": {"teacher": "t.pth", "student_memory": H}}
        assert checkpoint_memory_overrides(student) is None
    assert checkpoint_memory_overrides({"model": ActorCritic(12, 47, 14).state_dict()}) is None and checkpoint_memory_overrides({}) is None


def test_plan_of_an_update_with_both_cells():
    """Both trunks run the per-layer kernels, the values come from the stored activations, the tail is the separate launches; BG_GRU_GROUP resolves
    into the plan's gru_group; critic_memory = 0 is today's plan, field by field."""
    from booster_gym_amd.utils.runner import plan_update

    sw = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
              defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
    actor = ((128, 256, 128, 128, 12), 128)
    today = plan_update(((61, 256, 256, 128, 1), 64), actor, 24 * 4096, memory=128, **sw)
    assert plan_update(((61, 256, 256, 128, 1), 64), actor, 24 * 4096, memory=128, critic_memory=0, gru_group=1, **sw) == today and not today.gru_group
    for group in (2, 1, 0):
        plan = plan_update(((128, 256, 256, 128, 1), 128), actor, 24 * 1024, memory=128, critic_memory=128, gru_group=group, **sw)
        assert (plan.critic.fwd, plan.critic.bwd, plan.actor.fwd, plan.actor.bwd) == ("layer",) * 4 and all(plan.critic.grouped[:-1])
        assert not plan.chain_values and not plan.one_stream and not plan.one_tail and not plan.ahead and plan.defer and plan.fused_gae and plan.wgrad == 0
        assert plan.gru_group == group
    with pytest.raises(ValueError, match=r"algorithm\.rnn_critic.*algorithm\.rnn_hidden_size"):
        plan_update(((128, 256, 256, 128, 1), 128), ((47, 256, 128, 128, 12), 64), 24 * 4096, critic_memory=128, **sw)
    with pytest.raises(ValueError, match=r"algorithm\.rnn_critic.*layer kernels"):  # (a critic layer outside the grouped weight gradients' widths)
        plan_update(((128, 256, 200, 128, 1), 128), ((128, 256, 128, 128, 12), 128), 24 * 4096, memory=128, critic_memory=128, **sw)


def test_cell_trainer_shapes():
    """The padded input width is a parameter (pad_input of the critic's row), and the forward pass may walk one step more than the backward pass."""
    from types import SimpleNamespace

    from booster_gym_amd.utils.model import GRUTrainer, pad_input

    assert [pad_input(w) for w in (61, 67, 248, 435)] == [64, 128, 256, 512]
    cell = torch.nn.GRUCell(67, 128)
    trunk = SimpleNamespace()
    tr = GRUTrainer(cell, trunk, 5, 40, bias_partial=True, kin=pad_input(67), extra_steps=1)
    assert (tr.kin, tr.T, tr.TF, tr.B, tr.BF) == (128, 5, 6, 200, 240)
    assert tr.gi.shape == (240, 384) and tr.h.shape == (240, 128) and tr.gates.shape == (240, 512) and tr.resets.shape == (6, 40)
    assert tr.dgi.shape == (200, 384) and tr.dh_ext.shape == (200, 128) and tr.next_state.shape == (40, 128) and bool((tr.next_state == 0).all())
    today = GRUTrainer(torch.nn.GRUCell(47, 128), trunk, 5, 40)
    assert (today.kin, today.TF, today.BF) == (GRUTrainer.KIN, 5, 200) and today.next_state is None and today.resets.shape == (5, 40)
    with pytest.raises(ValueError, match="GRUTrainer"):
        GRUTrainer(cell, trunk, 5, 40, kin=64)  # narrower than the cell's input
    # the reset flags of a forward pass of T + 1 steps: row t = the done flags of step t - 1, every one of them
    dones = torch.rand(5, 40) < 0.3
    tr.rollout_begin(torch.ones(40, 128), torch.ones(40, dtype=torch.uint8))
    tr.rollout_end(dones)
    assert torch.equal(tr.resets[1:].bool(), dones) and bool(tr.resets[0].all()) and bool((tr.h0 == 1).all())
    tr.h.copy_(torch.arange(240.0).view(240, 1).expand(240, 128))
    tr.carry_state()
    assert torch.equal(tr.next_state, tr.h[160:200])  # the output of step T - 1


def test_group_entry_points_are_declared_bound_and_exported():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    for name, struct, cls in (("bg_gru_sequence_forward_group", "bg_gru_forward_problem", _lib.GruForwardProblem),
                              ("bg_gru_sequence_backward_group", "bg_gru_backward_problem", _lib.GruBackwardProblem)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")) == 4
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        fields = [f.strip().split()[-1].lstrip("*") for part in re.sub(r"/\*.*?\*/", "", body).split(";") for f in part.split(",") if f.strip()]
        assert fields == [f for f, _ in cls._fields_], (fields, cls._fields_)  # the single entry points' arguments, by their names
    assert re.search(r"#define BG_GRU_GROUP_MAX 4\b", header)
    # the argument errors that need no device: before any launch, naming the entry point
    one = (_lib.GruForwardProblem * 1)()
    for args, rc in (((None, 1, 128), -1), ((one, 0, 128), -1), ((one, 5, 128), -1), ((one, 1, 64), -4), ((one, 1, 128), -1)):
        assert lib.bg_gru_sequence_forward_group(*args, None) == rc and b"bg_gru_sequence_forward_group" in lib.bg_last_error(), (args, lib.bg_last_error())
    one = (_lib.GruBackwardProblem * 1)()
    for args, rc in (((None, 1, 128), -1), ((one, 0, 128), -1), ((one, 5, 128), -1), ((one, 1, 512), -4), ((one, 1, 256), -1)):
        assert lib.bg_gru_sequence_backward_group(*args, None) == rc and b"bg_gru_sequence_backward_group" in lib.bg_last_error(), (args, lib.bg_last_error())
