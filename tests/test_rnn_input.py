"""algorithm.rnn_input without a GPU: what rnn_input_of accepts and refuses, the two refusals of rnn_hidden_size_of that "row" lifts, and the key a
checkpoint's shapes name."""
import pytest
import torch

ON = {"algorithm.rnn_hidden_size": 128}
ROW = {**ON, "algorithm.rnn_input": "row"}
STACK = {"env.frame_stack": 2, "env.num_observations": 94}
SCAN = {"terrain.actor_heights": True, "terrain.measure_heights": True, "env.num_observations": 234, "env.num_privileged_obs": 201}


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", over)


@pytest.mark.parametrize("over, want", [
    ({}, 47), ({"algorithm.rnn_input": "row"}, 47),  # without a recurrent actor the key is not read
    (ON, 47), ({**ON, "algorithm.rnn_input": None}, 47), ({**ON, "algorithm.rnn_input": "observation"}, 47),
    (ROW, 47), ({**ROW, **STACK}, 94), ({**ROW, **SCAN}, 234), ({**ROW, **SCAN, "algorithm.rnn_cell": "lstm", "algorithm.rnn_hidden_size": 512}, 234),
    ({"algorithm.actor_memory": 256, "algorithm.rnn_input": "row", **STACK}, 94),  # a checkpoint re-entering to play
    ({**ON, "algorithm.rnn_input": "rows"}, r"algorithm\.rnn_input.*'rows'"), ({**ON, "algorithm.rnn_input": True}, r"algorithm\.rnn_input.*True"),
    ({**ROW, "env.frame_stack": 6, "env.num_observations": 282}, r"algorithm\.rnn_input.*282"),  # over the 256 columns of the cell's input tile
    ({**ON, **STACK}, r"algorithm\.rnn_hidden_size.*env\.frame_stack"), ({**ON, **SCAN}, r"algorithm\.rnn_hidden_size.*terrain\.actor_heights"),
    ({**ROW, **STACK, "algorithm.symmetry_loss": True}, r"algorithm\.rnn_hidden_size.*algorithm\.symmetry_loss"),  # the other refusals stay
    ({**ROW, **STACK, "estimator.enabled": True}, r"algorithm\.rnn_hidden_size.*estimator\.enabled"),
])
def test_rnn_input_of(over, want):
    from booster_gym_amd.utils.runner import rnn_cell_of, rnn_hidden_size_of, rnn_input_of

    cfg = _cfg(**over)
    if isinstance(want, int):
        assert rnn_input_of(cfg) == want
        assert rnn_hidden_size_of(cfg) == over.get("algorithm.rnn_hidden_size", 0) and rnn_cell_of(cfg) == over.get("algorithm.rnn_cell", "gru")
    else:
        with pytest.raises(ValueError, match=want):
            rnn_input_of(cfg)


@pytest.mark.parametrize("rows, K, critic, want", [
    (3, 47, False, {"algorithm.rnn_hidden_size": 128}),
    (3, 94, False, {"algorithm.rnn_hidden_size": 128, "algorithm.rnn_input": "row"}),
    (4, 234, False, {"algorithm.rnn_hidden_size": 128, "algorithm.rnn_cell": "lstm", "algorithm.rnn_input": "row"}),
    (3, 94, True, {"algorithm.rnn_hidden_size": 128, "algorithm.rnn_critic": True, "algorithm.rnn_input": "row"}),
])
def test_the_override_is_read_from_the_checkpoints_shapes(rows, K, critic, want):
    from booster_gym_amd.utils.runner import checkpoint_memory_overrides

    sd = {"memory.weight_ih": torch.zeros(rows * 128, K), "memory.weight_hh": torch.zeros(rows * 128, 128)}
    if critic:
        sd["critic_memory.weight_hh"] = torch.zeros(384, 128)
    assert checkpoint_memory_overrides({"model": sd}) == want
    assert checkpoint_memory_overrides({"model": sd, "distillation": {}}) is None  # a student re-enters under its own overrides


def test_the_model_builds_the_cell_on_memory_input():
    from booster_gym_amd.utils.model import ActorCritic

    for cell, kind, gates in (("gru", torch.nn.GRUCell, 3), ("lstm", torch.nn.LSTMCell, 4)):
        m = ActorCritic(12, 94, 14, memory_hidden=128, memory_cell=cell, memory_input=94)
        assert isinstance(m.memory, kind) and tuple(m.memory.weight_ih.shape) == (gates * 128, 94) and m.actor[0].in_features == 128
        assert m.critic[0].in_features == 94 + 14
    with pytest.raises(ValueError, match="memory_input"):
        ActorCritic(12, 94, 14, memory_hidden=128, memory_input=95)
