"""algorithm.rnn_cell without a GPU: what rnn_cell_of accepts and refuses, and the cell a checkpoint's shapes name."""
import pytest
import torch

H = 128
ON = {"rnn_hidden_size": H}


@pytest.mark.parametrize("alg, runner, want", [
    ({}, {}, "gru"),                                                     # no recurrent actor: the key is not read
    ({"rnn_cell": "lstm"}, {}, "gru"),                                   # ... whatever it holds
    (ON, {}, "gru"),
    ({**ON, "rnn_cell": None}, {}, "gru"),
    ({**ON, "rnn_cell": "gru", "rnn_type": "gru"}, {}, "gru"),
    ({**ON, "rnn_cell": "lstm"}, {}, "lstm"),
    ({**ON, "rnn_cell": "lstm"}, {"num_env_mini_batches": 1}, "lstm"),
    ({**ON, "rnn_cell": "LSTM"}, {}, ("algorithm.rnn_cell",)),
    ({**ON, "rnn_cell": 4}, {}, ("algorithm.rnn_cell",)),
    ({**ON, "rnn_cell": "lstm", "rnn_type": "gru"}, {}, ("algorithm.rnn_cell", "algorithm.rnn_type")),
    ({**ON, "rnn_cell": "lstm", "rnn_critic": True}, {}, ("algorithm.rnn_cell", "algorithm.rnn_critic")),
    ({**ON, "rnn_cell": "lstm"}, {"num_env_mini_batches": 2}, ("algorithm.rnn_cell", "runner.num_env_mini_batches")),
    ({**ON, "rnn_cell": "lstm", "rnn_type": "lstm"}, {}, ("algorithm.rnn_type", "algorithm.rnn_cell")),   # rnn_type keeps its rule, with the hint
    ({**ON, "rnn_cell": "lstm", "symmetry_loss": True}, {}, ("algorithm.rnn_hidden_size", "algorithm.symmetry_loss")),  # rnn_hidden_size_of's own
])
def test_rnn_cell_of(alg, runner, want):
    from booster_gym_amd.utils.runner import rnn_cell_of

    cfg = {"algorithm": dict(alg), "runner": dict(runner)}
    if isinstance(want, str):
        assert rnn_cell_of(cfg) == want
    else:
        with pytest.raises(ValueError) as e:
            rnn_cell_of(cfg)
        assert all(key in str(e.value) for key in want), str(e.value)


@pytest.mark.parametrize("gates, want", [(3, {"algorithm.rnn_hidden_size": H}), (4, {"algorithm.rnn_hidden_size": H, "algorithm.rnn_cell": "lstm"})])
def test_checkpoint_memory_overrides_read_the_cell_from_the_shapes(gates, want):
    from booster_gym_amd.utils.runner import checkpoint_memory_overrides

    assert checkpoint_memory_overrides({"model": {"memory.weight_hh": torch.zeros(gates * H, H)}}) == want
