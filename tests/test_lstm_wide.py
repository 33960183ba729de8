"""algorithm.rnn_hidden_size: 512 (legged_gym's width) without a GPU: the width is the LSTM's alone in the three functions that read it, LSTMTrainer
sizes its buffers from it, and the fp32 torch twin of tests/parity_util.lstm_sequence_case at H = 512 stays within a tenth of the project's two bounds
(2e-5 on forward quantities, 1e-4 of the largest entry on gradients) at the cases of tests/test_gpu_lstm_wide.py, so those cases use the bounds as
they are (K is twice H = 256's; measured here: forward quantities at most 5.0e-7 = 2.5 % of the bound, gradients at most 4.9e-7 of the largest entry = 0.5 %)."""
import pytest
import torch

from parity_util import lstm_sequence_case
from test_gpu_distill_memory import _bound, _grad_bound

WIDE_CASES = {"1x1": (1, 1, 1.0, 0.2, True, True), "2x16": (2, 16, 1.0, 0.2, True, True), "3x17": (3, 17, 1.0, 0.2, True, True),
              "5x40": (5, 40, 1.0, 0.2, True, True), "5x40_scale8": (5, 40, 8.0, 0.2, True, True), "5x40_null": (5, 40, 1.0, None, False, False)}


@pytest.mark.parametrize("cell, key, want", [("lstm", "rnn_hidden_size", 512), ("lstm", "actor_memory", 512), ("gru", "rnn_hidden_size", None),
                                             (None, "rnn_hidden_size", None), ("gru", "actor_memory", None), (None, "actor_memory", None)])
def test_the_width_is_the_lstm_cells(cell, key, want):
    from booster_gym_amd.utils.runner import actor_memory_of, rnn_cell_of, rnn_hidden_size_of

    cfg = {"algorithm": {key: 512, **({} if cell is None else {"rnn_cell": cell})}}
    read = rnn_hidden_size_of if key == "rnn_hidden_size" else actor_memory_of
    if want is None:
        with pytest.raises(ValueError, match=rf"algorithm\.{key}.*LSTM"):
            read(cfg)
    else:
        assert read(cfg) == want
        assert rnn_cell_of(cfg) == ("lstm" if key == "rnn_hidden_size" else "gru")  # (the re-entry key alone names no training cell)


def test_lstm_trainer_sizes_its_buffers_from_the_width():
    from booster_gym_amd.utils.model import ActorCritic, LSTMTrainer, MLPTrainer

    T, N, H = 5, 40, 512
    m = ActorCritic(12, 47, 14, memory_hidden=H, memory_cell="lstm")
    tr = LSTMTrainer(m.memory, MLPTrainer(m.actor), T, N)
    B = T * N
    assert tuple(m.actor[0].weight.shape) == (256, H) and tuple(m.memory.weight_hh.shape) == (4 * H, H)
    assert tr.gi.shape == (B, 4 * H) and tr.dg.shape == (B, 4 * H) and tr.gates.shape == (B, 5 * H) and tr.h0.shape == (2, N, H)
    assert all(x.shape == (B, H) for x in (tr.h_prev, tr.c_prev, tr.h, tr.c, tr.dh_ext)) and tr._cs.numel() == 2 * 4 * H  # two records of 128 rows


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_the_twin_stays_within_a_tenth_of_the_bounds_at_512(name):
    T, N, scale, reset, h0, c0 = WIDE_CASES[name]
    c = lstm_sequence_case(T, N, 512, scale, reset, h0, c0)
    ref, twin = c["ref"], c["twin"]
    tenfold = lambda k: ref[k] + 10.0 * (twin[k].double() - ref[k])
    for k in ("h_prev", "c_prev", "h", "c", "gates"):
        _bound(tenfold(k), ref[k], f"{name} {k}, ten times the twin's error")
    for k in ("dg", "dh0", "dc0"):
        if ref[k].abs().max().item() == 0.0:  # (the one row enters step 0 behind a reset)
            assert torch.all(twin[k] == 0.0)
        else:
            _grad_bound(tenfold(k), ref[k], f"{name} {k}, ten times the twin's error")
