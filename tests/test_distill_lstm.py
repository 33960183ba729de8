"""distillation.student_cell without a GPU: what student_cell_of accepts and refuses, an LSTM student's re-entry overrides, the new entry points."""
import os

import pytest
import torch

H, KEY, MEMORY = 128, "distillation.student_cell", "distillation.student_memory"
_cfg = lambda **section: {"env": {"frame_stack": 1}, "terrain": {}, "distillation": dict(section)}


@pytest.mark.parametrize("section, want", [
    ({}, "gru"), ({"student_cell": "lstm"}, "gru"), ({"student_memory": 0, "student_cell": 4}, "gru"),  # no memory: the key is not read, whatever it holds
    ({"student_memory": H}, "gru"), ({"student_memory": H, "student_cell": None}, "gru"), ({"student_memory": H, "student_cell": "gru"}, "gru"),
    ({"student_memory": H, "student_cell": "lstm"}, "lstm"), ({"student_memory": 256, "student_cell": "lstm"}, "lstm"),
    ({"student_memory": H, "student_cell": "LSTM"}, (KEY,)), ({"student_memory": H, "student_cell": 4}, (KEY,)),
    ({"student_memory": 64, "student_cell": "lstm"}, (MEMORY,)),  # student_memory_of's own refusals, unchanged
    ({"student_memory": H, "student_cell": "lstm", "symmetric_coef": 0.5}, (MEMORY, "distillation.symmetric_coef")),
    ({"student_memory": H, "student_cell": "lstm", "student_frame_stack": 3}, (MEMORY, "distillation.student_frame_stack")),
])
def test_student_cell_of(section, want):
    from booster_gym_amd.utils.distill import student_cell_of
    if isinstance(want, str):
        assert student_cell_of(_cfg(**section)) == want
    else:
        with pytest.raises(ValueError) as e:
            student_cell_of(_cfg(**section))
        assert all(key in str(e.value) for key in want), str(e.value)


@pytest.mark.parametrize("cell, gates", [("gru", 3), ("lstm", 4), (None, 3)])
def test_student_overrides_name_the_cell(cell, gates):
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides, student_overrides
    want = {"terrain.actor_heights": False, "env.num_observations": 47, "algorithm.actor_memory": H, **({"algorithm.rnn_cell": "lstm"} if cell == "lstm" else {})}
    assert student_overrides(47, None, H, None, cell) == want == student_cfg_overrides(_cfg(student_memory=H, student_cell=cell))
    ck = {"model": {"memory.weight_ih": torch.zeros(gates * H, 47), "memory.weight_hh": torch.zeros(gates * H, H)}, "distillation": {"student_memory": H}}
    assert checkpoint_student_overrides(ck) == want and "algorithm.rnn_cell" not in student_overrides(47, None, 0, None, "lstm")  # (no memory, no cell)


def test_entry_points_are_declared_bound_and_built():
    from booster_gym_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "booster_gym_amd.h")).read()
    for name, nargs in (("bg_distill_act_lstm", 21), ("bg_distill_act_lstm_own", 23)):
        assert f"int {name}(" in header and name in _lib.SYMBOLS and len(getattr(_lib.load(), name).argtypes) == nargs
