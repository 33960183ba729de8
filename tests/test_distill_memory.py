"""distillation.student_memory without a GPU: the key's rules (every error names its key), the shipped default, the parameter order of a model with
and without memory, the overrides a recurrent student's checkpoint re-enters the tools under, the ABI of the four new entry points, and the exported
stateful module against a torch.nn.GRUCell + MLP loop."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("bg_actor_sample_gru", "bg_distill_act_gru", "bg_gru_sequence_forward", "bg_gru_sequence_backward")


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_privileged_obs": 201, "env.num_observations": 234}
    ov.update(over)
    return load_cfg("T1", ov)


def test_shipped_default_is_off_and_the_accepted_values():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import DEFAULTS, distillation_cfg, student_cfg_overrides, student_memory_of

    shipped = load_cfg("T1")
    assert shipped["distillation"] == DEFAULTS and DEFAULTS["student_memory"] == 0
    assert "actor_memory" not in shipped["algorithm"]
    assert student_memory_of(_cfg()) == 0
    cfg = _cfg()
    del cfg["distillation"]["student_memory"]
    assert student_memory_of(cfg) == 0
    for H in (128, 256):
        cfg = _cfg(**{"distillation.student_memory": H})
        assert student_memory_of(cfg) == H and distillation_cfg(cfg) == distillation_cfg(_cfg())
        assert student_cfg_overrides(cfg) == {"terrain.actor_heights": False, "env.num_observations": 47, "algorithm.actor_memory": H}
    assert student_cfg_overrides(_cfg()) == {"terrain.actor_heights": False, "env.num_observations": 47}


@pytest.mark.parametrize("over", [
    {"distillation.student_memory": 64}, {"distillation.student_memory": 512}, {"distillation.student_memory": -128},
    {"distillation.student_memory": 128.0}, {"distillation.student_memory": True}, {"distillation.student_memory": "128"},
    {"distillation.student_memory": 128, "env.frame_stack": 2, "env.num_observations": 281},
    {"distillation.student_memory": 256, "distillation.student_frame_stack": 3},
    {"distillation.student_memory": 128, "distillation.symmetric_coef": 0.5},
])
def test_every_config_error_names_the_key(over):
    from booster_gym_amd.utils.distill import distillation_cfg

    with pytest.raises(ValueError, match=r"distillation\.student_memory"):
        distillation_cfg(_cfg(**over))


def test_the_sections_other_exclusions_stay():
    from booster_gym_amd.utils.distill import distillation_cfg

    for over, match in (({"algorithm.empirical_normalization": True}, r"algorithm\.empirical_normalization"), ({"estimator.enabled": True}, r"estimator\.enabled")):
        with pytest.raises(ValueError, match=match):
            distillation_cfg(_cfg(**{"distillation.student_memory": 128}, **over))
    with pytest.raises(ValueError, match=r"one rank"):
        distillation_cfg(_cfg(**{"distillation.student_memory": 128}), world_size=2)
    # off: the keys a recurrent student excludes are legal
    distillation_cfg(_cfg(**{"distillation.student_frame_stack": 3, "distillation.symmetric_coef": 0.5}))


def test_actor_memory_key_of_the_runner():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import actor_memory_of

    assert actor_memory_of(load_cfg("T1")) == 0
    assert actor_memory_of(load_cfg("T1", {"algorithm.actor_memory": 256})) == 256
    for bad in (64, True, 128.0, "128"):
        with pytest.raises(ValueError, match=r"algorithm\.actor_memory"):
            actor_memory_of(load_cfg("T1", {"algorithm.actor_memory": bad}))
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory"):
        actor_memory_of(load_cfg("T1", {"algorithm.actor_memory": 128, "estimator.enabled": True}))


def test_parameter_names_and_order():
    from booster_gym_amd.utils.model import ActorCritic

    today = ["logstd"] + [f"{net}.{i}.{p}" for net in ("critic", "actor") for i in (0, 2, 4, 6) for p in ("weight", "bias")]
    torch.manual_seed(3)
    plain = ActorCritic(12, 47, 14)
    torch.manual_seed(3)
    off = ActorCritic(12, 47, 14, memory_hidden=0)
    assert [n for n, _ in plain.named_parameters()] == today == [n for n, _ in off.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(plain.parameters(), off.parameters())) and not hasattr(off, "memory")
    assert list(off.state_dict()) == list(plain.state_dict())
    mem = ActorCritic(12, 47, 14, memory_hidden=128)
    names = [n for n, _ in mem.named_parameters()]
    assert names == today + ["memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"]
    assert isinstance(mem.memory, torch.nn.GRUCell) and (mem.memory.input_size, mem.memory.hidden_size) == (47, 128)
    assert mem.actor[0].in_features == 128 and tuple(mem.memory.weight_ih.shape) == (384, 47) and tuple(mem.memory.weight_hh.shape) == (384, 128)
    est = ActorCritic(12, 47, 14, estimator_hidden=(256, 128), estimator_cols=4)
    assert [n for n, _ in est.named_parameters()][: len(today)] == today
    with pytest.raises(ValueError, match="memory_hidden"):
        ActorCritic(12, 47, 14, estimator_hidden=(256, 128), estimator_cols=4, memory_hidden=128)
    with pytest.raises(ValueError, match="stateful"):
        mem.act(torch.zeros(2, 47))


def test_overrides_from_a_checkpoint_dict():
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_overrides
    from booster_gym_amd.utils.model import ActorCritic

    assert student_overrides(47) == {"terrain.actor_heights": False, "env.num_observations": 47}
    assert student_overrides(141, 3) == {"terrain.actor_heights": False, "env.frame_stack": 3, "env.num_observations": 141}
    assert student_overrides(47, None, 0) == student_overrides(47, None, None) == student_overrides(47)
    assert student_overrides(47, None, 256) == {"terrain.actor_heights": False, "env.num_observations": 47, "algorithm.actor_memory": 256}
    mem = ActorCritic(12, 47, 201, memory_hidden=256)
    ck = {"model": mem.state_dict(), "distillation": {"teacher": "t.pth", "iteration": 3, "loss": 0.1, "student_memory": 256}}
    assert checkpoint_student_overrides(ck) == {"terrain.actor_heights": False, "env.num_observations": 47, "algorithm.actor_memory": 256}
    plain = {"model": ActorCritic(12, 47, 201).state_dict(), "distillation": {"teacher": "t.pth", "iteration": 3, "loss": 0.1}}
    assert checkpoint_student_overrides(plain) == {"terrain.actor_heights": False, "env.num_observations": 47}
    assert checkpoint_student_overrides({"model": mem.state_dict()}) is None


def test_play_oracle_refuses_a_recurrent_student(tmp_path):
    import importlib.util

    from booster_gym_amd.utils.model import ActorCritic

    spec = importlib.util.spec_from_file_location("play_oracle", os.path.join(ROOT, "tools", "play_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "student.pth")
    torch.save({"model": ActorCritic(12, 47, 14, memory_hidden=128).state_dict()}, path)
    with pytest.raises(ValueError, match="recurrent student"):
        mod.load_actor(path)


def test_entry_points_are_declared_bound_and_exported():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
    assert "typedef struct bg_gru_desc" in header and [f[0] for f in _lib.GruDesc._fields_] == ["W_ih", "W_hh", "b_ih", "b_hh", "in_", "hidden"]


def test_recurrent_actor_scripts_and_matches_a_grucell_loop():
    from booster_gym_amd.utils.model import ActorCritic, RecurrentActor

    torch.manual_seed(11)
    m = ActorCritic(12, 47, 14, memory_hidden=128)
    mod = torch.jit.script(RecurrentActor(m.memory, m.actor))
    assert hasattr(mod, "reset")
    xs = torch.randn(6, 5, 47)

    def loop(x):
        h, out = torch.zeros(x.shape[1], 128), []
        with torch.no_grad():
            for t in range(x.shape[0]):
                h = m.memory(x[t], h)
                out.append(m.actor(h))
        return torch.stack(out)

    ref = loop(xs)
    got = torch.stack([mod(xs[t]) for t in range(6)])
    assert (got - ref).abs().max().item() <= 1e-6 and tuple(got.shape) == (6, 5, 12)
    assert (mod(xs[0]) - ref[0]).abs().max().item() > 1e-4  # (the state carries: a seventh step is not the first)
    mod.reset()
    assert torch.all(mod.h == 0) and (torch.stack([mod(xs[t]) for t in range(6)]) - ref).abs().max().item() <= 1e-6
    ys = torch.randn(2, 3, 47)  # another B: the state starts again at zero
    assert (torch.stack([mod(ys[t]) for t in range(2)]) - loop(ys)).abs().max().item() <= 1e-6 and tuple(mod.h.shape) == (3, 128)
