"""Teacher-student distillation without a GPU: the `distillation:` section's rules (every error names its key), the shipped section, the overrides a
student checkpoint re-enters the tools under, and the C ABI of the three new entry points (declared, exported, bound with the header's argument
counts; argument errors raised on the host before any launch)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("bg_distill_act", "bg_distill_head", "bg_distill_head_partial")


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_privileged_obs": 201, "env.num_observations": 234}
    ov.update(over)
    return load_cfg("T1", ov)


def test_shipped_section_is_accepted_with_actor_heights_on():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import DEFAULTS, distillation_cfg, student_cfg_overrides

    assert load_cfg("T1")["distillation"] == DEFAULTS  # (the shipped yaml names every key, at its default)
    d = distillation_cfg(_cfg())
    assert d == (None, (256, 128, 128), 5, 1.0e-3, 1.0, 0.1)
    d = distillation_cfg(_cfg(**{"distillation": {"teacher_checkpoint": "a.pth", "student_hidden": [512, 128]}}))  # absent keys: the defaults
    assert d.teacher_checkpoint == "a.pth" and d.student_hidden == (512, 128) and d.num_epochs == 5 and d.student_noise_std == 0.1
    assert student_cfg_overrides(_cfg()) == {"terrain.actor_heights": False, "env.num_observations": 47}
    assert student_cfg_overrides(_cfg(**{"env.frame_stack": 2})) == {"terrain.actor_heights": False, "env.num_observations": 94}


@pytest.mark.parametrize("over,match", [
    ({"terrain.actor_heights": False}, r"distillation.*terrain\.actor_heights"),
    ({"terrain.actor_heights": False, "terrain.measure_heights": False}, r"distillation.*terrain\.actor_heights"),
    ({"distillation.learning_rate": 0.0}, r"distillation\.learning_rate"),
    ({"distillation.learning_rate": -1.0e-3}, r"distillation\.learning_rate"),
    ({"distillation.learning_rate": "fast"}, r"distillation\.learning_rate"),
    ({"distillation.student_noise_std": 0.0}, r"distillation\.student_noise_std"),
    ({"distillation.student_noise_std": float("nan")}, r"distillation\.student_noise_std"),
    ({"distillation.max_grad_norm": -1.0}, r"distillation\.max_grad_norm"),
    ({"distillation.num_epochs": 0}, r"distillation\.num_epochs"),
    ({"distillation.num_epochs": 2.5}, r"distillation\.num_epochs"),
    ({"distillation.num_epochs": True}, r"distillation\.num_epochs"),
    ({"distillation.student_hidden": [256, 64]}, r"distillation\.student_hidden"),
    ({"distillation.student_hidden": [256, 128, 256]}, r"distillation\.student_hidden"),
    ({"distillation.student_hidden": [128]}, r"distillation\.student_hidden"),
    ({"distillation.student_hidden": 256}, r"distillation\.student_hidden"),
    ({"distillation.teacher_checkpoint": 7}, r"distillation\.teacher_checkpoint"),
    ({"distillation.epochs": 3}, r"distillation\.epochs"),
    ({"algorithm.empirical_normalization": True}, r"algorithm\.empirical_normalization.*not supported with distillation"),
])
def test_every_config_error_names_its_key(over, match):
    from booster_gym_amd.utils.distill import distillation_cfg

    with pytest.raises(ValueError, match=match):
        distillation_cfg(_cfg(**over))


def test_section_absent_and_more_than_one_rank_are_value_errors():
    from booster_gym_amd.utils.distill import distillation_cfg

    cfg = _cfg()
    del cfg["distillation"]
    with pytest.raises(ValueError, match=r"distillation.*unavailable"):
        distillation_cfg(cfg)
    with pytest.raises(ValueError, match=r"distillation.*one rank.*WORLD_SIZE = 2"):
        distillation_cfg(_cfg(), world_size=2)
    assert distillation_cfg(_cfg(), world_size=1).num_epochs == 5


def test_nothing_but_the_distiller_reads_the_section():
    """The section is inert for PPO: a config without it resolves the same widths, sizes and update plan inputs."""
    from booster_gym_amd.envs.t1 import check_env_sizes
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import hidden_widths, mini_batches, symmetry_loss

    a, b = load_cfg("T1"), load_cfg("T1")
    del b["distillation"]
    for cfg in (a, b):
        check_env_sizes(cfg, 0)
    assert hidden_widths(a) == hidden_widths(b) and mini_batches(a) == mini_batches(b) and symmetry_loss(a) == symmetry_loss(b)
    a.pop("distillation")
    assert a == b


def _header_arg_count(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_library_declares_exports_and_binds_the_entry_points_with_the_headers_argument_counts():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    want = {"bg_distill_act": 15, "bg_distill_head": 13, "bg_distill_head_partial": 14}
    for s in ENTRY_POINTS:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        n = _header_arg_count(header, s)
        assert n == want[s] and len(getattr(lib, s).argtypes) == n, (s, n, len(getattr(lib, s).argtypes))
    assert lib.bg_distill_head_partial.argtypes[-2] == C.POINTER(_lib.ReduceProblem)
    assert lib.bg_distill_act.argtypes[4] == lib.bg_distill_act.argtypes[6] == C.POINTER(_lib.MlpLayerDesc)


def test_abi_argument_errors_without_gpu():
    """The entry points check their arguments on the host before any launch."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    f = (C.c_float * 4096)()
    d = (C.c_double * 4)()
    fin = _lib.ReduceProblem()
    head = lambda B=4, h=f, W=f, b=f, t=f, g=f, gW=f, gb=f, gbh=f, st=d, sc=f: lib.bg_distill_head(B, h, W, b, t, None, g, gW, gb, gbh, st, sc, None)
    for kw in (dict(B=0), dict(h=None), dict(W=None), dict(b=None), dict(t=None), dict(g=None), dict(gW=None), dict(gb=None), dict(gbh=None), dict(st=None),
               dict(sc=None)):
        assert head(**kw) == -1 and b"bg_distill_head" in lib.bg_last_error(), kw
    assert lib.bg_distill_head_partial(4, f, f, f, f, None, f, f, f, f, d, f, None, None) == -1 and b"bg_distill_head_partial" in lib.bg_last_error()
    assert lib.bg_distill_head_partial(0, f, f, f, f, None, f, f, f, f, d, f, fin, None) == -1 and b"bg_distill_head_partial" in lib.bg_last_error()

    p16 = (C.addressof(f) + 15) & ~15  # (weight matrices after the first must be 16-byte aligned: its own argument error)

    def net(k_in, hidden=(128, 128)):
        w = (k_in,) + tuple(hidden) + (12,)
        return (_lib.MlpLayerDesc * (len(w) - 1))(*[_lib.MlpLayerDesc(p16, p16, w[i], w[i + 1]) for i in range(len(w) - 1)])

    act = lambda N=4, obs=f, stride=234, s=net(47), t=net(234), ns=3, nt=3, scan=187, ls=f, a=f, tm=f: lib.bg_distill_act(N, obs, stride, ns, s, nt, t, scan, ls, 0, 0, None,
                                                                                                                          a, tm, None)
    for kw in (dict(N=0), dict(obs=None), dict(s=None), dict(t=None), dict(ls=None), dict(a=None), dict(tm=None), dict(scan=-1), dict(scan=1025)):
        assert act(**kw) == -1 and b"bg_distill_act" in lib.bg_last_error(), kw
    for kw, word in ((dict(stride=235), b"obs_stride"),            # obs_stride is not the teacher's `in`
                     (dict(stride=47), b"obs_stride"),
                     (dict(s=net(48)), b"student"),                # a student `in` that is not 47 H
                     (dict(s=net(94)), b"student"),                # ... or another H than the teacher's
                     (dict(t=net(47 * 10 + 14), stride=484, scan=14, s=net(470)), b"teacher"),  # a teacher `in` above BG_ACTOR_MAX_INPUT
                     (dict(t=net(234, (128, 192))), b"teacher"),   # width rules per network
                     (dict(s=net(47, (128, 64))), b"student"),
                     (dict(ns=2), b"student"), (dict(nt=6), b"teacher")):
        assert act(**kw) == -4 and word in lib.bg_last_error(), (kw, lib.bg_last_error())
