"""distillation.symmetric_coef and distillation.teacher_action_prob / _iterations / _noise without a GPU: the four keys' rules (every error names its
key), the shipped section, the unchanged DistillCfg, the schedule of beta, the student's mirror map, and the C ABI of the three new entry points
(declared, exported, bound with the header's argument counts; argument errors raised on the host before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_privileged_obs": 201, "env.num_observations": 234}
    ov.update(over)
    return load_cfg("T1", ov)


def test_shipped_section_names_the_four_keys_at_their_defaults_and_the_cfg_tuple_is_unchanged():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import DEFAULTS, DistillCfg, distillation_cfg, symmetric_coef_of, teacher_action_of

    sec = load_cfg("T1")["distillation"]
    assert sec == DEFAULTS
    assert (sec["symmetric_coef"], sec["teacher_action_prob"], sec["teacher_action_iterations"], sec["teacher_action_noise"]) == (0.0, 0.0, 0, True)
    assert len(DistillCfg._fields) == 6 and distillation_cfg(_cfg()) == (None, (256, 128, 128), 5, 1.0e-3, 1.0, 0.1)
    assert symmetric_coef_of(_cfg()) == 0.0 and teacher_action_of(_cfg()) == (0.0, 0, True)
    cfg = _cfg()
    for k in ("symmetric_coef", "teacher_action_prob", "teacher_action_iterations", "teacher_action_noise"):
        del cfg["distillation"][k]  # the keys absent, as in a yaml written before they existed
    assert distillation_cfg(cfg) == (None, (256, 128, 128), 5, 1.0e-3, 1.0, 0.1) and symmetric_coef_of(cfg) == 0.0 and teacher_action_of(cfg) == (0.0, 0, True)
    on = _cfg(**{"distillation.symmetric_coef": 10, "distillation.teacher_action_prob": 1, "distillation.teacher_action_iterations": 50,
                 "distillation.teacher_action_noise": False})
    assert distillation_cfg(on) == (None, (256, 128, 128), 5, 1.0e-3, 1.0, 0.1)  # (the section accepts the keys; the tuple does not carry them)
    assert symmetric_coef_of(on) == 10.0 and teacher_action_of(on) == (1.0, 50, False)


@pytest.mark.parametrize("key,value", [
    ("symmetric_coef", -1.0), ("symmetric_coef", float("nan")), ("symmetric_coef", float("inf")), ("symmetric_coef", "big"), ("symmetric_coef", True),
    ("symmetric_coef", None),
    ("teacher_action_prob", -0.1), ("teacher_action_prob", 1.5), ("teacher_action_prob", float("nan")), ("teacher_action_prob", "half"),
    ("teacher_action_prob", True), ("teacher_action_prob", None),
    ("teacher_action_iterations", -1), ("teacher_action_iterations", 2.5), ("teacher_action_iterations", True), ("teacher_action_iterations", "ten"),
    ("teacher_action_iterations", None),
    ("teacher_action_noise", 1), ("teacher_action_noise", 0.0), ("teacher_action_noise", "yes"), ("teacher_action_noise", None),
])
def test_every_bad_value_of_the_four_keys_names_its_key(key, value):
    from booster_gym_amd.utils.distill import symmetric_coef_of, teacher_action_of

    cfg = _cfg(**{"distillation." + key: value})
    with pytest.raises(ValueError, match=r"distillation\." + key + r"\b"):
        symmetric_coef_of(cfg) if key == "symmetric_coef" else teacher_action_of(cfg)


def test_teacher_action_prob_schedule():
    from booster_gym_amd.utils.distill import teacher_action_prob_at

    assert teacher_action_prob_at(0.8, 10, 0) == 0.8
    assert teacher_action_prob_at(0.8, 10, 5) == 0.4
    assert teacher_action_prob_at(1.0, 2, 1) == 0.5
    assert teacher_action_prob_at(0.8, 10, 10) == 0.0 and teacher_action_prob_at(0.8, 10, 11) == 0.0 and teacher_action_prob_at(0.8, 10, 10 ** 6) == 0.0
    assert all(teacher_action_prob_at(0.3, 0, i) == 0.3 for i in (0, 1, 7, 10 ** 6))  # iterations = 0: constant
    assert all(teacher_action_prob_at(0.0, n, i) == 0.0 for n in (0, 5) for i in (0, 3, 9))
    betas = [teacher_action_prob_at(1.0, 7, i) for i in range(9)]
    assert betas == sorted(betas, reverse=True) and all(0.0 <= b <= 1.0 for b in betas)


def _default_pose(cfg, names):
    dja = cfg["init_state"]["default_joint_angles"]
    return np.array([([v for k, v in dja.items() if k != "default" and k in n] or [dja["default"]])[-1] for n in names], dtype=np.float32)


@pytest.mark.parametrize("frames", [1, 5])
def test_student_mirror_map_is_the_single_observations_map_tiled_over_the_frames(flat_model, frames):
    from booster_gym_amd.envs.mirror import mirror_maps, signed_permutation
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import student_mirror_maps

    axes = [int(a) for a in flat_model.joint_axis if int(a) != 0]
    q0 = _default_pose(load_cfg("T1", {}), flat_model.dof_names)
    src1, sign1, a1, s1 = mirror_maps(flat_model.dof_names, axes, q0, 47)
    src, sign, act_src, act_sign = student_mirror_maps(flat_model.dof_names, axes, q0, frames)
    assert len(src) == len(sign) == 47 * frames  # the student's row: no height scan behind the frames
    assert np.array_equal(act_src, a1) and np.array_equal(act_sign, s1)
    M = signed_permutation(src, sign)
    assert np.array_equal(M @ M, np.eye(47 * frames)) and np.array_equal(M, M.T)  # an involution
    for k in range(frames):
        assert np.array_equal(src[47 * k : 47 * (k + 1)] // 47, np.full(47, k))  # every frame maps to the same frame
        assert np.array_equal(src[47 * k : 47 * (k + 1)], src1 + 47 * k) and np.array_equal(sign[47 * k : 47 * (k + 1)], sign1)  # the 47-column map, tiled
    with pytest.raises(ValueError, match=r"no Left_\* / Right_\* joint pairs"):
        student_mirror_maps([f"Joint_{k}" for k in range(12)], axes, np.zeros(12), frames)


def _header_arg_count(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_library_declares_exports_and_binds_the_new_entry_points():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    want = {"bg_distill_act_mix": 19, "bg_distill_head_sym": 16, "bg_distill_head_sym_partial": 17}
    for s, n in want.items():
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        assert _header_arg_count(header, s) == n and len(getattr(lib, s).argtypes) == n, (s, _header_arg_count(header, s), len(getattr(lib, s).argtypes))
    assert _header_arg_count(header, "bg_distill_act_mix") == _header_arg_count(header, "bg_distill_act_hist") + 2
    assert lib.bg_distill_head_sym_partial.argtypes[-2] == C.POINTER(_lib.ReduceProblem)
    assert lib.bg_distill_act_mix.argtypes[13:15] == [C.c_float, C.c_int32]
    rng = open(os.path.join(ROOT, "booster_gym_amd", "csrc", "bg_rng.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"\b(RS_[A-Z0-9_]+)\s*=\s*(\d+)", rng)}
    assert ids["RS_DAGGER"] == 29 and ids["RS_PERM"] == 28 and ids["RS_ACTOR"] == 32 and list(ids.values()).count(29) == 1  # no existing id moved


def test_abi_argument_errors_without_gpu():
    """The entry points check their arguments on the host before any launch."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    f = (C.c_float * 4096)()
    d = (C.c_double * 4)()
    src, sign = (C.c_int32 * 12)(*range(12)), (C.c_float * 12)(*([1.0] * 12))
    fin = _lib.ReduceProblem()
    head = lambda B=4, h=f, W=f, b=f, t=f, c=1.0, s=src, sg=sign, g=f, gW=f, gb=f, gbh=f, st=d, sc=f: lib.bg_distill_head_sym(B, h, W, b, t, c, s, sg, None, g, gW, gb,
                                                                                                                               gbh, st, sc, None)
    bad_src = (C.c_int32 * 12)(*([1, 2, 0] + list(range(3, 12))))  # a permutation that is not its own inverse
    for kw in (dict(B=0), dict(h=None), dict(W=None), dict(b=None), dict(t=None), dict(g=None), dict(gW=None), dict(gb=None), dict(gbh=None), dict(st=None),
               dict(sc=None), dict(s=None), dict(sg=None), dict(s=bad_src), dict(c=-1.0), dict(c=float("nan")), dict(c=float("inf"))):
        assert head(**kw) < 0 and b"bg_distill_head_sym" in lib.bg_last_error(), kw
    assert lib.bg_distill_head_sym_partial(4, f, f, f, f, 1.0, src, sign, None, f, f, f, f, d, f, None, None) < 0 and b"bg_distill_head_sym_partial" in lib.bg_last_error()
    assert lib.bg_distill_head_sym_partial(0, f, f, f, f, 1.0, src, sign, None, f, f, f, f, d, f, fin, None) < 0 and b"bg_distill_head_sym_partial" in lib.bg_last_error()

    p16 = (C.addressof(f) + 15) & ~15

    def net(k_in, hidden=(128, 128)):
        w = (k_in,) + tuple(hidden) + (12,)
        return (_lib.MlpLayerDesc * (len(w) - 1))(*[_lib.MlpLayerDesc(p16, p16, w[i], w[i + 1]) for i in range(len(w) - 1)])

    mix = lambda N=4, obs=f, ts=234, sobs=f, ss=234, s=net(47), t=net(234), scan=187, ls=f, beta=0.5, a=f, tm=f: lib.bg_distill_act_mix(
        N, obs, ts, sobs, ss, 3, s, 3, t, scan, ls, 0, 0, beta, 1, None, a, tm, None)
    for beta in (1.5, float("nan"), -0.25, float("inf")):
        assert mix(beta=beta) < 0 and b"bg_distill_act_mix" in lib.bg_last_error() and b"beta" in lib.bg_last_error(), beta
    assert mix(beta=2.0, N=0, obs=None) < 0 and b"beta" in lib.bg_last_error()  # beta is looked at first
    for kw in (dict(N=0), dict(obs=None), dict(sobs=None), dict(s=None), dict(t=None), dict(ls=None), dict(a=None), dict(tm=None), dict(scan=-1)):
        assert mix(**kw) == -1 and b"bg_distill_act_mix" in lib.bg_last_error() and b"beta" not in lib.bg_last_error(), kw
    f2 = (C.c_float * 4096)()
    for kw, word in ((dict(ts=235), b"teacher_stride"), (dict(sobs=f2, ss=48, s=net(47)), b"student_stride"), (dict(s=net(94)), b"student"),
                     (dict(t=net(234, (128, 192))), b"teacher"), (dict(s=net(47, (128, 64))), b"student")):
        assert mix(**kw) == -4 and b"bg_distill_act_mix" in lib.bg_last_error() and word in lib.bg_last_error(), (kw, lib.bg_last_error())
