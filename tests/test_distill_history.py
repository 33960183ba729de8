"""distillation.student_frame_stack without a GPU: the key's resolution (student_frame_stack_of, every error names the key), the overrides the
longer-history student re-enters the tools under, the shipped section, DistillCfg's unchanged shape, the env-side reading of the key and the C ABI of
the three new entry points."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = r"distillation\.student_frame_stack"


def _cfg(H=1, Hs=None, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_privileged_obs": 201, "env.frame_stack": H,
          "env.num_observations": 47 * H + 187}
    if Hs is not None:
        ov["distillation.student_frame_stack"] = Hs
    ov.update(over)
    return load_cfg("T1", ov)


def test_key_resolves_to_the_teachers_frame_stack_by_default_and_to_a_valid_value():
    from booster_gym_amd.utils.distill import student_frame_stack_of

    assert student_frame_stack_of(_cfg()) == 1  # the shipped section (null) with the scan on: H
    assert student_frame_stack_of(_cfg(2)) == 2
    assert student_frame_stack_of(_cfg(1, 5)) == 5
    assert student_frame_stack_of(_cfg(1, 6)) == 6  # 47 x 6 + 14 + 187 = 483
    assert student_frame_stack_of(_cfg(2, 2)) == 2  # equal to H is allowed: today's path
    cfg = _cfg()
    del cfg["distillation"]["student_frame_stack"]  # a yaml written before the key existed
    assert student_frame_stack_of(cfg) == 1


@pytest.mark.parametrize("H,Hs", [(2, 1), (1, 11), (1, True), (1, 2.5), (1, 0), (1, "5")])
def test_bad_values_are_value_errors_naming_the_key(H, Hs):
    from booster_gym_amd.utils.distill import student_frame_stack_of

    with pytest.raises(ValueError, match=KEY):
        student_frame_stack_of(_cfg(H, Hs))


def test_a_student_config_past_the_critics_512_columns_names_the_key_and_the_grid():
    from booster_gym_amd.utils.distill import student_frame_stack_of

    with pytest.raises(ValueError, match=KEY + r".*terrain\.measured_points_x.*terrain\.measured_points_y") as e:
        student_frame_stack_of(_cfg(1, 7))  # 47 x 7 + 14 + 187 = 530 > 512
    assert "530" in str(e.value)
    small = {"terrain.measured_points_x": [-0.2, -0.1, 0.0, 0.1, 0.2], "terrain.measured_points_y": [-0.1, 0.0, 0.1], "env.num_privileged_obs": 29,
             "env.num_observations": 47 + 15}
    assert student_frame_stack_of(_cfg(1, 10, **small)) == 10  # 470 + 14 + 15 = 499


def test_overrides_of_a_longer_history_and_of_the_key_absent():
    from booster_gym_amd.envs.t1 import check_env_sizes
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import student_cfg_overrides

    assert student_cfg_overrides(_cfg(1, 5)) == {"terrain.actor_heights": False, "env.frame_stack": 5, "env.num_observations": 235}
    assert student_cfg_overrides(_cfg()) == {"terrain.actor_heights": False, "env.num_observations": 47}
    assert student_cfg_overrides(_cfg(2, 2)) == {"terrain.actor_heights": False, "env.num_observations": 94}
    # the student's config passes the env's own validation
    over = {"terrain.measure_heights": True, "env.num_privileged_obs": 201}
    over.update(student_cfg_overrides(_cfg(1, 6)))
    check_env_sizes(load_cfg("T1", over), 187)


def test_shipped_section_equals_the_defaults_and_distillcfg_keeps_six_fields():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import DEFAULTS, distillation_cfg

    assert load_cfg("T1")["distillation"] == DEFAULTS and DEFAULTS["student_frame_stack"] is None
    assert len(distillation_cfg(_cfg())) == 6 and len(distillation_cfg(_cfg(1, 5))) == 6
    assert "student_frame_stack" not in load_cfg("T1")["env"]  # nothing ships it in the env: section


def test_env_side_reading_of_the_key():
    from booster_gym_amd.envs.t1 import student_frame_stack_of

    assert student_frame_stack_of(_cfg()) == 0
    assert student_frame_stack_of(_cfg(2, **{"env.student_frame_stack": 5})) == 5
    assert student_frame_stack_of(_cfg(2, **{"env.student_frame_stack": 2})) == 2
    for H, bad in ((2, 1), (1, 11), (1, True), (1, 2.5)):
        with pytest.raises(ValueError, match=KEY):
            student_frame_stack_of(_cfg(H, **{"env.student_frame_stack": bad}))
    with pytest.raises(ValueError, match=KEY + r".*terrain\.actor_heights"):
        student_frame_stack_of(_cfg(**{"env.student_frame_stack": 5, "terrain.actor_heights": False, "env.num_observations": 47}))


def _header_arg_count(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_library_declares_exports_and_binds_the_new_entry_points_and_the_config_field():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    for name, n in {"bg_env_bind_student_obs": 2, "bg_env_step_to_student": 9, "bg_distill_act_hist": 17}.items():
        assert _header_arg_count(header, name) == n and name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == n, name
    E = _lib.EnvCfg
    assert E.student_frame_stack.offset == E.noise_height_measurements.offset + C.sizeof(_lib.Rand)  # appended at the end
    assert E.student_frame_stack.offset + 4 <= C.sizeof(E)
    assert _lib.EnvCfg().student_frame_stack == 0  # a zero-initialised struct: off


def test_env_create_refuses_a_bad_field_before_it_looks_for_a_device():
    from booster_gym_amd import _lib

    lib = _lib.load()
    for Hs, scan in ((5, 0), (11, 1), (-1, 1), (1, 1)):  # without actor_heights; above the maximum; negative; below frame_stack = 2
        cfg = _lib.EnvCfg()
        cfg.num_envs, cfg.decimation, cfg.sim_dt, cfg.frame_stack, cfg.student_frame_stack = 4, 10, 0.002, 2, Hs
        pts = (C.c_float * 4)(0.0, 0.0, 0.1, 0.0)
        if scan:
            cfg.terrain_type, cfg.height_scan_points, cfg.height_scan_xy, cfg.actor_heights = 1, 2, C.cast(pts, C.c_void_p).value, 1
        out = C.c_void_p()
        assert lib.bg_env_create(C.byref(cfg), C.c_void_p(1), C.byref(out)) == -1 and b"student_frame_stack" in lib.bg_last_error(), (Hs, scan)


def test_distill_act_hist_argument_errors_are_raised_on_the_host():
    from booster_gym_amd import _lib

    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = (C.addressof(buf) + 15) & ~15  # (weight matrices after the first must be 16-byte aligned: an argument error of its own)
    net = lambda k_in: (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(p, p, k_in, 128), _lib.MlpLayerDesc(p, p, 128, 128), _lib.MlpLayerDesc(p, p, 128, 12))
    call = lambda ts, ss, s, t, scan: lib.bg_distill_act_hist(4, p, ts, p, ss, 3, net(s), 3, net(t), scan, p, 0, 0, None, p, p, None)
    assert call(235, 235, 235, 234, 187) == -4 and b"teacher_stride" in lib.bg_last_error()
    assert call(234, 236, 235, 234, 187) == -4 and b"student_stride" in lib.bg_last_error()
    assert call(234, 240, 240, 234, 187) == -4 and b"student" in lib.bg_last_error()   # not 47 Hs
    assert call(234, 517, 517, 234, 187) == -4 and b"student" in lib.bg_last_error()   # Hs = 11
    assert call(109, 47, 47, 109, 15) == -4 and b"student" in lib.bg_last_error()      # 47 Hs below the teacher's 47 H = 94
