"""The gait record without a GPU: gait_report on a hand-made record against numbers worked out here, the rule's restatement (tests/gait_ref.py) on
synthetic contact streams against closed forms, the `evaluation.gait` key, and the two entry points' ABI and argument errors."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from gait_ref import GaitRestatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, G = 0.02, 10.0
MASS = [30.0, 30.0, 40.0, 40.0, 30.0, 50.0]  # mass g = 300, 300, 400, 400, 300, 500 N


# ------------------------------------------------------------------ 1. the report
def _records():
    """6 robots on 2 levels (a third is empty) and 3 columns.
    robot level type STATE LEN  L'  MOV  D1    D2    TAU2 TILT WOB  DS FL STANCE  TD    IMP        PEAK     SLIP       CLR        SWT    SWC   dist POWER
      0     0    0     1   101 100  50   9.9   4.9   2000 1.0  4.0  10  0 30,30   5,5   1500,2000  600,900  0.1,0.3    0.25,0.20  50,40  5,4   5    3000
      1     0    2     1    51  50   0   0.49  0.48   500 0.5  1.0   0  0  0,0    0,0      0,0     300,300  0,0        0,0         0,0   0,0   0     100   never moved
      2     0    0     0    80  80  40   7.9   7.8   1600 0.8  1.6   0 10 10,20   4,2   2000,600   800,400  0.2,0.0    0.12,0      12,0  3,0   2    1600   unfinished
      3     1    1     1     1   0   0   0     0        0 0    0     0  0  0,0    0,0      0,0       0,0    0,0        0,0         0,0   0,0   0       0   ended at step 1
      4     1    0     1    61  60  20   5.9   5.8    600 0.6  1.2   5  5 10,10   2,2    600,800   450,600  0.0,0.1    0.06,0.10  10,12  2,2   3     900
      5     1    1     1    31  30  10   2.9   2.8    300 0.3  0.6  10  0 10,10   0,0      0,0     250,500  0.05,0.05  0,0         0,0   0,0   0     150   SWC = 0"""
    from booster_gym_amd import _lib as L

    g, r = np.zeros((L.GAIT_PLANES, 6), dtype=np.float32), np.zeros((L.EVAL_PLANES, 6), dtype=np.float32)
    r[L.EVAL_LEVEL], r[L.EVAL_TYPE] = [0, 0, 0, 1, 1, 1], [0, 2, 0, 1, 0, 1]
    r[L.EVAL_X0], r[L.EVAL_Y0] = [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 0]
    r[L.EVAL_X1], r[L.EVAL_Y1] = [3, 0, 0, 0, 1, 0], [4, 0, 2, 0, 4, 0]
    r[L.EVAL_POWER] = [3000, 100, 1600, 0, 900, 150]
    g[L.GAIT_STATE], g[L.GAIT_LEN], g[L.GAIT_MOV] = [1, 1, 0, 1, 1, 1], [101, 51, 80, 1, 61, 31], [50, 0, 40, 0, 20, 10]
    g[L.GAIT_D1], g[L.GAIT_D2] = [9.9, 0.49, 7.9, 0, 5.9, 2.9], [4.9, 0.48, 7.8, 0, 5.8, 2.8]
    g[L.GAIT_TAU2], g[L.GAIT_TILT], g[L.GAIT_WOBBLE] = [2000, 500, 1600, 0, 600, 300], [1.0, 0.5, 0.8, 0, 0.6, 0.3], [4.0, 1.0, 1.6, 0, 1.2, 0.6]
    g[L.GAIT_DS], g[L.GAIT_FL] = [10, 0, 0, 0, 5, 10], [0, 0, 10, 0, 5, 0]
    feet = {L.GAIT_STANCE: ([30, 0, 10, 0, 10, 10], [30, 0, 20, 0, 10, 10]), L.GAIT_TD: ([5, 0, 4, 0, 2, 0], [5, 0, 2, 0, 2, 0]),
            L.GAIT_IMP: ([1500, 0, 2000, 0, 600, 0], [2000, 0, 600, 0, 800, 0]), L.GAIT_PEAK: ([600, 300, 800, 0, 450, 250], [900, 300, 400, 0, 600, 500]),
            L.GAIT_SLIP: ([0.1, 0, 0.2, 0, 0.0, 0.05], [0.3, 0, 0.0, 0, 0.1, 0.05]), L.GAIT_CLR: ([0.25, 0, 0.12, 0, 0.06, 0], [0.20, 0, 0, 0, 0.10, 0]),
            L.GAIT_SWT: ([50, 0, 12, 0, 10, 0], [40, 0, 0, 0, 12, 0]), L.GAIT_SWC: ([5, 0, 3, 0, 2, 0], [4, 0, 0, 0, 2, 0])}
    for k, (left, right) in feet.items():
        g[L.gait_foot_plane(k, 0)], g[L.gait_foot_plane(k, 1)] = left, right
    g[L.GAIT_A1 :] = 7.0  # the carries are the kernel's own: nothing of the report may read them
    return g, r


def test_report_of_a_hand_made_record():
    from booster_gym_amd.utils.evaluate import gait_report

    g, r = _records()
    rep = gait_report(g, r, DT, MASS, G, 3, 3)
    ap = lambda x: pytest.approx(x, rel=1e-6, abs=1e-6)  # (the record is float32: 0.49 is not 0.49, 0.25 / 5 not 0.20 / 4)
    assert set(rep) == {"all", "by_level", "by_type"} and len(rep["by_level"]) == 3 and len(rep["by_type"]) == 3
    a = rep["all"]
    assert a["moving_steps"] == 120
    assert a["mean_action_rate"] == ap(27.09 / 315) and a["mean_action_accel"] == ap(21.78 / 310)  # sum max(L' - 1, 0) = 315, sum max(L' - 2, 0) = 310
    assert a["mean_torque_sq"] == ap(5000 / 320) and a["mean_tilt_sq"] == ap(3.2 / 320) and a["mean_ang_vel_xy_sq"] == ap(8.4 / 320)
    assert a["duty_factor"] == [ap(60 / 120), ap(70 / 120)] and a["double_support"] == ap(25 / 120) and a["flight"] == ap(15 / 120)
    assert a["step_frequency_hz"] == [ap(11 / 2.4), ap(9 / 2.4)]
    assert a["stance_asymmetry"] == ap((0 + 1 / 3 + 0 + 0) / 4)  # robots 0, 2, 4, 5 ever stood while moving
    assert a["swing_asymmetry"] == ap((0 + 0.02 / 0.08) / 2)     # robots 0 (0.05, 0.05) and 4 (0.03, 0.05) closed a swing on both feet
    assert a["foot_slip_m_per_s"] == ap(0.8 / 2.4)
    assert a["touchdown_force_n"] == [ap(4100 / 11), ap(3400 / 9)]
    assert a["peak_force_bw"] == [ap((2 + 1 + 2 + 0 + 1.5 + 0.5) / 6), ap((3 + 1 + 1 + 0 + 2 + 1) / 6)]
    assert a["swing_clearance_m"] == [ap(0.43 / 10), ap(0.30 / 6)] and a["swing_time_s"] == [ap(DT * 72 / 10), ap(DT * 52 / 6)]
    assert a["cost_of_transport"] == ap(DT * 5750 / (300 * 5 + 400 * 2 + 300 * 3))
    l0, l1, l2 = rep["by_level"]
    assert l0["duty_factor"] == [ap(40 / 90), ap(50 / 90)] and l0["stance_asymmetry"] == ap((0 + 1 / 3) / 2) and l0["swing_asymmetry"] == ap(0.0)
    assert l0["mean_action_rate"] == ap((9.9 + 0.49 + 7.9) / (99 + 49 + 79)) and l0["cost_of_transport"] == ap(DT * 4700 / 2300)
    assert l1["mean_action_rate"] == ap(8.8 / 88) and l1["mean_action_accel"] == ap(8.6 / 86) and l1["mean_torque_sq"] == ap(900 / 90)
    assert l1["cost_of_transport"] == ap(DT * 1050 / 900) and l1["moving_steps"] == 30 and l1["flight"] == ap(5 / 30)
    assert l1["peak_force_bw"] == [ap((0 + 1.5 + 0.5) / 3), ap((0 + 2 + 1) / 3)]
    # the empty group: every quotient lacks its denominator
    assert l2["moving_steps"] == 0
    for key, v in l2.items():
        if key != "moving_steps":
            assert v is None or v == [None, None], key
    t0, t1, t2 = rep["by_type"]
    # type 1 = robots 3 and 5: they moved, but nobody touched down, closed a swing or covered any distance
    assert t1["moving_steps"] == 10 and t1["duty_factor"] == [ap(1.0), ap(1.0)] and t1["double_support"] == ap(1.0) and t1["flight"] == ap(0.0)
    assert t1["step_frequency_hz"] == [ap(0.0), ap(0.0)] and t1["touchdown_force_n"] == [None, None]
    assert t1["swing_clearance_m"] == [None, None] and t1["swing_time_s"] == [None, None] and t1["swing_asymmetry"] is None
    assert t1["stance_asymmetry"] == ap(0.0) and t1["cost_of_transport"] is None and t1["foot_slip_m_per_s"] == ap(0.1 / 0.2)
    assert t1["mean_action_rate"] == ap(2.9 / 29)  # robot 3 ended at its first step: no live step, nothing in any denominator
    # type 2 = robot 1, which never moved: nothing over MOV, the per-step means still there
    for key in ("double_support", "flight", "foot_slip_m_per_s", "stance_asymmetry", "swing_asymmetry", "cost_of_transport"):
        assert t2[key] is None, key
    assert t2["duty_factor"] == [None, None] and t2["step_frequency_hz"] == [None, None] and t2["moving_steps"] == 0
    assert t2["mean_torque_sq"] == ap(10.0) and t2["mean_action_rate"] == ap(0.01) and t2["peak_force_bw"] == [ap(1.0), ap(1.0)]
    for part in (rep["by_level"], rep["by_type"]):
        assert sum(x["moving_steps"] for x in part) == a["moving_steps"]
    json.dumps(rep)  # (plain Python numbers throughout)
    with pytest.raises(ValueError, match="60"):
        gait_report(g[:59], r, DT, MASS, G, 1, 1)
    with pytest.raises(ValueError, match="23"):
        gait_report(g, r[:, :5], DT, MASS, G, 1, 1)
    with pytest.raises(ValueError, match="mass"):
        gait_report(g, r, DT, MASS[:5], G, 1, 1)


def test_report_table_is_added_only_with_the_key():
    from booster_gym_amd.utils.evaluate import evaluation_report, format_report, gait_report

    g, r = _records()
    rep = evaluation_report(r, DT, 3, 3)
    plain = format_report(rep)
    assert "gait" not in plain and len(plain.split("\n")) == 1 + 7
    gr = gait_report(g, r, DT, MASS, G, 3, 3)
    rep["all"]["gait"] = gr["all"]
    for key in ("by_level", "by_type"):
        for grp, gg in zip(rep[key], gr[key]):
            grp["gait"] = gg
    both = format_report(rep)
    assert both.startswith(plain + "\n") and len(both.split("\n")) == len(plain.split("\n")) + 3 + 7  # the first table byte for byte, then the second
    assert "0.500/0.583" in both and " - " in both  # "all"'s duty factors; the empty level's dashes


# ------------------------------------------------------------------ 2. the rule on synthetic streams
def _drive(stance, swing, steps, settle=0, command=0.5):
    """One robot whose foot f is in stance for stance[f] steps, then in swing for swing[f], foot 1 half of its period ahead; constant actions;
    a swing foot 5 cm up, a stance foot loaded with 400 N and at rest."""
    ref = GaitRestatement(1)
    ref.begin()
    f32 = np.float32
    a, tau = np.full((1, 12), 0.25, f32), np.full((1, 12), 2.0, f32)
    g, w, cmd = np.array([[0.1, 0.2, -0.97]], f32), np.array([[0.3, 0.4, 0.5]], f32), np.array([[command, 0.0, 0.0]], f32)
    for t in range(1, steps + 1):
        c = [((t - 1 + f * (stance[f] + swing[f]) // 2) % (stance[f] + swing[f])) < stance[f] for f in range(2)]
        contact = np.array([[1.0 if c[0] else 0.0, 1.0 if c[1] else 0.0]], f32)
        forces = np.array([[0, 0, 400.0 * c[0], 0, 0, 400.0 * c[1]]], f32)
        pos = np.array([[1.0, 0.1, 0.0 if c[0] else 0.05, 1.0, -0.1, 0.0 if c[1] else 0.05]], f32)
        ref.step(np.zeros(1, bool), a, tau, g, w, cmd, contact, forces, pos, pos[:, [2, 5]].astype(np.float64), settle)
    return ref


def _report(ref):
    from booster_gym_amd import _lib as L
    from booster_gym_amd.utils.evaluate import gait_report

    return gait_report(ref.rec, np.zeros((L.EVAL_PLANES, ref.n)), DT, np.full(ref.n, 30.0), G, 1, 1)["all"]


def test_alternating_stream_gives_the_closed_forms():
    from booster_gym_amd import _lib as L

    K = 80  # five periods of 10 stance + 6 swing steps, the right foot eight steps ahead
    ref = _drive((10, 10), (6, 6), K)
    r, a = ref.rec, _report(ref)
    assert r[L.GAIT_D1, 0] == 0 and r[L.GAIT_D2, 0] == 0 and a["mean_action_rate"] == 0 and a["mean_action_accel"] == 0
    assert a["stance_asymmetry"] == 0 and a["swing_asymmetry"] == 0 and a["moving_steps"] == K
    assert a["duty_factor"] == [pytest.approx(10 / 16), pytest.approx(10 / 16)]
    assert a["double_support"] == pytest.approx(4 / 16) and a["flight"] == 0  # both feet down during 2 + 2 of a period's 16 steps
    # the left foot lands at steps 17, 33, 49, 65 (step 1 has no step before it), the right at 9, 25, 41, 57, 73
    assert a["step_frequency_hz"] == [pytest.approx(4 / (K * DT)), pytest.approx(5 / (K * DT))]
    assert a["swing_time_s"] == [pytest.approx(6 * DT), pytest.approx(6 * DT)] and a["swing_clearance_m"] == [pytest.approx(0.05), pytest.approx(0.05)]
    assert a["touchdown_force_n"] == [pytest.approx(400.0), pytest.approx(400.0)] and a["peak_force_bw"] == [pytest.approx(400 / 300), pytest.approx(400 / 300)]
    assert a["foot_slip_m_per_s"] == 0 and a["cost_of_transport"] is None  # (no distance in the zero first record)
    assert a["mean_torque_sq"] == pytest.approx(48.0) and a["mean_tilt_sq"] == pytest.approx(0.05) and a["mean_ang_vel_xy_sq"] == pytest.approx(0.25)
    assert [t for t, e, f, s in ref.touchdowns if f == 0] == [17, 33, 49, 65] and {s for _, _, _, s in ref.touchdowns} == {6}


def test_a_longer_left_stance_gives_the_closed_form_asymmetry():
    K = 144  # eight periods of 12 + 6 on the left, nine of 10 + 6 on the right
    a = _report(_drive((12, 10), (6, 6), K))
    assert a["duty_factor"] == [pytest.approx(96 / 144), pytest.approx(90 / 144)] and a["stance_asymmetry"] == pytest.approx(6 / 186)
    assert a["swing_time_s"] == [pytest.approx(6 * DT), pytest.approx(6 * DT)]


def test_settling_a_zero_command_and_the_end_of_the_episode():
    from booster_gym_amd import _lib as L

    # settle_steps = 20: the sums over all live steps go on, the gait counters start at step 21; a swing that began before lands after and counts whole
    ref = _drive((10, 10), (6, 6), 80, settle=20)
    assert ref.rec[L.GAIT_MOV, 0] == 60 and ref.rec[L.GAIT_TAU2, 0] == pytest.approx(80 * 48.0)
    assert (25, 0, 1, 6) in ref.touchdowns  # the right foot's swing of steps 19 .. 24
    still = _drive((10, 10), (6, 6), 80, command=0.0)
    assert still.rec[L.GAIT_MOV, 0] == 0 and still.rec[L.gait_foot_plane(L.GAIT_TD, 0), 0] == 0 and still.rec[L.GAIT_TILT, 0] > 0
    # done: LEN counts the step, nothing else moves, and the record stays frozen
    before = ref.rec.copy()
    z = np.zeros
    args = (z((1, 12), np.float32), z((1, 12), np.float32), z((1, 3), np.float32), z((1, 3), np.float32), np.ones((1, 3), np.float32),
            np.ones((1, 2), np.float32), z((1, 6), np.float32), z((1, 6), np.float32), z((1, 2)), 20)
    ref.step(np.ones(1, bool), *args)
    before[L.GAIT_LEN] += 1
    before[L.GAIT_STATE] = 1
    assert np.array_equal(ref.rec, before)
    ref.step(np.zeros(1, bool), *args)
    assert np.array_equal(ref.rec, before)


# ------------------------------------------------------------------ 3. the section
def test_gait_key_is_optional_boolean_and_not_in_the_shipped_mapping():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.evaluate import evaluation_cfg, gait_of

    cfg = load_cfg("T1")
    assert cfg["evaluation"] == {"settle_s": 1.0, "spread_terrain_levels": True}  # exactly the mapping of before the key
    assert evaluation_cfg(cfg) == (1.0, True) and gait_of(cfg) is False
    cfg["evaluation"]["gait"] = True
    assert evaluation_cfg(cfg) == (1.0, True) and gait_of(cfg) is True
    cfg["evaluation"] = {"gait": False}
    assert evaluation_cfg(cfg) == (1.0, True) and gait_of(cfg) is False
    for absent in (None, {}):
        cfg["evaluation"] = absent
        assert gait_of(cfg) is False
    del cfg["evaluation"]
    assert gait_of(cfg) is False
    for bad in (1, 0, "true", None, [True]):
        cfg["evaluation"] = {"gait": bad}
        for fn in (evaluation_cfg, gait_of):
            with pytest.raises(ValueError, match=r"evaluation\.gait\b"):
                fn(cfg)
    assert gait_of(load_cfg("T1", {"evaluation.gait": True})) is True


# ------------------------------------------------------------------ 4. C ABI
def test_entry_points_are_declared_exported_and_bound():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    for name, n in (("bg_env_gait_begin", 3), ("bg_env_gait_step", 5)):
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", header)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, name
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n, name
        assert getattr(lib, name).restype is C.c_int32
    assert lib.bg_env_gait_step.argtypes[2] is C.c_int32
    assert int(re.search(r"#define BG_GAIT_PLANES (\d+)", header).group(1)) == _lib.GAIT_PLANES == 60
    names = _lib.gait_plane_names()
    assert len(names) == len(set(names)) == _lib.GAIT_PLANES and names[_lib.GAIT_FL] == "FL" and names[_lib.GAIT_A1] == "A1_0"
    assert names[_lib.gait_foot_plane(_lib.GAIT_SWC, 1)] == "SWC_1" and _lib.gait_foot_plane(_lib.GAIT_SWC, 1) + 1 == _lib.GAIT_A1 == 26
    assert names[_lib.GAIT_A2] == "A2_0" and names[_lib.GAIT_CPREV] == "CPREV_0" and names[_lib.GAIT_PPREV + 3] == "PPREV_1_y"
    assert names[_lib.GAIT_SWMAX] == "SWMAX_0" and names[_lib.GAIT_SWN + 1] == "SWN_1" and _lib.GAIT_SWN + 2 == _lib.GAIT_PLANES
    assert len(_lib.eval_plane_names()) == _lib.EVAL_PLANES and _lib.eval_plane_names()[_lib.eval_track_plane(2, 3)] == "SQ_yaw_fast"
    assert "gait" not in " ".join(f[0] for f in _lib.EnvCfg._fields_ if f[0] != "cmd_gait_frequency")  # the caller's buffer: bg_env_cfg has no new field


def test_null_arguments_are_errors_naming_the_argument_before_any_launch():
    """No device: every check precedes the first use of `env`, so a buffer that is no env at all stands in for one and is never read."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    err = lambda: lib.bg_last_error().decode()
    assert lib.bg_env_gait_begin(None, p, None) < 0 and "bg_env_gait_begin" in err() and "env" in err()
    assert lib.bg_env_gait_begin(p, None, None) < 0 and "bg_env_gait_begin" in err() and "record" in err()
    assert lib.bg_env_gait_step(None, p, 5, p, None) < 0 and "bg_env_gait_step" in err() and "env" in err()
    assert lib.bg_env_gait_step(p, None, 5, p, None) < 0 and "null done" in err()
    assert lib.bg_env_gait_step(p, p, 5, None, None) < 0 and "record" in err()
    assert lib.bg_env_gait_step(p, p, -3, p, None) < 0 and "settle_steps" in err() and "-3" in err()
    assert bytes(buf) == bytes(64)
