"""evaluate.py without a GPU: the report of a hand-made record against values worked out here, the `evaluation:` section's rules (every error names
its key), the student overrides from a checkpoint dict against distill.student_cfg_overrides, and the two entry points' argument errors."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the report
def _record():
    """7 robots on 2 levels and 2 columns.  dt = 0.02.
    robot  level type state len   rew   x0,y0 -> x1,y1    class power  tracked (class: cnt, sq x / y / yaw)
      0      0    0   2     50   5.0   0,0 -> 3,4           2    98    none (fell before settling)
      1      0    0   1   1501 150.0   1,1 -> 1,1           0  3000    still: 1000, 10 / 40 / 90;  slow: 400, 16 / 4 / 36
      2      0    1   1   1501 140.0   0,0 -> 6,8           1  4500    slow: 1400, 56 / 14 / 126
      3      0    1   0   1502 100.0   0,0 -> 0,5           1  1502    slow: 1450, 58 / 58 / 58     (unfinished)
      4      1    0   2    301  20.0   2,0 -> 2,12          1   600    slow: 250, 250 / 0 / 1000
      5      1    1   2    100   2.0   0,0 -> 0,0           0   198    still: 50, 2 / 8 / 18
      6      1    1   1   1501 160.0   -1,0 -> 2,4          1  3000    slow: 1450, 14.5 / 58 / 232
    No robot ever tracked a fast command (class 2): its count is 0 in every group."""
    from booster_gym_amd import _lib as L

    r = np.zeros((L.EVAL_PLANES, 7), dtype=np.float32)
    r[L.EVAL_LEVEL] = [0, 0, 0, 0, 1, 1, 1]
    r[L.EVAL_TYPE] = [0, 0, 1, 1, 0, 1, 1]
    r[L.EVAL_STATE] = [2, 1, 1, 0, 2, 2, 1]
    r[L.EVAL_LEN] = [50, 1501, 1501, 1502, 301, 100, 1501]
    r[L.EVAL_REW] = [5, 150, 140, 100, 20, 2, 160]
    r[L.EVAL_X0], r[L.EVAL_Y0] = [0, 1, 0, 0, 2, 0, -1], [0, 1, 0, 0, 0, 0, 0]
    r[L.EVAL_X1], r[L.EVAL_Y1] = [3, 1, 6, 0, 2, 0, 2], [4, 1, 8, 5, 12, 0, 4]
    r[L.EVAL_CLASS] = [2, 0, 1, 1, 1, 0, 1]
    r[L.EVAL_POWER] = [98, 3000, 4500, 1502, 600, 198, 3000]
    still, slow = [L.eval_track_plane(0, k) for k in range(4)], [L.eval_track_plane(1, k) for k in range(4)]
    for p, v in zip(still, ([0, 1000, 0, 0, 0, 50, 0], [0, 10, 0, 0, 0, 2, 0], [0, 40, 0, 0, 0, 8, 0], [0, 90, 0, 0, 0, 18, 0])):
        r[p] = v
    for p, v in zip(slow, ([0, 400, 1400, 1450, 250, 0, 1450], [0, 16, 56, 58, 250, 0, 14.5], [0, 4, 14, 58, 0, 0, 58], [0, 36, 126, 58, 1000, 0, 232])):
        r[p] = v
    return r


def test_report_of_a_hand_made_record():
    from booster_gym_amd.utils.evaluate import evaluation_report

    rep = evaluation_report(_record(), 0.02, 2, 2)
    assert set(rep) == {"all", "by_level", "by_type"} and len(rep["by_level"]) == 2 and len(rep["by_type"]) == 2
    a = rep["all"]
    assert (a["robots"], a["fell"], a["timed_out"], a["unfinished"]) == (7, 3, 3, 1)
    assert a["fall_rate"] == pytest.approx(3 / 6)
    # falls at 50, 100 and 301 steps = 1 s, 2 s and 6.02 s: two within 2 s (the bound is inclusive), two within 6 s, three within 10 s
    assert a["fell_within_s"] == {"2": pytest.approx(2 / 7), "6": pytest.approx(2 / 7), "10": pytest.approx(3 / 7), "20": pytest.approx(3 / 7)}
    total_len = 50 + 1501 + 1501 + 1502 + 301 + 100 + 1501
    assert a["mean_episode_length"] == pytest.approx(total_len / 7)
    assert a["mean_reward_per_step"] == pytest.approx(577 / total_len)
    assert a["mean_distance_m"] == pytest.approx((5 + 0 + 10 + 5 + 12 + 0 + 5) / 7)
    # the six finished robots added LEN - 1 steps to POWER, the unfinished one all 1502
    assert a["mean_abs_joint_power_w"] == pytest.approx(12898 / (total_len - 6))
    assert a["tracked_steps"] == {"still": 1050, "slow": 4950, "fast": 0}
    assert a["tracking_rmse"]["still"] == {"lin_vel_x": pytest.approx(math.sqrt(12 / 1050)), "lin_vel_y": pytest.approx(math.sqrt(48 / 1050)),
                                           "ang_vel_yaw": pytest.approx(math.sqrt(108 / 1050))}
    assert a["tracking_rmse"]["slow"] == {"lin_vel_x": pytest.approx(math.sqrt(394.5 / 4950)), "lin_vel_y": pytest.approx(math.sqrt(134 / 4950)),
                                          "ang_vel_yaw": pytest.approx(math.sqrt(1452 / 4950))}
    assert a["tracking_rmse"]["fast"] == {"lin_vel_x": None, "lin_vel_y": None, "ang_vel_yaw": None}  # a class nobody tracked: no division
    assert a["falls_by_class"] == {"still": 1, "slow": 1, "fast": 1}
    l0, l1 = rep["by_level"]
    assert (l0["robots"], l0["fell"], l0["timed_out"], l0["unfinished"]) == (4, 1, 2, 1) and l0["fall_rate"] == pytest.approx(1 / 3)
    assert (l1["robots"], l1["fell"], l1["timed_out"], l1["unfinished"]) == (3, 2, 1, 0) and l1["fall_rate"] == pytest.approx(2 / 3)
    assert l1["mean_distance_m"] == pytest.approx(17 / 3) and l1["mean_reward_per_step"] == pytest.approx(182 / 1902)
    assert l1["mean_abs_joint_power_w"] == pytest.approx(3798 / 1899)
    assert l1["tracking_rmse"]["slow"]["lin_vel_x"] == pytest.approx(math.sqrt(264.5 / 1700)) and l1["tracked_steps"] == {"still": 50, "slow": 1700, "fast": 0}
    assert l1["falls_by_class"] == {"still": 1, "slow": 1, "fast": 0}
    t0, t1 = rep["by_type"]
    assert (t0["robots"], t0["fell"], t0["timed_out"], t0["unfinished"]) == (3, 2, 1, 0)
    assert (t1["robots"], t1["fell"], t1["timed_out"], t1["unfinished"]) == (4, 1, 2, 1)
    # every group adds up, and the groups of a partition add up to "all"
    for g in [a, l0, l1, t0, t1]:
        assert g["fell"] + g["timed_out"] + g["unfinished"] == g["robots"]
    for part in (rep["by_level"], rep["by_type"]):
        for key in ("robots", "fell", "timed_out", "unfinished"):
            assert sum(g[key] for g in part) == a[key], key
        for c in ("still", "slow", "fast"):
            assert sum(g["tracked_steps"][c] for g in part) == a["tracked_steps"][c] and sum(g["falls_by_class"][c] for g in part) == a["falls_by_class"][c]


def test_an_empty_group_reports_nulls():
    from booster_gym_amd.utils.evaluate import evaluation_report

    rep = evaluation_report(_record(), 0.02, 3, 2)  # nobody is on level 2
    g = rep["by_level"][2]
    assert (g["robots"], g["fell"], g["timed_out"], g["unfinished"]) == (0, 0, 0, 0)
    for key in ("fall_rate", "mean_episode_length", "mean_reward_per_step", "mean_distance_m", "mean_abs_joint_power_w"):
        assert g[key] is None, key
    assert all(v is None for v in g["fell_within_s"].values()) and all(v is None for c in g["tracking_rmse"].values() for v in c.values())
    import json

    json.dumps(rep)  # (plain Python numbers throughout)
    with pytest.raises(ValueError, match="23"):
        evaluation_report(np.zeros((22, 4)), 0.02, 1, 1)


# ------------------------------------------------------------------ the section
def test_evaluation_section_defaults_and_errors():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.evaluate import evaluation_cfg, settle_steps_of

    cfg = load_cfg("T1")
    assert cfg["evaluation"] == {"settle_s": 1.0, "spread_terrain_levels": True}  # the shipped section states the defaults
    assert evaluation_cfg(cfg) == (1.0, True)
    del cfg["evaluation"]
    assert evaluation_cfg(cfg) == (1.0, True)  # absent: the defaults
    cfg["evaluation"] = None
    assert evaluation_cfg(cfg) == (1.0, True)
    cfg["evaluation"] = {"settle_s": 0, "spread_terrain_levels": False}
    assert evaluation_cfg(cfg) == (0.0, False)
    assert settle_steps_of(1.0, 0.02) == 50 and settle_steps_of(0.0, 0.02) == 0 and settle_steps_of(0.05, 0.02) == 3 and settle_steps_of(0.1, 0.02) == 5
    for sec, key in (({"settle": 1.0}, "evaluation.settle"), ({"settle_s": -0.5}, "evaluation.settle_s"), ({"settle_s": "1"}, "evaluation.settle_s"),
                     ({"settle_s": True}, "evaluation.settle_s"), ({"settle_s": float("nan")}, "evaluation.settle_s"),
                     ({"spread_terrain_levels": 1}, "evaluation.spread_terrain_levels"), ({"spread_terrain_levels": None}, "evaluation.spread_terrain_levels")):
        cfg["evaluation"] = sec
        with pytest.raises(ValueError, match=re.escape(key) + r"\b"):
            evaluation_cfg(cfg)
    cfg["evaluation"] = [1.0]
    with pytest.raises(ValueError, match="evaluation must be a mapping"):
        evaluation_cfg(cfg)


# ------------------------------------------------------------------ the student's overrides
@pytest.mark.parametrize("H,Hs", [(1, None), (2, None), (2, 2), (2, 4)])
def test_student_overrides_from_a_checkpoint_equal_those_from_the_teachers_config(H, Hs):
    """The fake checkpoint holds what Distiller.checkpoint_dict writes for that config: the actor's first layer 47 max(H, Hs) wide, and
    "student_frame_stack" in the entry only with a history longer than the teacher's."""
    import torch

    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides, student_overrides

    P = 15
    cfg = load_cfg("T1", {"env.frame_stack": H, "terrain.type": "trimesh", "terrain.measure_heights": True, "terrain.actor_heights": True,
                          "env.num_observations": 47 * H + P, "env.num_privileged_obs": 14 + P, "distillation.student_frame_stack": Hs,
                          "terrain.measured_points_x": [-0.2, -0.1, 0.0, 0.1, 0.2], "terrain.measured_points_y": [-0.1, 0.0, 0.1]})
    longer = Hs is not None and Hs > H
    entry = {"teacher": "teacher.pth", "iteration": 1, "loss": 0.5}
    if longer:
        entry["student_frame_stack"] = Hs
    ck = {"model": {"actor.0.weight": torch.zeros(256, 47 * (Hs if longer else H))}, "distillation": entry}
    want = student_cfg_overrides(cfg)
    assert checkpoint_student_overrides(ck) == want
    assert want == student_overrides(47 * (Hs if longer else H), Hs if longer else None)
    assert ("env.frame_stack" in want) == longer and want["terrain.actor_heights"] is False
    assert checkpoint_student_overrides({"model": ck["model"]}) is None  # a checkpoint of Runner's: no entry, no overrides


# ------------------------------------------------------------------ C ABI
def test_entry_points_are_declared_exported_and_bound():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    lib = _lib.load()
    for name, n in (("bg_env_eval_begin", 3), ("bg_env_eval_step", 7)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, name
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n, name
    assert int(re.search(r"#define BG_EVAL_PLANES (\d+)", header).group(1)) == _lib.EVAL_PLANES == 23
    assert _lib.eval_track_plane(_lib.EVAL_CLASSES - 1, 3) == _lib.EVAL_PLANES - 1 and _lib.EVAL_TRACK == _lib.EVAL_POWER + 1 == 11
    assert "evaluation" not in " ".join(f[0] for f in _lib.EnvCfg._fields_)  # the record is the caller's buffer: bg_env_cfg has no new field


def test_null_arguments_are_errors_naming_the_argument_before_any_launch():
    """No device: every check precedes the first use of `env`, so a buffer that is no env at all stands in for one and is never read."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    buf = C.create_string_buffer(64)
    p = C.c_void_p(C.addressof(buf))
    err = lambda: lib.bg_last_error().decode()
    assert lib.bg_env_eval_begin(None, p, None) < 0 and "bg_env_eval_begin" in err() and "env" in err()
    assert lib.bg_env_eval_begin(p, None, None) < 0 and "bg_env_eval_begin" in err() and "record" in err()
    assert lib.bg_env_eval_step(None, p, p, p, 5, p, None) < 0 and "bg_env_eval_step" in err() and "env" in err()
    assert lib.bg_env_eval_step(p, None, p, p, 5, p, None) < 0 and "null rew" in err()
    assert lib.bg_env_eval_step(p, p, None, p, 5, p, None) < 0 and "null done" in err()
    assert lib.bg_env_eval_step(p, p, p, None, 5, p, None) < 0 and "time_outs" in err()
    assert lib.bg_env_eval_step(p, p, p, p, 5, None, None) < 0 and "record" in err()
    assert lib.bg_env_eval_step(p, p, p, p, -1, p, None) < 0 and "settle_steps" in err() and "-1" in err()
    assert bytes(buf) == bytes(64)
