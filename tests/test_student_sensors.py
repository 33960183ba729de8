"""distillation.student_sensors without a GPU: the key's rules (absent or null = off; every refusal of the `sensors:` section's list, under the new
prefix, names its key), the untouched refusal of sensors.enabled with terrain.actor_heights, the re-entry overrides from a config and from a
checkpoint (key on and off, Hs = H and Hs > H, a recurrent student), and bg_env_create's argument checks of sensor_model = 2."""
import ctypes as C

import pytest
import torch

import test_sensors
from test_sensors import FULL_BIAS, GAUSS, LATENCY

P = 187
PREFIX = "distillation.student_sensors"
SECTION = {"bias": FULL_BIAS, "latency_steps": LATENCY}
# the `sensors:` section's own refusals (tests/test_sensors.py), without those of `enabled` (the key has none) and of terrain.actor_heights (the key needs it)
SENSORS_REFUSALS = [(over, match) for over, match in test_sensors.test_every_refusal_names_its_key.pytestmark[0].args[1]
                    if not any(k == "sensors.enabled" or k.startswith("terrain.") for k in over)]


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", {"terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 + P, "env.num_privileged_obs": 14 + P,
                           **over})


def test_absent_or_null_is_off_and_a_mapping_is_the_sensors_section_without_enabled():
    from booster_gym_amd.envs import t1
    from booster_gym_amd.utils.distill import DEFAULTS, distillation_cfg, student_sensors_of
    from booster_gym_amd.utils.sensors import GROUPS, SensorsCfg, sensors_as_section

    assert DEFAULTS["student_sensors"] is None and _cfg()["distillation"] == DEFAULTS
    assert student_sensors_of(_cfg()) is None and student_sensors_of(_cfg(**{PREFIX: None})) is None
    absent = _cfg()
    del absent["distillation"]["student_sensors"]
    assert student_sensors_of(absent) is None and distillation_cfg(absent) == distillation_cfg(_cfg())
    assert student_sensors_of({"terrain": {}}) is None  # (no distillation section: nothing to read)
    nothing = SensorsCfg((None, None, None, None), (0.0, 0.0))
    assert student_sensors_of(_cfg(**{PREFIX: {}})) == nothing
    assert student_sensors_of(_cfg(**{PREFIX: {"bias": None, "latency_steps": None}})) == nothing
    got = student_sensors_of(_cfg(**{PREFIX: SECTION}))
    assert got.bias == tuple(FULL_BIAS[g] for g in GROUPS) and got.latency_steps == (0.25, 1.75) and got.extra_planes == 2
    assert distillation_cfg(_cfg(**{PREFIX: SECTION})) == distillation_cfg(_cfg())  # (the other keys are read as before)
    plain = sensors_as_section(got)
    assert plain == {"bias": FULL_BIAS, "latency_steps": LATENCY} and plain["bias"]["gravity"] is not FULL_BIAS["gravity"]
    assert sensors_as_section(nothing) == {"bias": {g: None for g in GROUPS}, "latency_steps": [0.0, 0.0]}
    # the env's side of the hand-over (env.student_sensors, as env.student_frame_stack): the same rules, and the student's own row
    cfg = _cfg()
    cfg["env"]["student_sensors"] = plain
    with pytest.raises(ValueError, match=r"distillation\.student_sensors needs the student's own row"):
        t1.student_sensors_of(cfg)
    cfg["env"]["student_frame_stack"] = 1
    assert t1.student_sensors_of(cfg) == got and t1.student_sensors_of(_cfg()) is None


@pytest.mark.parametrize("over,match", SENSORS_REFUSALS + [
    ({"sensors.enabled": True}, r"distillation\.student_sensors\.enabled is not a key"),
    ({"sensors": [1]}, r"distillation\.student_sensors must be null or a mapping"),
    ({"sensors": 1}, r"distillation\.student_sensors must be null or a mapping"),
])
def test_every_refusal_names_its_key(over, match):
    from booster_gym_amd.envs import t1
    from booster_gym_amd.utils.distill import distillation_cfg, student_cfg_overrides, student_sensors_of

    assert len(SENSORS_REFUSALS) >= 20
    match = match.replace(r"sensors\.", r"distillation\.student_sensors\.") if match.startswith(r"sensors\.") else match
    cfg = _cfg(**({PREFIX: over["sensors"]} if "sensors" in over else {PREFIX: {}}))
    for k, v in over.items():  # "sensors.bias.gravity": entry -> distillation.student_sensors.bias.gravity
        node, keys = cfg["distillation"]["student_sensors"], k.split(".")[1:]
        for key in keys[:-1]:
            node = node.setdefault(key, {})
        if keys:
            node[keys[-1]] = v
    for f in (student_sensors_of, distillation_cfg, student_cfg_overrides):
        with pytest.raises(ValueError, match=match):
            f(cfg)
    env_cfg = _cfg(**{"env.student_frame_stack": 1, "env.student_sensors": cfg["distillation"]["student_sensors"]})
    with pytest.raises(ValueError, match=match):
        t1.student_sensors_of(env_cfg)


def test_sensors_enabled_with_actor_heights_still_raises_its_old_message():
    from booster_gym_amd.utils.sensors import sensors_cfg

    for extra in ({}, {PREFIX: SECTION}):
        with pytest.raises(ValueError, match=r"^sensors\.enabled is not available with terrain\.actor_heights: true: those rows, and a distillation's student "
                                             r"row with them, are written by bg_obs_assemble, which knows nothing of the sensor model$"):
            sensors_cfg(_cfg(**{"sensors.enabled": True, **extra}))
    with pytest.raises(ValueError, match=r"^sensors\.latency_steps must be"):  # (the section's own rules come first, as before)
        sensors_cfg(_cfg(**{"sensors.enabled": True, "sensors.latency_steps": [0, 3]}))


def _checkpoint(cfg, in_features, memory=0):
    """The entries of a student checkpoint that checkpoint_student_overrides reads, as Distiller.checkpoint_dict writes them."""
    from booster_gym_amd.envs.t1 import frame_stack_of
    from booster_gym_amd.utils.distill import student_frame_stack_of, student_sensors_of
    from booster_gym_amd.utils.sensors import sensors_as_section

    entry, sc = {"teacher": "t.pth", "iteration": 1, "loss": 0.5}, student_sensors_of(cfg)
    if student_frame_stack_of(cfg) > frame_stack_of(cfg):
        entry["student_frame_stack"] = student_frame_stack_of(cfg)
    if sc is not None:
        entry["student_sensors"] = sensors_as_section(sc)
    if memory:
        entry["student_memory"] = memory
        sd = {"memory.weight_ih": torch.zeros(3 * memory, 47), "memory.weight_hh": torch.zeros(3 * memory, memory), "actor.0.weight": torch.zeros(256, memory)}
    else:
        sd = {"actor.0.weight": torch.zeros(256, in_features)}
    return {"model": sd, "distillation": entry}


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("H,Hs,memory", [(1, None, 0), (2, 2, 0), (1, 3, 0), (2, 5, 0), (1, None, 128)])
def test_re_entry_overrides_from_the_config_and_from_the_checkpoint(on, H, Hs, memory):
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides

    p = 15 if H > 1 else P  # (a scan of 5 x 3 points where the frames need the room)
    over = {"env.frame_stack": H, "env.num_observations": 47 * H + p, "env.num_privileged_obs": 14 + p, "distillation.student_frame_stack": Hs,
            "distillation.student_memory": memory}
    if p == 15:
        over.update({"terrain.measured_points_x": [-0.2, -0.1, 0.0, 0.1, 0.2], "terrain.measured_points_y": [-0.1, 0.0, 0.1]})
    if on:
        over[PREFIX] = SECTION
    cfg = _cfg(**over)
    want = {"terrain.actor_heights": False}
    if Hs is not None and Hs > H:
        want["env.frame_stack"] = Hs
    want["env.num_observations"] = 47 * (Hs or H)
    if memory:
        want["algorithm.actor_memory"] = memory
    if on:
        want.update({"sensors.enabled": True, "sensors.bias": FULL_BIAS, "sensors.latency_steps": LATENCY})
    got = student_cfg_overrides(cfg)
    assert got == want and list(got) == list(want)  # (the existing keys in their order, the sensor model's behind them)
    from_ck = checkpoint_student_overrides(_checkpoint(cfg, 47 * (Hs or H), memory))
    assert from_ck == want
    assert any(k.startswith("sensors.") for k in got) == on
    # the overrides make a config the sensor model accepts, with the parameters of the section
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.sensors import sensors_cfg
    from booster_gym_amd.utils.distill import student_sensors_of

    assert sensors_cfg(load_cfg("T1", got)) == student_sensors_of(cfg)


def test_a_checkpoint_without_the_entry_re_enters_as_before():
    from booster_gym_amd.utils.distill import checkpoint_student_overrides

    ck = {"model": {"actor.0.weight": torch.zeros(256, 141)}, "distillation": {"teacher": "t.pth", "iteration": 3, "loss": 0.1, "student_frame_stack": 3}}
    assert checkpoint_student_overrides(ck) == {"terrain.actor_heights": False, "env.frame_stack": 3, "env.num_observations": 141}
    assert checkpoint_student_overrides({"model": ck["model"]}) is None


def test_struct_and_symbols():
    from booster_gym_amd import _lib

    assert "bg_distill_act_gru_own" in _lib.SYMBOLS
    assert _lib.EnvCfg._fields_[-1][0] == "sensor_latency_hi"  # (value 2 reuses the sensor model's fields: none is added behind them)


def test_env_create_checks_sensor_model_2_without_gpu(flat_model):
    """bg_env_create checks the sensor fields before it touches the device: value 2 needs actor_heights and student_frame_stack >= 1, value 1 keeps its
    refusal of actor_heights and its message, the ranges are the existing ones; a consistent struct gets as far as the device check."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    m = flat_model
    d = _lib.ModelDesc(); d.num_bodies, d.num_dofs = 13, 12
    for b in range(13):
        d.parent[b], d.joint_axis[b], d.mass[b] = int(m.parent[b]), int(m.joint_axis[b]), float(m.mass[b])
    model = C.c_void_p()
    assert lib.bg_model_create(C.byref(d), C.byref(model)) == 0
    xy = (C.c_float * 12)(*[0.1 * k for k in range(12)])  # 6 points of the scan
    perceptive = {"actor_heights": 1, "height_scan_points": 6, "terrain_type": 1, "height_scan_xy": C.cast(xy, C.c_void_p)}

    def create(**fields):
        cfg = _lib.EnvCfg(); cfg.num_envs, cfg.decimation, cfg.sim_dt, cfg.sensor_model = 4, 10, 0.002, 2
        for k, v in fields.items():
            if isinstance(v, tuple):
                r = getattr(cfg, k); r.mode, r.a, r.b = v
            else:
                setattr(cfg, k, v)
        env = C.c_void_p()
        return lib.bg_env_create(C.byref(cfg), model, C.byref(env)), lib.bg_last_error()

    try:
        for fields in ({}, {"frame_stack": 3}, dict(perceptive), dict(perceptive, frame_stack=2)):  # no actor_heights, or no student_frame_stack
            rc, msg = create(**fields)
            assert rc == -1 and b"sensor_model 2" in msg and b"actor_heights and student_frame_stack" in msg, (fields, msg)
        rc, msg = create(student_frame_stack=2)  # (the student's row without the perceptive env: the field's own, older refusal)
        assert rc == -1 and b"student_frame_stack needs actor_heights" in msg, msg
        rc, msg = create(**dict(perceptive, sensor_model=1))
        assert rc == -1 and b"sensor_model is not available with actor_heights (bg_obs_assemble writes those rows, and the student's)" in msg, msg
        rc, msg = create(**dict(perceptive, sensor_model=3, student_frame_stack=1))
        assert rc == -1 and b"sensor_model must be 0" in msg, msg
        ok = dict(perceptive, student_frame_stack=1)
        for fields, word in (({"sensor_bias_gravity": (2, 0.0, 1.0)}, b"sensor_bias"), ({"sensor_bias_dof_pos": (1, 0.0, -1.0)}, b"sensor_bias"),
                             ({"sensor_bias_dof_vel": (3, float("inf"), 1.0)}, b"sensor_bias"), ({"sensor_latency_lo": 1.0, "sensor_latency_hi": 0.5}, b"sensor_latency"),
                             ({"sensor_latency_hi": 2.5}, b"sensor_latency"), ({"sensor_latency_hi": float("nan")}, b"sensor_latency")):
            rc, msg = create(**dict(ok, **fields))
            assert rc == -1 and word in msg, (fields, msg)
        if not torch.cuda.is_available():
            for fields in (ok, dict(ok, student_frame_stack=3, frame_stack=2, sensor_bias_gravity=(1, 0.0, 0.05), sensor_latency_lo=0.25, sensor_latency_hi=2.0)):
                rc, msg = create(**fields)
                assert rc == -3 and b"no HIP device" in msg, (fields, msg)
    finally:
        lib.bg_model_destroy(model)
