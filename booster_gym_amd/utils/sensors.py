"""Sensor model of the actor's observations (IsaacLab's NoiseModelWithAdditiveBias, and a sensing delay): the `sensors:` section of a config.

The env's white noise (noise.gravity / ang_vel / dof_pos / dof_vel) is drawn fresh at every policy step inside the env-step kernels.  This section adds
what stays put for an episode, in one launch of its own (bg_obs_sensor, csrc/bg_sim.hip) behind them:

    bias.<group>    an additive offset per column of the group (gravity: columns 0-2, ang_vel: 3-5, dof_pos: 11-22, dof_vel: 23-34 of the single
                    observation), drawn once per env per episode in physical units from the reference's {range, operation, distribution} entry and
                    multiplied by the group's normalization.* factor, as the group's white noise is;
    latency_steps   [lo, hi] in policy steps, 0 <= lo <= hi <= 2: one delay lam per env per episode, uniform in [lo, hi) (lam = lo when lo == hi); the
                    30 sensor columns of every frame are read lam steps late, linearly interpolated between the two stored observations around it,
                    and never from before the env's last reset.

Commands, the gait clock and the last actions are the controller's own values: neither bias nor latency.  With `enabled` false, null or the section
absent nothing else of the section is read and nothing else in this file is used.
"""
import math
from typing import NamedTuple, Optional, Tuple

from .terrain import actor_heights_of

GROUPS = ("gravity", "ang_vel", "dof_pos", "dof_vel")  # the order of bg_env_cfg.sensor_bias_* and of the columns
# the 30 sensor columns of the 47-wide single observation, in column order: sensor column s = c for c < 6, c - 5 for 11 <= c <= 34
GROUP_COLUMNS = {"gravity": tuple(range(0, 3)), "ang_vel": tuple(range(3, 6)), "dof_pos": tuple(range(11, 23)), "dof_vel": tuple(range(23, 35))}
SENSOR_COLUMNS = tuple(c for g in GROUPS for c in GROUP_COLUMNS[g])
NUM_SENSOR_COLUMNS = len(SENSOR_COLUMNS)
MAX_LATENCY_STEPS = 2  # BG_MAX_SENSOR_LATENCY: the env's ring holds env.frame_stack + ceil(hi) planes
RS_SENSOR, RS_SENSOR_RESET, RS_SENSOR_LATENCY = 640, 656, 8  # csrc/bg_rng.h: bias of column s at entry s & 3 of stream + (s >> 2), lam at entry 0 of + 8
BIAS_KEYS = ("range", "operation", "distribution")
DEFAULTS = {"enabled": False, "bias": {g: None for g in GROUPS}, "latency_steps": [0.0, 0.0]}


class SensorsCfg(NamedTuple):
    bias: Tuple[Optional[dict], ...]  # per group of GROUPS: None, or the entry {range: [a, b], operation: "additive", distribution}
    latency_steps: Tuple[float, float]

    @property
    def extra_planes(self):
        """Planes of the env's observation ring beyond env.frame_stack: ceil(hi)."""
        return int(math.ceil(self.latency_steps[1]))


def sensors_enabled(cfg):
    """sensors.enabled of a config (the section absent or null, the key absent, null or false: False), or ValueError naming the key.  Pure."""
    sec = cfg.get("sensors")
    if sec is None:
        return False
    if not isinstance(sec, dict):
        raise ValueError(f"sensors must be a mapping of its keys ({', '.join(DEFAULTS)}), got {sec!r}")
    on = sec.get("enabled", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"sensors.enabled must be true or false, got {on!r}")
    return on


def _number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)


def _bias_entry(group, entry, prefix="sensors"):
    key = f"{prefix}.bias.{group}"
    if entry is None:
        return None
    if not isinstance(entry, dict):
        raise ValueError(f"{key} must be null or an entry {{range: [a, b], operation: additive, distribution: gaussian | uniform}}, got {entry!r}")
    unknown = sorted(set(entry) - set(BIAS_KEYS))
    if unknown:
        raise ValueError(f"{key}.{unknown[0]} is not a key of the entry ({', '.join(BIAS_KEYS)})")
    if entry.get("operation") != "additive":
        raise ValueError(f"{key}.operation must be \"additive\" (a bias is an offset), got {entry.get('operation')!r}")
    dist = entry.get("distribution")
    if dist not in ("gaussian", "uniform"):
        raise ValueError(f"{key}.distribution must be \"gaussian\" (range = mean, std) or \"uniform\" (range = low, high), got {dist!r}")
    rng = entry.get("range")
    if not isinstance(rng, (list, tuple)) or len(rng) != 2 or not all(_number(x) for x in rng):
        raise ValueError(f"{key}.range must be two finite numbers, got {rng!r}")
    if dist == "gaussian" and rng[1] < 0:
        raise ValueError(f"{key}.range = {list(rng)!r}: the std of a gaussian entry must be >= 0")
    return {"range": [float(rng[0]), float(rng[1])], "operation": "additive", "distribution": dist}


def sensors_cfg(cfg):
    """The `sensors:` section of a config as a SensorsCfg (absent keys: DEFAULTS), None with the key off or the section absent ("off": nothing else of
    the section is read then), or ValueError naming the key.  Pure: no tensors, no device."""
    if not sensors_enabled(cfg):
        return None
    parsed = sensors_section(cfg["sensors"], "sensors", tuple(DEFAULTS))
    if actor_heights_of(cfg["terrain"]):
        raise ValueError("sensors.enabled is not available with terrain.actor_heights: true: those rows, and a distillation's student row with them, "
                         "are written by bg_obs_assemble, which knows nothing of the sensor model")
    return parsed


def sensors_section(sec, prefix, keys):
    """A mapping {bias: {gravity, ang_vel, dof_pos, dof_vel}, latency_steps: [lo, hi]} as a SensorsCfg (absent keys: DEFAULTS), or ValueError naming
    `prefix`.<key>.  keys: the keys the mapping may hold.  The rules of the `sensors:` section, written once for it and for
    distillation.student_sensors (utils/distill.py).  Pure."""
    unknown = sorted(set(sec) - set(keys))
    if unknown:
        raise ValueError(f"{prefix}.{unknown[0]} is not a key of the section ({', '.join(keys)})")
    bias = sec.get("bias")
    if bias is None:
        bias = {}
    if not isinstance(bias, dict):
        raise ValueError(f"{prefix}.bias must be null or a mapping of {', '.join(GROUPS)}, got {bias!r}")
    unknown = sorted(set(bias) - set(GROUPS))
    if unknown:
        raise ValueError(f"{prefix}.bias.{unknown[0]} is not a group of sensor columns ({', '.join(GROUPS)})")
    entries = tuple(_bias_entry(g, bias.get(g), prefix) for g in GROUPS)
    lat = sec.get("latency_steps", DEFAULTS["latency_steps"])
    if lat is None:
        lat = DEFAULTS["latency_steps"]
    if not isinstance(lat, (list, tuple)) or len(lat) != 2 or not all(_number(x) for x in lat) or not 0 <= lat[0] <= lat[1] <= MAX_LATENCY_STEPS:
        raise ValueError(f"{prefix}.latency_steps must be [lo, hi] in policy steps with 0 <= lo <= hi <= {MAX_LATENCY_STEPS}, got {lat!r}")
    return SensorsCfg(entries, (float(lat[0]), float(lat[1])))


def sensors_as_section(sc):
    """A SensorsCfg as plain dicts, lists and floats: {bias: {group: entry or None}, latency_steps: [lo, hi]} (a checkpoint's entry, a config's
    `sensors.bias` and `sensors.latency_steps`)."""
    return {"bias": {g: (None if e is None else {"range": [float(e["range"][0]), float(e["range"][1])], "operation": e["operation"],
                                                  "distribution": e["distribution"]}) for g, e in zip(GROUPS, sc.bias)},
            "latency_steps": [float(sc.latency_steps[0]), float(sc.latency_steps[1])]}
