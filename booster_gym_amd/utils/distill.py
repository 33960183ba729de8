"""Teacher-student distillation of a perceptive actor into a blind one (rsl_rl's `Distillation`, DAgger): a mode beside PPO.

The teacher is an actor trained with terrain.actor_heights: its row is [47 H observations | P height-scan values].  The robot has no height sensor,
so the deployed policy must act on the first 47 H columns alone.  Here the STUDENT acts in the teacher's env (noise, randomisation and curriculum as
in training), the teacher labels every visited row with its mean action, and the student regresses onto the labels:

  rollout   per env step ONE launch for both networks (bg_distill_act: the student samples from columns [0, 47 H), the teacher's mean from all
            47 H + P) and ONE env launch (bg_env_step_to), outputs written in place as in Runner.rollout();
  update    the prefix columns of the B = T N rows once into the student's zero-padded input, then num_epochs full-batch steps: MLPTrainer's
            hidden layers forward, bg_distill_head (output layer + mean squared error + its backward), backward_hidden, the grouped weight
            gradients, the fixed-order finishes, FlatAdam.step (global-norm clip + Adam) over the student's actor parameters at a constant rate; the step
            writes none of the trainer's weight copies, so the WeightClock ticks behind it and the next pass rewrites them (model.WeightCopies).

The student checkpoint is what Runner, play.py, export_model.py and tools/play_oracle.py load under the config with terrain.actor_heights: false and
env.num_observations: 47 H: `actor.*`, `logstd` (fixed at log(student_noise_std)) and an UNTRAINED `critic.*` of that config's shape.

distillation.student_frame_stack: Hs > H gives the student a longer history than its teacher has: a blind policy learns about the ground only from
what its joints and IMU did over the last steps, a perceptive teacher does not need (and with 187 points cannot afford) that history.  The env then
writes a second row per step, the student's [47 Hs] (env.student_frame_stack; the last 47 H columns are the teacher's first 47 H, noise included), the
rollout's launch is bg_distill_act_hist (the student half on its own buffer), the update regresses on buffer["student_obses"], and the checkpoint
re-enters under env.frame_stack: Hs, env.num_observations: 47 Hs.  Absent, null or equal to H: every call is the one described above.

distillation.symmetric_coef: c > 0 adds the mirror-symmetry loss of algorithm.symmetry_loss to the student: an epoch minimises
1 / (A B) sum_r |mu(x_r) - label_r|^2 + c / (A B) sum_r |mu(M_o x_r) - M_a mu(x_r)|^2, M_o / M_a the maps of envs/mirror.py for the student's row
(47 H or 47 Hs columns, the single observation's map tiled over the frames; no scan).  The student's input then holds 2B rows, the batch and behind it
its mirror images (bg_mirror_rows, once per update), the hidden layers and the grouped weight gradients run on 2B rows under the plan of 2B rows, and
the output layer is bg_distill_head_sym.  Nothing but the teacher's labels ties a blind student's left to its right; this term does.

distillation.teacher_action_prob: beta_0 > 0 is DAgger's mixing (Ross et al. 2011): in iteration i the teacher drives each (env, step) with
probability beta_i = beta_0 max(0, 1 - i / teacher_action_iterations) (teacher_action_iterations: 0 = constant), the student otherwise; the rollout's
launch is bg_distill_act_mix, on the same buffers.  teacher_action_noise: a teacher-driven step carries the student's exploration noise (the very
draw the student would have used), false: the teacher's mean alone.  The update is untouched: labels are the teacher's mean on every visited row,
whoever drove.  With both keys at their defaults every launch, random stream, buffer, log name and checkpoint key is what it is without them.

distillation.student_memory: H = 128 or 256 makes the student recurrent (rsl_rl's recurrent student): `memory`, a torch.nn.GRUCell(47, H), reads the
newest single observation (columns [0, 47) of the teacher's row) and the actor's MLP reads its new state h' instead of the observation.  The state
[N][H] is zero at begin(), advances in every env step whoever drives (bg_distill_act_gru, in place; an env the step before reset enters with h = 0,
the frame stack's rule) and carries across iterations; the update back-propagates through the iteration's T steps from the state h0 stored at its
start (the gradient is truncated there): model.GRUTrainer around the trunk's MLPTrainer.  The optimiser holds memory.* and actor.*; the checkpoint
carries memory.* and re-enters under algorithm.actor_memory: H.  0 (the default, also absent): everything above, unchanged.

distillation.student_sensors: {bias: {gravity, ang_vel, dof_pos, dof_vel}, latency_steps: [lo, hi]} (the `sensors:` section without `enabled`, its
meaning, defaults and rules: utils/sensors.py) distils the student under the sensor model it will meet on the robot while the teacher keeps acting
and labelling on its clean row: the env's last launch sends the student's row, and only that row, through bg_obs_sensor's rule (bg_env_cfg.sensor_model
= 2, inside bg_obs_assemble).  The student's row is then no prefix of the teacher's, so it always has a buffer of its own (env.student_frame_stack
also at Hs = H; bg_distill_act_hist / _mix, a recurrent student's cell through bg_distill_act_gru_own), the checkpoint's entry carries the section, and
the student re-enters under sensors.enabled: true with the same bias and latency_steps.  Absent or null: everything above, unchanged.
"""
import argparse
import ctypes
import math
import os
import random
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ..envs import TASKS
from ..envs.mirror import mirror_maps
from ..envs.t1 import MAX_CRITIC_INPUT, MAX_FRAME_STACK, frame_stack_of, privileged_extras_of
from .buffer import ExperienceBuffer
from .config import load_cfg
from .estimator import estimator_enabled
from .model import CRITIC_HIDDEN, ActorCritic, WeightClock, check_hidden, hidden_of, layer_descriptors, pad_input
from .optim import FlatAdam
from .recorder import Recorder
from .runner import hidden_widths
from .sensors import sensors_as_section, sensors_section
from .supervised import SupervisedTrainer
from .terrain import actor_heights_of, height_scan_points
from .utils import mirror_rows

DEFAULTS = {"teacher_checkpoint": None, "student_hidden": [256, 128, 128], "num_epochs": 5, "learning_rate": 1.0e-3, "max_grad_norm": 1.0,
            "student_noise_std": 0.1, "student_frame_stack": None, "symmetric_coef": 0.0, "teacher_action_prob": 0.0, "teacher_action_iterations": 0,
            "teacher_action_noise": True, "student_memory": 0, "student_sensors": None}
STUDENT_MEMORY = (0, 128, 256)  # the widths of the recurrent student's cell the kernels take (0: no memory)


class DistillCfg(NamedTuple):
    teacher_checkpoint: Optional[str]
    student_hidden: tuple
    num_epochs: int
    learning_rate: float
    max_grad_norm: float
    student_noise_std: float


def distillation_cfg(cfg, world_size=1):
    """The `distillation:` section of a config as a DistillCfg (absent keys: DEFAULTS), or ValueError naming the key.  Pure: no tensors, no device.
    The mode needs a perceptive teacher's env (terrain.actor_heights), runs without observation normalisation and on one rank."""
    sec = cfg.get("distillation")
    if sec is None:
        raise ValueError("the config has no `distillation` section: the distillation mode is unavailable (envs/T1.yaml ships one)")
    if not isinstance(sec, dict):
        raise ValueError(f"distillation must be a mapping of its keys ({', '.join(DEFAULTS)}), got {sec!r}")
    unknown = sorted(set(sec) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"distillation.{unknown[0]} is not a key of the section ({', '.join(DEFAULTS)})")
    if not actor_heights_of(cfg["terrain"]):
        raise ValueError("distillation needs terrain.actor_heights: true (with terrain.measure_heights: the config the teacher was trained under): "
                         "without the height scan in the actor's row there is nothing to distil from")
    if (cfg.get("algorithm", {}) or {}).get("empirical_normalization", False):
        raise ValueError("algorithm.empirical_normalization: true is not supported with distillation for now (a teacher trained with it carries "
                         "statistics of its own row, the student's would be others)")
    if estimator_enabled(cfg):
        raise ValueError("estimator.enabled: true is not supported with distillation for now (the student's row would need the estimates of a network "
                         "the Distiller does not train): set estimator.enabled to false")
    if int(world_size) != 1:
        raise ValueError(f"distillation runs on one rank (WORLD_SIZE = {world_size}): data parallelism is out of scope")
    student_memory_of(cfg)  # (ValueError naming the key: its value, and what a recurrent student excludes)
    student_sensors_of(cfg)
    v = dict(DEFAULTS, **sec)
    ck = v["teacher_checkpoint"]
    if ck is not None and not isinstance(ck, str):
        raise ValueError(f"distillation.teacher_checkpoint must be a path or null, got {ck!r}")
    try:
        hidden, _ = check_hidden(v["student_hidden"], CRITIC_HIDDEN)
    except ValueError as e:
        raise ValueError(str(e).replace("algorithm.actor_hidden", "distillation.student_hidden")) from None
    n = v["num_epochs"]
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"distillation.num_epochs must be an integer >= 1, got {n!r}")
    for key in ("learning_rate", "max_grad_norm", "student_noise_std"):
        x = v[key]
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x <= 0:
            raise ValueError(f"distillation.{key} must be a finite number > 0, got {x!r}")
    return DistillCfg(ck, hidden, n, float(v["learning_rate"]), float(v["max_grad_norm"]), float(v["student_noise_std"]))


def student_frame_stack_of(cfg):
    """distillation.student_frame_stack as the number Hs of single observations in the student's row: null or absent = the teacher's env.frame_stack = H.
    Pure.  ValueError naming the key unless it is an integer in H .. MAX_FRAME_STACK whose student config passes the env's own size check: the
    student's critic takes 47 Hs + 14 + P (+ X) columns (P points of terrain.measured_points_x x measured_points_y, X columns of
    env.privileged_extras), MAX_CRITIC_INPUT at most."""
    H = frame_stack_of(cfg)
    sec = cfg.get("distillation")
    Hs = sec.get("student_frame_stack") if isinstance(sec, dict) else None
    if Hs is None:
        return H
    if isinstance(Hs, bool) or not isinstance(Hs, int) or not H <= Hs <= MAX_FRAME_STACK:
        raise ValueError(f"distillation.student_frame_stack = {Hs!r} must be null or an integer from env.frame_stack = {H} (the teacher's) to "
                         f"{MAX_FRAME_STACK}: the student sees the env's last student_frame_stack observations, the teacher's {H} among them")
    P = len(height_scan_points(cfg["terrain"])[1])
    X = privileged_extras_of(cfg)[1]  # (env.privileged_extras: the student's untrained critic has the teacher config's privileged row)
    if _lib.NUM_OBS * Hs + _lib.NUM_PRIV + P + X > MAX_CRITIC_INPUT:
        extras = f" + {X} (env.privileged_extras)" if X else ""
        raise ValueError(f"distillation.student_frame_stack = {Hs}: the student's config (env.frame_stack: {Hs}, terrain.actor_heights: false) has a critic of "
                         f"{_lib.NUM_OBS} x {Hs} + {_lib.NUM_PRIV} + {P} (terrain.measured_points_x x terrain.measured_points_y){extras} = "
                         f"{_lib.NUM_OBS * Hs + _lib.NUM_PRIV + P + X} inputs, above {MAX_CRITIC_INPUT} (the widest first layer of the kernels): a smaller "
                         f"distillation.student_frame_stack, or fewer points of the height scan")
    return Hs


def _key(cfg, key):
    sec = cfg.get("distillation")
    return sec.get(key, DEFAULTS[key]) if isinstance(sec, dict) else DEFAULTS[key]


def _number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)


def symmetric_coef_of(cfg):
    """distillation.symmetric_coef as a float: the weight c of the mirror-symmetry loss on the student's mean, 0 (the default, also absent) = off.
    Pure.  ValueError naming the key unless it is a finite number >= 0."""
    c = _key(cfg, "symmetric_coef")
    if not _number(c) or c < 0:
        raise ValueError(f"distillation.symmetric_coef must be a finite number >= 0 (0: no symmetry loss on the student), got {c!r}")
    return float(c)


def student_memory_of(cfg):
    """distillation.student_memory as the width H of the recurrent student's GRU cell: 0 (the default, also absent) = a memoryless student.  Pure.
    ValueError naming the key unless it is one of STUDENT_MEMORY, and with H > 0 unless env.frame_stack is 1, distillation.student_frame_stack is
    not above the teacher's and distillation.symmetric_coef is 0: the cell reads one observation, and the mirror image of a hidden state is not defined."""
    H = _key(cfg, "student_memory")
    if isinstance(H, bool) or not isinstance(H, int) or H not in STUDENT_MEMORY:
        raise ValueError(f"distillation.student_memory must be one of {', '.join(map(str, STUDENT_MEMORY))} (the width of the student's GRU cell; 0: a "
                         f"memoryless student), got {H!r}")
    if H == 0:
        return 0
    fs = frame_stack_of(cfg)
    if fs != 1:
        raise ValueError(f"distillation.student_memory = {H} needs env.frame_stack: 1 (got {fs}): the cell reads the newest single observation; a frame "
                         "stack in front of it is not supported for now")
    if student_frame_stack_of(cfg) > fs:
        raise ValueError(f"distillation.student_memory = {H} is not supported with distillation.student_frame_stack above the teacher's env.frame_stack "
                         "for now: the memory is the student's history")
    if symmetric_coef_of(cfg) > 0:
        raise ValueError(f"distillation.student_memory = {H} is not supported with distillation.symmetric_coef > 0: the mirror image of a hidden state "
                         "is not defined")
    return H


STUDENT_SENSORS_KEYS = ("bias", "latency_steps")  # the `sensors:` section's keys minus `enabled`


def student_sensors_of(cfg):
    """distillation.student_sensors as a SensorsCfg: the sensor model of the student's row (bias per episode and a sensing delay on its 30 sensor
    columns; the teacher's row stays clean), None with the key absent or null (off).  Pure.  The rules are the `sensors:` section's
    (sensors.sensors_section); every refusal is a ValueError naming distillation.student_sensors.<key>."""
    sec = _key(cfg, "student_sensors")
    if sec is None:
        return None
    if not isinstance(sec, dict):
        raise ValueError(f"distillation.student_sensors must be null or a mapping of its keys ({', '.join(STUDENT_SENSORS_KEYS)}), got {sec!r}")
    return sensors_section(sec, "distillation.student_sensors", STUDENT_SENSORS_KEYS)


def teacher_action_of(cfg):
    """(beta_0, iterations, noise) of DAgger's mixing: distillation.teacher_action_prob in [0, 1] (0, the default: the student always acts),
    teacher_action_iterations (an integer >= 0: beta reaches 0 after that many iterations, 0 = constant) and teacher_action_noise (a bool).  Pure.
    ValueError naming the key of a bad value."""
    b0, n, noise = (_key(cfg, k) for k in ("teacher_action_prob", "teacher_action_iterations", "teacher_action_noise"))
    if not _number(b0) or not 0 <= b0 <= 1:
        raise ValueError(f"distillation.teacher_action_prob must be a number in [0, 1] (the probability with which the teacher acts; 0: never), got {b0!r}")
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"distillation.teacher_action_iterations must be an integer >= 0 (iterations until the probability is 0; 0: constant), got {n!r}")
    if not isinstance(noise, bool):
        raise ValueError(f"distillation.teacher_action_noise must be true or false, got {noise!r}")
    return float(b0), n, noise


def teacher_action_prob_at(beta0, iterations, it):
    """beta of iteration `it`: beta0 max(0, 1 - it / iterations), constant beta0 with iterations = 0."""
    return float(beta0) if not iterations else float(beta0) * max(0.0, 1.0 - it / iterations)


def student_mirror_maps(dof_names, dof_axes, default_dof_pos, frames):
    """(obs_src, obs_sign, act_src, act_sign) of the student's row: `frames` single observations side by side (H, or Hs with
    distillation.student_frame_stack), the single observation's map tiled over them, and no height scan behind them.  mirror_maps' ValueErrors."""
    return mirror_maps(dof_names, dof_axes, default_dof_pos, _lib.NUM_OBS * int(frames), int(frames), None)


def student_overrides(num_observations, student_frame_stack=None, student_memory=None, student_sensors=None):
    """The rule under which a student re-enters Runner / play.py / export_model.py / evaluate.py, written once: the teacher's config without the
    actor's scan, the student's own history when it has one, the row its actor takes, and the sensor model it was distilled under
    (student_sensors: the section {bias, latency_steps} as plain dicts and lists; bg_obs_sensor then writes the row the student trained on).
    student_cfg_overrides derives the arguments from the teacher's config, checkpoint_student_overrides from a student checkpoint."""
    over = {"terrain.actor_heights": False}
    if student_frame_stack is not None:
        over["env.frame_stack"] = int(student_frame_stack)
    over["env.num_observations"] = int(num_observations)
    if student_memory:  # a recurrent student: Runner(test=True) builds its actor behind a GRU cell of that width
        over["algorithm.actor_memory"] = int(student_memory)
    if student_sensors is not None:
        over["sensors.enabled"] = True
        over["sensors.bias"] = dict(student_sensors["bias"])
        over["sensors.latency_steps"] = list(student_sensors["latency_steps"])
    return over


def student_cfg_overrides(cfg):
    """The overrides under which the student checkpoint re-enters Runner / play.py / export_model.py: the teacher's config without the actor's scan,
    and with distillation.student_frame_stack = Hs > H the student's own history."""
    H = int(cfg["env"].get("frame_stack", 1) or 1)
    sc = student_sensors_of(cfg)
    sensors = None if sc is None else sensors_as_section(sc)
    if isinstance(cfg.get("distillation"), dict) and cfg["distillation"].get("student_frame_stack") is not None:
        Hs = student_frame_stack_of(cfg)
        if Hs > H:
            return student_overrides(_lib.NUM_OBS * Hs, Hs, None, sensors)
    return student_overrides(_lib.NUM_OBS * H, None, student_memory_of(cfg) if isinstance(cfg.get("distillation"), dict) else None, sensors)


def checkpoint_student_overrides(checkpoint):
    """student_overrides from a loaded checkpoint dict alone, or None for a checkpoint that is no student's (no "distillation" entry): the frame
    stack from the entry's "student_frame_stack" when present, the row from the width of the actor's first layer."""
    entry = checkpoint.get("distillation")
    if entry is None:
        return None
    sd = checkpoint["model"]
    if "memory.weight_ih" in sd:  # a recurrent student: the row is what its cell reads, the actor takes the cell's state
        return student_overrides(int(sd["memory.weight_ih"].shape[1]), entry.get("student_frame_stack"), int(sd["memory.weight_hh"].shape[1]),
                                 entry.get("student_sensors"))
    return student_overrides(int(sd["actor.0.weight"].shape[1]), entry.get("student_frame_stack"), None, entry.get("student_sensors"))


class Distiller:
    def __init__(self, cfg=None, args=None):
        if cfg is None:
            self._get_args(args)
            cfg = load_cfg(self.args.task)
            for arg in ("num_envs",):
                if getattr(self.args, arg) is not None:
                    cfg["env"][arg] = getattr(self.args, arg)
            for arg in ("seed", "max_iterations", "sim_device", "rl_device"):
                if getattr(self.args, arg) is not None:
                    cfg["basic"][arg] = getattr(self.args, arg)
            if self.args.teacher is not None:
                cfg.setdefault("distillation", {})
                if isinstance(cfg["distillation"], dict):
                    cfg["distillation"]["teacher_checkpoint"] = self.args.teacher
            for arg in ("student_frame_stack", "symmetric_coef", "teacher_action_prob", "teacher_action_iterations", "student_memory"):
                if getattr(self.args, arg) is not None:
                    cfg.setdefault("distillation", {})
                    if isinstance(cfg["distillation"], dict):
                        cfg["distillation"][arg] = getattr(self.args, arg)
        self.cfg = cfg
        cfg["basic"].setdefault("task", "T1")
        cfg["basic"]["rank"] = self.rank = 0
        self.dcfg = distillation_cfg(cfg, int(os.environ.get("WORLD_SIZE", "1")))  # (ValueError before anything is built)
        if not self.dcfg.teacher_checkpoint:
            raise ValueError("distillation.teacher_checkpoint is not set: the path of a checkpoint trained with terrain.actor_heights (distill.py --teacher=PATH)")
        self.symmetric_coef = symmetric_coef_of(cfg)
        self.beta0, self.beta_iterations, self.teacher_noise = teacher_action_of(cfg)
        self.memory = student_memory_of(cfg)  # the width of the recurrent student's GRU cell; 0: none
        Hs, H = student_frame_stack_of(cfg), frame_stack_of(cfg)
        sensors = student_sensors_of(cfg)
        self.student_sensors = None if sensors is None else sensors_as_section(sensors)  # the validated section as plain dicts, lists and floats
        # the student's own row, a second output of the env, through bg_distill_act_hist: a longer history, or the sensor model at any Hs (the
        # student's row is then no prefix of the teacher's)
        self.history = Hs > H or sensors is not None
        if self.history:
            cfg["env"]["student_frame_stack"] = Hs  # (the env's name of it; T1 builds the ring of Hs planes and the third output of its last launch)
        if sensors is not None:
            cfg["env"]["student_sensors"] = self.student_sensors  # (the env's name of it: bg_env_cfg.sensor_model = 2)
        critic_hidden = hidden_widths(cfg)[1]
        self._set_seed()
        task = cfg["basic"]["task"]
        if task not in TASKS:
            raise NameError(f"name {task!r} is not defined")
        self.env = env = TASKS[task](cfg)  # the teacher's env, exactly as Runner builds it
        self.device = dev = cfg["basic"]["rl_device"]
        if torch.device(dev) != torch.device(env.device):
            raise ValueError("rl_device must equal sim_device: the rollout writes simulator outputs straight into the distillation buffers")
        self.student_obs, self.scan = env.scan_obs_offset, env.num_scan_obs  # 47 H columns, then P
        if self.history:
            self.student_obs = env.num_student_obs  # 47 Hs columns of a row of their own
        self.teacher = self._load_teacher(self.dcfg.teacher_checkpoint)
        A = env.num_actions
        self.student = ActorCritic(A, self.student_obs, env.num_privileged_obs, self.dcfg.student_hidden, critic_hidden,
                                   **({"memory_hidden": self.memory} if self.memory else {})).to(dev)
        with torch.no_grad():
            self.student.logstd.fill_(math.log(self.dcfg.student_noise_std))
        self.student.logstd.requires_grad_(False)  # fixed exploration noise of the data-collecting student; not trained
        # only the student's actor is trained: the critic and logstd keep their storage outside the flat Adam buffer
        trained = (list(self.student.memory.parameters()) if self.memory else []) + list(self.student.actor.parameters())
        self.optimizer = FlatAdam(trained, lr=self.dcfg.learning_rate, max_grad_norm=self.dcfg.max_grad_norm)

        T, N = int(cfg["runner"]["horizon_length"]), env.num_envs
        self.T, self.N, self.B = T, N, T * N
        self.buffer = buf = ExperienceBuffer(T, N, dev)
        buf.add_buffer("actions", (A,))
        buf.add_buffer("teacher_mu", (A,))
        buf.add_buffer("obses", (env.num_obs,), extra_rows=1)
        if self.history:
            buf.add_buffer("student_obses", (self.student_obs,), extra_rows=1)
        buf.add_buffer("privileged_obses", (env.num_privileged_obs,), extra_rows=1)
        buf.add_buffer("rewards", ())
        buf.add_buffer("dones", (), dtype=torch.bool)
        buf.add_buffer("time_outs", (), dtype=torch.bool)
        kin = pad_input(self.student_obs)
        self.symmetry = self.symmetric_coef > 0
        rows = 2 * self.B if self.symmetry else self.B  # with the symmetry loss: the batch, then its mirror images (bg_mirror_rows in update())
        if self.symmetry:  # (ValueError for a model without a left / right pairing or with an asymmetric default pose)
            axes = [int(a) for a in env.model.joint_axis if int(a) != 0]
            obs_src, obs_sign, act_src, act_sign = student_mirror_maps(env.dof_names, axes, env.default_dof_pos[0].cpu().numpy(), Hs if self.history else H)
            self._act_mirror = ((ctypes.c_int32 * A)(*[int(v) for v in act_src]), (ctypes.c_float * A)(*[float(v) for v in act_sign]))
            self._obs_mirror = (obs_src.tolist() + [-1] * (kin - len(obs_src)), obs_sign.tolist() + [1.0] * (kin - len(obs_sign)))
        self._student_in = torch.zeros(rows, kin, device=dev)  # (the padded columns stay zero)
        self._clock = WeightClock()  # (of the student's trained parameters; one trainer reads it)
        # the supervised update: the actor's MLPTrainer, with a memory the cell around it (model.GRUTrainer), the statistics [squared errors (, squared
        # mean asymmetries)]; its plan is resolved once, here (a batch the layer kernels cannot take is a ValueError before the first iteration)
        self._sup = SupervisedTrainer("distillation", self.student.actor, self.optimizer, self._clock, rows, kin, n_stats=2 if self.symmetry else 1,
                                      **({"cell": self.student.memory, "steps": T} if self.memory else {}))
        self._sup.resolve_plan()
        if self.memory:
            # the cell's rollout state [N][H] (advanced in place by bg_distill_act_gru, zero at begin()) and the done flags of the previous iteration's
            # last step: the resets of this iteration's step 0
            self.state = torch.zeros(N, self.memory, device=dev)
            self._last_dones = torch.zeros(N, dtype=torch.uint8, device=dev)
            self._gru_desc = (None, None)
        self._losses = torch.zeros(self.dcfg.num_epochs, self._sup.stats.numel(), dtype=torch.float64, device=dev)
        self._act_counter = 0
        self._descs = (None, None, None)
        self.iteration_count = 0
        self.last_loss = self.last_symmetry_loss = float("nan")

    # ------------------------------------------------------------------ config / seed / teacher
    def _get_args(self, args=None):
        parser = argparse.ArgumentParser()
        parser.add_argument("--task", required=True, type=str, help="Name of the task to run.")
        parser.add_argument("--teacher", type=str, help="Path of the perceptive teacher's checkpoint. Overrides distillation.teacher_checkpoint.")
        parser.add_argument("--student_frame_stack", type=int, help="Observation frames of the student's input (at least the teacher's env.frame_stack). "
                            "Overrides distillation.student_frame_stack.")
        parser.add_argument("--symmetric_coef", type=float, help="Weight of the mirror-symmetry loss on the student's mean (0: off). Overrides distillation.symmetric_coef.")
        parser.add_argument("--teacher_action_prob", type=float, help="Probability with which the teacher acts in the rollout (DAgger's mixing; 0: never). "
                            "Overrides distillation.teacher_action_prob.")
        parser.add_argument("--teacher_action_iterations", type=int, help="Iterations over which that probability falls to 0 (0: constant). "
                            "Overrides distillation.teacher_action_iterations.")
        parser.add_argument("--student_memory", type=int, help="Width of the recurrent student's GRU cell (128 or 256; 0: a memoryless student). "
                            "Overrides distillation.student_memory.")
        parser.add_argument("--max_iterations", type=int, help="Number of distillation iterations. Overrides config file if provided.")
        parser.add_argument("--num_envs", type=int, help="Number of environments to create. Overrides config file if provided.")
        parser.add_argument("--sim_device", type=str, help="Device for physics simulation. Overrides config file if provided.")
        parser.add_argument("--rl_device", type=str, help="Device for the networks. Overrides config file if provided.")
        parser.add_argument("--seed", type=int, help="Random seed. Overrides config file if provided.")
        self.args = parser.parse_args(args)

    def _set_seed(self):
        if self.cfg["basic"]["seed"] == -1:
            self.cfg["basic"]["seed"] = int(np.random.randint(0, 10000))
        seed = self.cfg["basic"]["seed"]
        print("Setting seed: {}".format(seed))
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        os.environ["PYTHONHASHSEED"] = str(seed)
        torch.cuda.manual_seed_all(seed)

    def _load_teacher(self, ck):
        env = self.env
        print("Loading teacher from {}".format(ck))
        d = torch.load(ck, map_location=self.device, weights_only=True)
        sd = d["model"]
        if d.get("obs_normalizer") is not None:
            raise ValueError(f"teacher checkpoint {ck} was trained with algorithm.empirical_normalization (it has an \"obs_normalizer\"): not supported "
                             "with distillation for now")
        if any(k.startswith("memory.") for k in sd):
            raise ValueError(f"teacher checkpoint {ck} carries memory.* (a recurrent actor, algorithm.rnn_hidden_size or a recurrent student): the teacher "
                             "of a distillation is a feed-forward perceptive actor")
        a_in = int(sd["actor.0.weight"].shape[1])
        if a_in != env.num_obs:
            raise ValueError(f"teacher checkpoint {ck} has an actor of {a_in} inputs, the env's row has {env.num_obs} (env.num_observations = 47 x "
                             "env.frame_stack + the points of terrain.measured_points_x / measured_points_y): the config must be the teacher's")
        pts = d.get("height_points")
        if pts is None or tuple(pts.shape) != tuple(env.height_points.shape) or not torch.equal(pts.to(env.height_points.device), env.height_points):
            raise ValueError(f"teacher checkpoint {ck} " + ("has no \"height_points\" (it was not trained with terrain.actor_heights)" if pts is None else
                                                            "has other \"height_points\" than the env's terrain.measured_points_x / measured_points_y"))
        teacher = ActorCritic(env.num_actions, a_in, int(sd["critic.0.weight"].shape[1]) - a_in, hidden_of(sd, "actor"), hidden_of(sd, "critic")).to(self.device)
        teacher.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("rnd_predictor.", "rnd_target."))})  # (a teacher trained under rnd.enabled: its curiosity networks stay behind)
        teacher.requires_grad_(False)
        if "curriculum" in d:
            try:
                env.curriculum_prob = d["curriculum"]
            except Exception as e:
                print(f"Failed to load curriculum: {e}")
        if env.terrain.curriculum and "terrain_levels" in d:
            try:
                lv = d["terrain_levels"]
                if tuple(lv.shape) != (env.num_envs,):
                    raise ValueError(f"shape {tuple(lv.shape)}, the env has {env.num_envs} envs")
                env.terrain_levels = lv
            except Exception as e:
                print(f"Failed to load terrain levels: {e!r}")
        return teacher

    def checkpoint_dict(self):
        """The student as a checkpoint of the config with terrain.actor_heights: false and env.num_observations: 47 H (student_cfg_overrides): no
        "height_points", no "optimizer"; the critic is the untrained one built here."""
        d = {"model": self.student.state_dict(), "curriculum": self.env.curriculum_prob,
             "distillation": {"teacher": str(self.dcfg.teacher_checkpoint), "iteration": int(self.iteration_count), "loss": float(self.last_loss)}}
        if self.history and self.env.student_frame_stack > self.env.frame_stack:
            d["distillation"]["student_frame_stack"] = self.env.student_frame_stack
        if self.student_sensors is not None:
            d["distillation"]["student_sensors"] = self.student_sensors
        if self.symmetry:
            d["distillation"]["symmetric_coef"] = self.symmetric_coef
        if self.beta0 > 0:
            d["distillation"]["teacher_action_prob"] = [self.beta0, self.beta_iterations]
        if self.memory:
            d["distillation"]["student_memory"] = self.memory
        if self.env.terrain.curriculum:
            d["terrain_levels"] = self.env.terrain_levels
        return d

    # ------------------------------------------------------------------ one iteration
    def _descriptors(self):
        """bg_mlp_layer_desc arrays of the student's and the teacher's actor on their current parameter storage."""
        lins = [[m for m in net.actor if isinstance(m, torch.nn.Linear)] for net in (self.student, self.teacher)]
        key = tuple(t.data_ptr() for lin in lins for l in lin for t in (l.weight, l.bias))
        if key != self._descs[0]:
            self._descs = (key, layer_descriptors(lins[0]), layer_descriptors(lins[1]))
        return self._descs[1], self._descs[2]

    def teacher_action_prob(self):
        """beta of the current iteration (distillation.teacher_action_prob and teacher_action_iterations): 0 with the key off."""
        return teacher_action_prob_at(self.beta0, self.beta_iterations, self.iteration_count)

    def rollout(self):
        """T env steps with the student's sampled actions (with distillation.teacher_action_prob: the teacher's on a share beta of the rows); every
        visited row and the teacher's mean action on it are kept.  One launch per env step for both networks, its kind chosen once in front of the
        loop (the mixing by beta_0, not by the decayed beta); a recurrent student's also advances the state in place, and an env that the step
        before reset enters with a zero state (dones[n - 1]; at step 0 the previous iteration's last flags)."""
        buf, T, N, p = self.buffer, self.T, self.N, _lib.ptr
        obses, priv, actions, labels, dones = buf["obses"], buf["privileged_obses"], buf["actions"], buf["teacher_mu"], buf["dones"]
        seed = int(self.cfg["basic"]["seed"]) + 1000003  # (Runner's rollout seed of rank 0)
        sd, td = self._descriptors()
        logstd, beta, noise, mt = self.student.logstd, self.teacher_action_prob(), int(self.teacher_noise), self._sup.gru
        sobs = buf["student_obses"] if self.history else obses  # the student's rows: its own with a longer history
        # what the four launches take between the teacher's rows and the outputs: the student's rows, the networks, the noise stream (, the mixing)
        own, nets, rng = (lambda n: (p(sobs[n]), sobs.shape[-1])), (len(sd), sd, len(td), td, self.scan), (lambda: (p(logstd), seed, self._act_counter))
        if mt is not None:  # a recurrent student (beta = 0 is its plain form): the cell between the networks, the resets and the state behind the mixing
            m, h = self.student.memory, self.state
            key = tuple(t.data_ptr() for t in (m.weight_ih, m.weight_hh, m.bias_ih, m.bias_hh))
            if key != self._gru_desc[0]:
                self._gru_desc = (key, self.student.gru_descriptor())
            gnets = (len(td), td, self.scan, self._gru_desc[1], len(sd), sd)
            tail = lambda n: gnets + rng() + (beta, noise, p(mt.rollout_reset(n, self._last_dones, dones)), p(h), p(h))
            # (the cell's 47 inputs from the student's own row where it has one: the sensor model)
            name, mid = ("bg_distill_act_gru_own", lambda n: own(n) + tail(n)) if self.history else ("bg_distill_act_gru", tail)
        elif self.beta0 > 0:  # DAgger's mixing: one launch of its own kind on the same buffers
            name, mid = "bg_distill_act_mix", lambda n: own(n) + nets + rng() + (beta, noise)
        elif self.history:
            name, mid = "bg_distill_act_hist", lambda n: own(n) + nets + rng()
        else:
            name, mid = "bg_distill_act", lambda n: nets + rng()
        launch, student_obs = getattr(_lib.load(), name), (lambda n: {"student_obs": sobs[n + 1]}) if self.history else (lambda n: {})
        with torch.no_grad():
            if mt is not None:
                mt.rollout_begin(h, self._last_dones)  # the state the update's recurrence starts from, step 0's resets
            for n in range(T):
                _lib.check(launch(N, p(obses[n]), obses.shape[-1], *mid(n), None, p(actions[n]), p(labels[n]), _lib.current_stream_ptr()), name)
                self._act_counter += 1
                self.env.step_to(actions[n], obses[n + 1], priv[n + 1], buf["rewards"][n], dones[n], buf["time_outs"][n], **student_obs(n))
            if mt is not None:
                mt.rollout_end(dones, self._last_dones)

    def update(self):
        """num_epochs full-batch behaviour-cloning steps on the rollout's rows.  Returns the per-epoch mean losses (float64 device tensor: the loss
        each step's gradient was taken of); with distillation.symmetric_coef the per-epoch mean squared asymmetries are left in symmetry_losses."""
        B, A = self.B, self.env.num_actions
        target = self.buffer["teacher_mu"].reshape(B, A)
        symmetry = (self.symmetric_coef, self._act_mirror) if self.symmetry else None
        with torch.no_grad():
            rows = self.buffer["student_obses" if self.history else "obses"][: self.T].reshape(B, -1)
            self._student_in[:B, : self.student_obs].copy_(rows[:, : self.student_obs])
            if self.symmetry:  # rows [B, 2B): the mirror images M_o x of the batch (the padded columns stay zero)
                mirror_rows(self._student_in[:B], self._student_in[B:], *self._obs_mirror)
            for e in range(self.dcfg.num_epochs):
                self._sup.step(self._student_in, target, symmetry)
                self._losses[e].copy_(self._sup.stats)
        if self.symmetry:
            self.symmetry_losses = self._losses[:, 1] / float(A * B)
        return self._losses[:, 0] / float(A * B)

    def iteration(self):
        self.rollout()
        losses = self.update()
        self.buffer.roll()
        self.iteration_count += 1
        return losses

    # ------------------------------------------------------------------ entry point
    def begin(self, recorder=None):
        self.recorder = recorder if recorder is not None else Recorder(self.cfg, rank=0)
        obs, infos = self.env.reset()
        self.buffer["obses"][0].copy_(obs)
        self.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
        if self.history:
            self.buffer["student_obses"][0].copy_(infos["student_obs"])
        if self.memory:
            self.state.zero_()
            self._last_dones.zero_()

    def train_iteration(self, it):
        beta = self.teacher_action_prob()  # (of the iteration about to run)
        losses = self.iteration()
        if self.symmetry:
            self.last_loss, self.last_symmetry_loss = (float(v) for v in (self._losses[-1] / float(self.env.num_actions * self.B)).tolist())  # (one host read)
        else:
            self.last_loss = float(losses[-1].item())  # (one host read per iteration)
        self.recorder.record_episode_statistics(self.env, self.env.reward_names, it)
        stats = {"distill/behaviour_loss": self.last_loss}
        if self.symmetry:
            stats["distill/symmetry_loss"] = self.last_symmetry_loss
        if self.beta0 > 0:
            stats["distill/teacher_action_prob"] = beta
        if self.env.terrain.curriculum:
            stats["terrain/mean_level"] = float(self.env.terrain_level_sum().item()) / self.env.num_envs
        self.recorder.record_statistics(stats, it)
        if (it + 1) % self.cfg["runner"]["save_interval"] == 0:
            self.recorder.save(self.checkpoint_dict(), it + 1)

    def train(self):
        self.begin()
        max_it = self.cfg["basic"]["max_iterations"]
        for it in range(max_it):
            self.train_iteration(it)
            print("distillation: {}/{}  behaviour loss {:.6f}".format(it + 1, max_it, self.last_loss))
        if max_it % self.cfg["runner"]["save_interval"]:
            self.recorder.save(self.checkpoint_dict(), max_it)
