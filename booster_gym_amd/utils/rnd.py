"""Curiosity by random network distillation (rsl_rl's `rnd_cfg`; Burda et al. 2018, Schwarke et al. 2023 for legged robots): the `rnd:` section of a
config and the pieces a Runner adds under it.

Two MLPs read a state row s: a `target` network, random and never trained, and a `predictor` trained to reproduce the target's output.  Both end in
the 12-wide output layer of every fused head and rollout launch of this build, so the embedding is 12 wide (rsl_rl's num_outputs is not configurable
here; utils/estimator.py made the same choice).  After env step t the raw intrinsic reward of env e is

    rho[t][e] = sqrt(sum_j (predictor_j(s) - target_j(s))^2),        s = the state AFTER the step, row t + 1 of the buffer's streams,

zero where dones[t][e] is set (the successor row opens the next episode), and GAE sees rewards[t][e] + w / sigma x rho[t][e]: ONE launch per env step
(bg_rnd_reward, csrc/bg_actor_mlp.hip) behind the env step writes the predictor's labels, rho and the in-place add.  The networks read the RAW rows,
also under algorithm.empirical_normalization.

sigma is the reward normaliser's: the running (mean, variance, count) of rho over the rows without dones, float64 on the device, initial state
(0, 1, 0), sigma = sqrt(var) + algorithm.normalization_eps; the mean is not subtracted.  It is utils/value_norm.py's ValueNormalizer as it stands (the
same state, the same merge launch bg_value_norm_update, the same fp32 triple), fed with the sums of rho instead of the returns'.  It moves once per
PPO iteration behind the last optimiser step, so the rollout of iteration i divides by the statistics of iterations < i.

The predictor's update is utils/supervised.py's, on an optimiser and a WeightClock of its own.  With `enabled` false or the section absent nothing
else in this file is used.
"""
import hashlib
import math
from typing import NamedTuple, Optional

from .. import _lib

RND_WIDTH = _lib.NUM_DOFS  # the embedding: the 12 columns of every fused output layer
MAX_STATE = 480            # BG_ACTOR_MAX_INPUT (envs/t1.py's MAX_ACTOR_INPUT): the widest first layer of the rollout's launches
STATES = ("critic", "actor")
DEFAULTS = {"enabled": False, "weight": None, "weight_schedule": None, "state": "critic", "predictor_hidden": [256, 128], "target_hidden": [256, 128],
            "num_epochs": 1, "learning_rate": 1.0e-3, "max_grad_norm": 1.0, "reward_normalization": True}
SCHEDULE_KEYS = ("mode", "initial_step", "final_step", "final_value")
ENTRY_POINTS = ("bg_rnd_reward",)  # what the section adds to the library's calls


class RndSchedule(NamedTuple):
    initial_step: int
    final_step: int
    final_value: float


class RndCfg(NamedTuple):
    weight: float
    schedule: Optional[RndSchedule]  # None: constant
    state: str                       # "critic": [obs | privileged_obs]; "actor": obs
    width: int                       # the state row's columns
    predictor_hidden: tuple
    target_hidden: tuple
    num_epochs: int
    learning_rate: float
    max_grad_norm: float
    reward_normalization: bool


def rnd_enabled(cfg):
    """rnd.enabled of a config (the section absent or null, the key absent, null or false: False), or ValueError naming the key.  Pure."""
    sec = cfg.get("rnd")
    if sec is None:
        return False
    if not isinstance(sec, dict):
        raise ValueError(f"rnd must be a mapping of its keys ({', '.join(DEFAULTS)}), got {sec!r}")
    on = sec.get("enabled", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"rnd.enabled must be true or false, got {on!r}")
    return on


def _number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)


def _step(x):
    return not isinstance(x, bool) and isinstance(x, int) and x >= 0


def rnd_cfg(cfg, world_size=1):
    """The `rnd:` section of a config as an RndCfg (absent keys: DEFAULTS), None with the key off or the section absent ("off": nothing else of the
    section is read then), or ValueError naming the key.  Pure: no tensors, no device."""
    if not rnd_enabled(cfg):
        return None
    from .model import CRITIC_HIDDEN, check_hidden

    sec = cfg["rnd"]
    unknown = sorted(set(sec) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"rnd.{unknown[0]} is not a key of the section ({', '.join(DEFAULTS)})")
    v = dict(DEFAULTS, **sec)
    w = v["weight"]
    if not _number(w) or w < 0:
        raise ValueError(f"rnd.weight must be a finite number >= 0 when rnd.enabled is on (there is no default: nobody has measured one), got {w!r}")
    sch = v["weight_schedule"]
    if sch is not None:
        if not isinstance(sch, dict):
            raise ValueError(f"rnd.weight_schedule must be null or a mapping of {', '.join(SCHEDULE_KEYS)}, got {sch!r}")
        unknown = sorted(set(sch) - set(SCHEDULE_KEYS))
        if unknown:
            raise ValueError(f"rnd.weight_schedule.{unknown[0]} is not a key of the schedule ({', '.join(SCHEDULE_KEYS)})")
        if sch.get("mode") != "linear":
            raise ValueError(f"rnd.weight_schedule.mode must be \"linear\" (the one schedule there is; a constant weight is weight_schedule: null), got {sch.get('mode')!r}")
        for key in ("initial_step", "final_step"):
            if not _step(sch.get(key)):
                raise ValueError(f"rnd.weight_schedule.{key} must be an integer >= 0 (a PPO iteration), got {sch.get(key)!r}")
        if sch["final_step"] <= sch["initial_step"]:
            raise ValueError(f"rnd.weight_schedule.final_step = {sch['final_step']} must be above rnd.weight_schedule.initial_step = {sch['initial_step']}")
        fv = sch.get("final_value")
        if not _number(fv) or fv < 0:
            raise ValueError(f"rnd.weight_schedule.final_value must be a finite number >= 0, got {fv!r}")
        sch = RndSchedule(int(sch["initial_step"]), int(sch["final_step"]), float(fv))
    state = v["state"]
    if not isinstance(state, str) or state not in STATES:
        raise ValueError(f"rnd.state must be \"critic\" (the row [observations | privileged observations]) or \"actor\" (the observations), got {state!r}")
    env = cfg["env"]
    width = int(env["num_observations"]) + (int(env["num_privileged_obs"]) if state == "critic" else 0)
    if width > MAX_STATE:
        raise ValueError(f"rnd.state = {state!r}: the state row has {width} columns, above {MAX_STATE} (BG_ACTOR_MAX_INPUT, the widest first layer of the "
                         "rollout's launches)" + ("; rnd.state: \"actor\" reads the observations only" if state == "critic" else ""))
    hidden = {}
    split = int((cfg.get("parallel", {}) or {}).get("gemm_split", 0) or 0)
    for key in ("predictor_hidden", "target_hidden"):
        try:
            hidden[key], _ = check_hidden(v[key], CRITIC_HIDDEN)
            if split and key == "predictor_hidden":  # (the target is never trained: no layer kernel of the update runs on it)
                check_hidden(hidden[key], CRITIC_HIDDEN, split)
        except ValueError as e:
            raise ValueError(str(e).replace("algorithm.actor_hidden", f"rnd.{key}")) from None
    n = v["num_epochs"]
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"rnd.num_epochs must be an integer >= 1, got {n!r}")
    for key in ("learning_rate", "max_grad_norm"):
        x = v[key]
        if not _number(x) or x <= 0:
            raise ValueError(f"rnd.{key} must be a finite number > 0, got {x!r}")
    rn = v["reward_normalization"]
    if not isinstance(rn, bool):
        raise ValueError(f"rnd.reward_normalization must be true or false, got {rn!r}")
    if int(world_size) != 1:
        raise ValueError(f"rnd.enabled runs on one rank (WORLD_SIZE = {world_size}): data parallelism is out of scope for now")
    return RndCfg(float(w), sch, state, width, hidden["predictor_hidden"], hidden["target_hidden"], n, float(v["learning_rate"]), float(v["max_grad_norm"]), rn)


def weight_at(rnd, iteration):
    """The weight of PPO iteration `iteration` (0-based, counted over the whole run: the counter is saved with the checkpoint): rnd.weight up to
    initial_step, linear to final_value at final_step, final_value behind it; the constant rnd.weight without a schedule."""
    s = rnd.schedule
    if s is None or iteration <= s.initial_step:
        return rnd.weight
    if iteration >= s.final_step:
        return s.final_value
    return rnd.weight + (s.final_value - rnd.weight) * (iteration - s.initial_step) / (s.final_step - s.initial_step)


def merge_f64(state, batch):
    """The reward normaliser's merge on the host, in float64: state = (mean, population variance, count), batch = (sum, sum of squares, count) of the
    iteration's rho over the rows without dones; Chan et al.'s rule, as bg_value_norm_update applies it.  A batch of count 0 leaves the state."""
    mean, var, n = (float(x) for x in state)
    s, ss, nb = (float(x) for x in batch)
    if nb <= 0:
        return mean, var, n
    mb = s / nb
    vb = max(ss / nb - mb * mb, 0.0)
    tot, delta = n + nb, mb - mean
    return mean + delta * nb / tot, (var * n + vb * nb + delta * delta * n * nb / tot) / tot, tot


def module_seed(seed):
    """The seed of the generator that initialises both networks, from (basic.seed, "rnd"): the global generator's draws stay as without the key."""
    return int.from_bytes(hashlib.sha256(f"{int(seed)}:rnd".encode()).digest()[:8], "little") & 0x7FFFFFFFFFFFFFFF


class RndTrainer:
    """What rnd.enabled adds to a Runner behind the model's two modules and the buffer's two streams: the descriptors of the rollout's launch, the
    reward normaliser (ValueNormalizer as it stands; None with reward_normalization false), the predictor's supervised update (SupervisedTrainer on
    `optimizer` under `clock`), the iteration counter of the weight's schedule and the four log scalars (device, float64)."""

    def __init__(self, rnd, model, optimizer, clock, T, N, num_obs, eps, device):
        import torch

        from .model import pad_input
        from .supervised import SupervisedTrainer
        from .value_norm import ValueNormalizer

        self.rnd, self.model, self.optimizer, self.T, self.N, self.num_obs = rnd, model, optimizer, int(T), int(N), int(num_obs)
        B = self.T * self.N
        self.iteration = 0  # PPO iterations begun (the schedule's clock; saved with the checkpoint)
        self.weight = weight_at(rnd, 0)  # ... and the weight of the rollout in flight
        self.norm = ValueNormalizer(eps, device) if rnd.reward_normalization else None
        self.eps = float(eps)
        self._mom_scratch = torch.zeros(_lib.OBS_MOMENTS_MAX_GROUPS * 2, dtype=torch.float64, device=device)
        self._sums = self.norm.sums if self.norm is not None else torch.zeros(6, dtype=torch.float64, device=device)
        self.x = torch.zeros(B, pad_input(rnd.width), device=device)  # (the padded columns stay zero)
        self.loss = torch.zeros(1, dtype=torch.float64, device=device)  # the last epoch's SSE / (12 B): rnd/loss
        self.log = torch.zeros(4, dtype=torch.float64, device=device)   # rnd/intrinsic_reward, rnd/weight, rnd/reward_std, rnd/loss
        self.sup = SupervisedTrainer("rnd.enabled", model.rnd_predictor, optimizer, clock, B, self.x.shape[1])
        self._key, self._descs = None, None
        self.resolve_plan()  # (a batch outside the layer kernels' range is a ValueError here, not at the first update)

    def resolve_plan(self):
        from .model import MLPTrainer

        kin, hidden = self.x.shape[1], list(self.rnd.predictor_hidden)
        if MLPTrainer.SPLIT and (kin > 256 or any(w > 256 for w in hidden[:-1])):
            raise ValueError(f"parallel.gemm_split / BG_GEMM_SPLIT runs split-bf16 layer kernels that take layer inputs of 64, 128 or 256 columns only; the "
                             f"RND state pads to {kin} and rnd.predictor_hidden = {hidden} (use gemm_split 0)")
        return self.sup.resolve_plan()

    def begin_rollout(self):
        """The weight of this iteration's rollout (the schedule's clock then ticks)."""
        self.weight = weight_at(self.rnd, self.iteration)
        self.iteration += 1

    def _descriptors(self):
        from .model import layer_descriptors
        import torch

        lins = [[m for m in net if isinstance(m, torch.nn.Linear)] for net in (self.model.rnd_target, self.model.rnd_predictor)]
        key = tuple(t.data_ptr() for lin in lins for l in lin for t in (l.weight, l.bias))
        if key != self._key:  # descriptors of the current parameter storage (the optimiser moves the predictor's into its flat buffer once)
            for lin in lins:
                for l in lin:
                    if not (l.weight.is_contiguous() and l.bias.is_contiguous() and l.weight.is_cuda):
                        raise RuntimeError("bg_rnd_reward needs contiguous CUDA parameters")
            self._descs, self._key = (layer_descriptors(lins[0]), len(lins[0]), layer_descriptors(lins[1]), len(lins[1])), key
        return self._descs

    def reward(self, obs, priv, dones, target_out, intrinsic, rewards):
        """ONE launch on the current stream, behind the env step that wrote these rows: obs [N][num_obs] and priv [N][num_privileged_obs] the state
        after the step, dones / rewards [N] the step's, target_out [N][12] and intrinsic [N] the buffer's rows of the step."""
        td, nt, pd, np_ = self._descriptors()
        crit = self.rnd.state == "critic"
        _lib.check(_lib.load().bg_rnd_reward(obs.shape[0], _lib.ptr(obs), obs.shape[-1], _lib.ptr(priv) if crit else None, priv.shape[-1] if crit else 0, nt, td, np_, pd,
                                             _lib.ptr(dones), None if self.norm is None else _lib.ptr(self.norm.stats), float(self.weight), _lib.ptr(target_out),
                                             _lib.ptr(intrinsic), _lib.ptr(rewards), _lib.current_stream_ptr()), "bg_rnd_reward")

    def update(self, obses, priv, dones, targets, intrinsic):
        """Behind the last PPO optimiser step of the iteration, on the current stream: rnd.num_epochs full-batch Adam steps of
        L = 1 / (12 B) sum |predictor(s) - target(s)|^2 on the successor rows obses [T][N][num_obs] / priv [T][N][npv] (rows 1 .. T of the buffer) with
        the labels the rollout stored; then the reward normaliser's move: the fixed-order float64 sums of intrinsic [T][N] (bg_obs_moments on its one
        column; rows with dones hold zero and are not counted) merged on the device (bg_value_norm_update).  No host read; leaves the log scalars."""
        import torch

        B, no = self.x.shape[0], self.num_obs
        self.resolve_plan()
        self.x.view(self.T, self.N, -1)[:, :, :no].copy_(obses)
        if self.rnd.state == "critic":
            self.x.view(self.T, self.N, -1)[:, :, no : self.rnd.width].copy_(priv)
        for _ in range(self.rnd.num_epochs):
            self.sup.step(self.x, targets.reshape(B, RND_WIDTH))
        torch.mul(self.sup.stats, 1.0 / (RND_WIDTH * B), out=self.loss)
        s = self._sums
        _lib.check(_lib.load().bg_obs_moments(B, _lib.ptr(intrinsic), 1, 1, None, 0, 0, _lib.ptr(s[3:]), _lib.ptr(s[4:]), _lib.ptr(self._mom_scratch),
                                              _lib.current_stream_ptr()), "bg_obs_moments")
        s[5:6].copy_(float(B) - dones.sum().double())  # (an integer sum: exact, in any order)
        log = self.log
        torch.div(s[3:4], torch.clamp(s[5:6], min=1.0), out=log[0:1])  # the iteration's mean raw rho over the rows without dones
        log[1].fill_(self.weight)
        log[3:4].copy_(self.loss)
        if self.norm is not None:
            self.norm.update_from()
            torch.sqrt(self.norm.state[1:2], out=log[2:3])
        else:
            log[2].fill_(1.0)

    # ---- checkpoint
    def state_dict(self):
        n = self.norm
        return {"optimizer": self.optimizer.state_dict(), "normalizer": None if n is None else n.state_dict(), "iteration": int(self.iteration),
                "state": self.rnd.state, "predictor_hidden": list(self.rnd.predictor_hidden), "target_hidden": list(self.rnd.target_hidden)}

    def load_state_dict(self, entry):
        self.iteration = int(entry.get("iteration", 0))
        self.weight = weight_at(self.rnd, self.iteration)
        if self.norm is not None and entry.get("normalizer") is not None:
            self.norm.load_state_dict(entry["normalizer"])
        try:
            self.optimizer.load_state_dict(entry["optimizer"])
        except Exception as e:
            print(f"Failed to load the RND predictor's optimizer: {e}")


def check_rnd_checkpoint(ck, model_dict, rnd):
    """A training Runner's _load: checkpoint `ck` (loaded: model_dict) against the config's RndCfg `rnd` (None: off).  ValueError naming rnd.enabled /
    rnd.state / rnd.predictor_hidden / rnd.target_hidden unless both are without the networks or both carry the same ones.  (Runner(test=True), play,
    evaluation and export never evaluate these networks and do not call this.)"""
    from .model import hidden_of

    sd = model_dict["model"]
    has_ck = any(k.startswith("rnd_predictor.") for k in sd)
    if has_ck != (rnd is not None):
        raise ValueError(f"checkpoint {ck} was saved " + ("with" if has_ck else "without") + " random network distillation, the config has rnd.enabled: "
                         f"{'true' if rnd is not None else 'false'}: rnd.enabled must be as in the run that saved the checkpoint")
    if rnd is None:
        return
    entry = model_dict.get("rnd") or {}
    if entry.get("state") != rnd.state or int(sd["rnd_predictor.0.weight"].shape[1]) != rnd.width:
        raise ValueError(f"checkpoint {ck} has RND networks on rnd.state = {entry.get('state')!r} of {int(sd['rnd_predictor.0.weight'].shape[1])} columns, the "
                         f"config's rnd.state = {rnd.state!r} has {rnd.width}: rnd.state (and the env's rows) must be as in the run that saved the checkpoint")
    for key, net in (("predictor_hidden", "rnd_predictor"), ("target_hidden", "rnd_target")):
        h_ck = hidden_of(sd, net)
        if h_ck != getattr(rnd, key):
            raise ValueError(f"checkpoint {ck} has {net} hidden widths {list(h_ck)}, the config rnd.{key} = {list(getattr(rnd, key))}: set it to the "
                             "checkpoint's widths")
    if (entry.get("normalizer") is not None) != rnd.reward_normalization:
        raise ValueError(f"checkpoint {ck} was saved with rnd.reward_normalization: {'true' if entry.get('normalizer') is not None else 'false'}, the config "
                         f"has {'true' if rnd.reward_normalization else 'false'}: set rnd.reward_normalization to the checkpoint's")
