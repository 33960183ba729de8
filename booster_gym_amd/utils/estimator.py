"""The learned state estimator in front of the actor (concurrent training of a state estimator, Ji et al. 2022): the `estimator:` section of a
config and the few pure rules around it.  The deployable actor's row has no base linear velocity and no base height -- they are columns 4..7 of the
privileged observation only (reference envs/t1.py:593-602) -- so a small MLP 47 H -> hidden -> 12 regresses chosen privileged columns from the
observation history, supervised, and the actor takes [47 H observations | E estimates].

The output layer is 12 wide at any E, the width of every fused output layer of this build (bg_actor_mlp.hip's last layer, bg_distill_head): columns
[0, E) are the estimates, columns [E, 12) regress onto zero and are never read by the actor.  So the rollout's layer code and the regression head run
unchanged; the price is 12 - E output neurons that learn a constant.

Runner reads the section (utils/runner.py) and trains the network through EstimatorTrainer, utils/distill.py refuses it.  With `enabled` false or the
section absent nothing else in this file is used.
"""
import math
from typing import NamedTuple

import torch

from .. import _lib
from ..envs.t1 import MAX_ACTOR_INPUT
from .terrain import actor_heights_of
from .model import CRITIC_HIDDEN, MLPTrainer, check_hidden, hidden_of, pad_input
from .supervised import SupervisedTrainer

EST_WIDTH = _lib.NUM_DOFS  # the estimator's output layer: 12 columns, E <= 12 of them estimates
DEFAULTS = {"enabled": False, "targets": [4, 5, 6, 7], "hidden": [256, 128], "num_epochs": 2, "learning_rate": 1.0e-3, "max_grad_norm": 1.0}


class EstimatorCfg(NamedTuple):
    targets: tuple       # E indices into the privileged row
    hidden: tuple
    num_epochs: int
    learning_rate: float
    max_grad_norm: float


def estimator_enabled(cfg):
    """estimator.enabled of a config (the section or the key absent: False), or ValueError naming the key.  Pure."""
    sec = cfg.get("estimator")
    if sec is None:
        return False
    if not isinstance(sec, dict):
        raise ValueError(f"estimator must be a mapping of its keys ({', '.join(DEFAULTS)}), got {sec!r}")
    on = sec.get("enabled", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"estimator.enabled must be true or false, got {on!r}")
    return on


def estimator_cfg(cfg, world_size=1):
    """The `estimator:` section of a config as an EstimatorCfg (absent keys: DEFAULTS), None with the key off or the section absent ("off": nothing
    else of the section is read then), or ValueError naming the key.  Pure: no tensors, no device."""
    if not estimator_enabled(cfg):
        return None
    sec = cfg["estimator"]
    unknown = sorted(set(sec) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"estimator.{unknown[0]} is not a key of the section ({', '.join(DEFAULTS)})")
    v = dict(DEFAULTS, **sec)
    env, alg, terrain = cfg["env"], cfg.get("algorithm", {}) or {}, cfg.get("terrain", {}) or {}
    npv = env["num_privileged_obs"]
    t = v["targets"]
    if (not isinstance(t, (list, tuple)) or not 1 <= len(t) <= EST_WIDTH or any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < npv for i in t)
            or len(set(t)) != len(t)):
        raise ValueError(f"estimator.targets = {t!r} must be 1 to {EST_WIDTH} distinct indices into the privileged row, each from 0 to "
                         f"env.num_privileged_obs - 1 = {npv - 1}")
    try:
        hidden, _ = check_hidden(v["hidden"], CRITIC_HIDDEN)
    except ValueError as e:
        raise ValueError(str(e).replace("algorithm.actor_hidden", "estimator.hidden")) from None
    split = int((cfg.get("parallel", {}) or {}).get("gemm_split", 0) or 0)
    if split:
        try:
            check_hidden(hidden, CRITIC_HIDDEN, split)
        except ValueError as e:
            raise ValueError(str(e).replace("algorithm.actor_hidden", "estimator.hidden")) from None
    n = v["num_epochs"]
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"estimator.num_epochs must be an integer >= 1, got {n!r}")
    for key in ("learning_rate", "max_grad_norm"):
        x = v[key]
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x <= 0:
            raise ValueError(f"estimator.{key} must be a finite number > 0, got {x!r}")
    # what the key does not compose with, for now
    if alg.get("symmetry_loss", False):
        raise ValueError("estimator.enabled together with algorithm.symmetry_loss is not supported for now (the mirror map of the estimates is not "
                         "defined): set one of the two to false")
    if alg.get("empirical_normalization", False):
        raise ValueError("estimator.enabled together with algorithm.empirical_normalization is not supported for now: set one of the two to false")
    if actor_heights_of(terrain):
        raise ValueError("estimator.enabled together with terrain.actor_heights is not supported for now (the perceptive actor's row ends with the "
                         "height scan): set one of the two to false")
    K = (cfg.get("runner", {}) or {}).get("num_mini_batches", 1)
    if K is not None and K != 1:
        raise ValueError(f"estimator.enabled together with runner.num_mini_batches = {K!r} is not supported for now: set runner.num_mini_batches to 1")
    if int(world_size) != 1:
        raise ValueError(f"estimator.enabled runs on one rank (WORLD_SIZE = {world_size}): data parallelism is out of scope for now")
    no = env["num_observations"]
    if no + len(t) > MAX_ACTOR_INPUT:
        raise ValueError(f"estimator.targets: the actor's input env.num_observations + {len(t)} estimates = {no + len(t)} exceeds {MAX_ACTOR_INPUT} "
                         "(BG_ACTOR_MAX_INPUT, the widest first layer of the rollout's sampling kernel): a smaller env.frame_stack or fewer targets")
    return EstimatorCfg(tuple(int(i) for i in t), hidden, n, float(v["learning_rate"]), float(v["max_grad_norm"]))


def estimator_targets(privileged, targets, out=None):
    """The regression target [..., 12] of privileged rows [..., num_privileged_obs]: the chosen columns in the order of `targets`, then zeros."""
    if out is None:
        out = torch.zeros(tuple(privileged.shape[:-1]) + (EST_WIDTH,), dtype=privileged.dtype, device=privileged.device)
    idx = torch.as_tensor(list(targets), dtype=torch.long, device=privileged.device)
    out[..., : len(targets)].copy_(privileged.index_select(-1, idx))
    out[..., len(targets):].zero_()
    return out


class EstimatorTrainer:
    """The estimator's supervised update, what estimator.enabled adds to a Runner behind the model, the second FlatAdam (`optimizer`, over the
    estimator's parameters under `clock`) and the `estimates` buffer: the zero-padded input, the regression target [B][12] of B = T x N rows, the
    target columns' index and gather buffer, the last epoch's loss and the SupervisedTrainer that takes the steps."""

    def __init__(self, est, net, optimizer, clock, T, N, num_obs, device):
        B = int(T) * int(N)
        self.est, self.num_obs = est, int(num_obs)
        self.x = torch.zeros(B, pad_input(num_obs), device=device)  # (the padded columns stay zero)
        self.target = torch.zeros(B, EST_WIDTH, device=device)  # columns [E, 12) stay zero: what the unread outputs regress onto
        self.idx = torch.tensor(est.targets, dtype=torch.long, device=device)
        self.sel = torch.zeros(B, len(est.targets), device=device)
        self.loss = torch.zeros(1, dtype=torch.float64, device=device)  # the last epoch's loss, SSE / (12 B): estimator/loss of the log
        self.sup = SupervisedTrainer("estimator.enabled", net, optimizer, clock, B, self.x.shape[1])
        self.resolve_plan()  # (a batch outside the layer kernels' range is a ValueError here, not at the first update)

    def resolve_plan(self):
        """The plan of MLPTrainer's switches as they are now (SupervisedTrainer.resolve_plan), behind the width check of the split-bf16 layer kernels."""
        kin, hidden = self.x.shape[1], [l.out_features for l in self.sup.mlp.layers[:-1]]
        if MLPTrainer.SPLIT and (kin > 256 or any(w > 256 for w in hidden[:-1])):
            raise ValueError(f"parallel.gemm_split / BG_GEMM_SPLIT runs split-bf16 layer kernels that take layer inputs of 64, 128 or 256 columns only; the "
                             f"estimator's input pads to {kin} and estimator.hidden = {hidden} (use gemm_split 0)")
        return self.sup.resolve_plan()

    def update(self, obses, privileged):
        """estimator.num_epochs full-batch Adam steps of L = 1 / (12 B) sum |estimator(obses) - target|^2 on the iteration's rows obses [T][N][num_obs]
        and privileged [T][N][num_privileged_obs], target = the chosen privileged columns, then zeros, on the current stream; no library GEMM.  The
        plan is resolved anew (MLPTrainer's switches are process-wide).  Leaves the last epoch's loss in `loss` (device)."""
        B = self.target.shape[0]
        self.resolve_plan()
        self.x[:, : self.num_obs].copy_(obses.reshape(B, -1))
        torch.index_select(privileged.reshape(B, -1), 1, self.idx, out=self.sel)
        self.target[:, : len(self.est.targets)].copy_(self.sel)
        for _ in range(self.est.num_epochs):
            self.sup.step(self.x, self.target)
        torch.mul(self.sup.stats, 1.0 / (EST_WIDTH * B), out=self.loss)


def check_estimator_checkpoint(ck, model_dict, est, ck_ain, a_in):
    """Runner._load's check of checkpoint `ck` (loaded: model_dict) against the config's EstimatorCfg `est` (None: off); ck_ain / a_in: the inputs of
    the checkpoint's and of the config's actor.  ValueError naming estimator.enabled / estimator.targets / estimator.hidden unless the checkpoint's
    estimator is the config's: both without one, or both with the same targets and widths."""
    has_ck = any(k.startswith("estimator.") for k in model_dict["model"])
    entry = model_dict.get("estimator") if has_ck else None
    t_ck = [int(i) for i in entry["targets"]] if isinstance(entry, dict) and "targets" in entry else None
    if has_ck != (est is not None):
        raise ValueError(f"checkpoint {ck} was saved " + (f"with a state estimator (estimator.enabled: true, estimator.targets: {t_ck}; its actor takes "
                                                          f"{ck_ain} inputs)" if has_ck else f"without a state estimator (its actor takes {ck_ain} inputs)")
                         + f", the config has estimator.enabled: {'true' if est is not None else 'false'} (its actor takes {a_in}): estimator.enabled "
                         "and estimator.targets must be as in the run that saved the checkpoint")
    if est is None:
        return
    if t_ck != list(est.targets):
        raise ValueError(f"checkpoint {ck} has an estimator of estimator.targets = {t_ck}, the config's estimator.targets = {list(est.targets)}: "
                         "estimator.targets must be as in the run that saved the checkpoint")
    h_ck = hidden_of(model_dict["model"], "estimator")
    if h_ck != est.hidden:
        raise ValueError(f"checkpoint {ck} has estimator hidden widths {list(h_ck)}, the config estimator.hidden = {list(est.hidden)}: set it to "
                         "the checkpoint's widths")
