"""Value normalisation (algorithm.normalize_value; rl_games' `normalize_value`, restated): the critic regresses onto standardised returns.

State: a running mean m, population variance s2 and count n of the returns, float64 ON THE DEVICE; initial state 0, 1, 0.  With
sigma = sqrt(s2) + eps (eps = algorithm.normalization_eps, the key observation normalisation reads; 1e-2) the critic's output u on a row stands for
the value

    v = fmaf(sigma, u, m)                                  (one rounding)

and the buffer `returns` of a mini-epoch receives Rn = (R - m) * (1 / sigma), R = v + advantage, so that the value loss mean((u - Rn)^2) is
mean(((v - R) / sigma)^2): the loss heads run unchanged on u and Rn.  Everything else of the whole-batch pass -- the time-out bootstrap, GAE, the
advantages and their moments -- runs on v.  All of that is inside ONE launch, bg_critic_values_gae_norm (csrc/bg_head.hip), which reads the fp32
triple (m, sigma, 1 / sigma) from the device and leaves (sum R, sum R^2, count) of the rank's un-normalised returns in float64.

The statistics change ONCE per PPO iteration, behind the last optimiser step of Runner.update(): the last mini-epoch's sums, added over the ranks in
one float64 exchange (tag "value_norm"), are merged by Chan et al.'s rule in one small launch (bg_value_norm_update: utils/obs_norm.py's
moments_from_sums / merge_moments on the device), which also rewrites the fp32 triple.  No host read: all mini-epochs of an iteration and the next
iteration's forward-ahead (which writes raw u) see one set of statistics.  Because sigma starts at 1 + eps, the first iteration runs on v = 1.01 u.

Output-preserving rescaling of the critic's last layer when the statistics move (PopArt) is not done: the critic's next targets simply move.
"""
import math

import numpy as np

KEY = "algorithm.normalize_value"


def normalize_value_of(cfg):
    """(on, eps) of a config: algorithm.normalize_value (absent, null or false = off; anything but a bool: ValueError naming the key) and
    algorithm.normalization_eps (default 1e-2; not a finite number > 0: ValueError naming that key), read whether or not
    algorithm.empirical_normalization is set."""
    alg = cfg.get("algorithm", {}) or {}
    on = alg.get("normalize_value", False)
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"{KEY} must be true or false, got {on!r}")
    eps = alg.get("normalization_eps", 1.0e-2)
    if eps is None:
        eps = 1.0e-2
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not np.isfinite(eps) or eps <= 0:
        raise ValueError(f"algorithm.normalization_eps must be a finite number > 0, got {eps!r}")
    return on, float(eps)


def triple_of(mean, var, eps):
    """The fp32 triple (m, sigma, 1 / sigma) of a float64 state, as bg_value_norm_update rounds it."""
    sigma = math.sqrt(float(var)) + float(eps)
    return np.array([mean, sigma, 1.0 / sigma], dtype=np.float64).astype(np.float32)


class ValueNormalizer:
    """The float64 device state [mean, var, count], the fp32 device triple the kernels read, and the float64 [6] vector that
    bg_critic_values_gae_norm writes: [0:3] the advantage moments (Runner._adv_sums is this view), [3:6] (sum R, sum R^2, count)."""

    def __init__(self, eps=1.0e-2, device=None):
        import torch

        if not eps > 0:
            raise ValueError(f"algorithm.normalization_eps must be > 0, got {eps!r}")
        self.eps, self.device = float(eps), device
        self.state = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=device)
        self.stats = torch.from_numpy(triple_of(0.0, 1.0, self.eps)).to(device)
        self.sums = torch.zeros(6, dtype=torch.float64, device=device)

    def update_from(self, sums=None, dp=None):
        """Once per iteration, on the current stream: sums[3:6] = this rank's (sum R, sum R^2, count), added over the ranks in ONE float64 exchange
        (dp.sum_, tag "value_norm"), then the merge and the new fp32 triple in one launch.  No host read."""
        from .utils import value_norm_update

        sums = self.sums if sums is None else sums
        if dp is not None:
            dp.sum_(sums[3:6], tag="value_norm")
        value_norm_update(sums, self.state, self.stats, self.eps)

    def denormalize(self, u):
        """v = fmaf(sigma, u, m) of a critic output (ActorCritic.est_value under the key) as a new fp32 tensor (bg_value_denormalize)."""
        from .utils import value_denormalize

        return value_denormalize(u.detach().float().contiguous().clone(), self.stats)

    @staticmethod
    def scalars_from(state):
        """The three log scalars from (mean, var, count) on the host."""
        mean, var, count = (float(x) for x in state)
        return {"value_norm/mean": mean, "value_norm/std": math.sqrt(max(var, 0.0)), "value_norm/count": count}

    def scalars(self):
        """value_norm/mean, value_norm/std, value_norm/count (reads the device: the training loop carries the state in its own host read instead)."""
        return self.scalars_from(self.state.cpu().tolist())

    def state_dict(self):
        mean, var, count = self.state.cpu().tolist()
        return {"mean": mean, "var": var, "count": count, "eps": self.eps}

    def load_state_dict(self, sd):
        import torch

        check_entry(sd, True, self.eps)
        mean, var, count = (float(sd[k]) for k in ("mean", "var", "count"))  # (Python floats: float64, as saved)
        self.state.copy_(torch.tensor([mean, var, count], dtype=torch.float64))
        self.stats.copy_(torch.from_numpy(triple_of(mean, var, self.eps)))


def check_entry(entry, on, eps, ck="the checkpoint"):
    """The rules of check_checkpoint on plain values: `entry` = the checkpoint's "value_normalizer" dict or None, on / eps = the config's."""
    if entry is None and on:
        raise ValueError(f"checkpoint {ck} has no value normaliser but the config sets {KEY}: true; its critic was trained on returns in reward units: "
                         f"set {KEY}: false")
    if entry is not None and not on:
        raise ValueError(f"checkpoint {ck} carries a value normaliser but the config has {KEY}: false (or no such key); its critic was trained on "
                         f"standardised returns: set {KEY}: true")
    if entry is not None and float(entry["eps"]) != float(eps):
        raise ValueError(f"{KEY}: checkpoint {ck} was trained with algorithm.normalization_eps = {float(entry['eps'])!r}, the config has {float(eps)!r}: set "
                         "algorithm.normalization_eps to the checkpoint's value")


def check_checkpoint(ck, entry, norm):
    """A training Runner's _load: `entry` = the checkpoint's "value_normalizer" (or None), `norm` = the runner's ValueNormalizer (or None).  A critic
    whose outputs mean something else than the config says must not load silently: key and entry must agree, and so must eps (ValueError naming the
    key); loads the state.  (Runner(test=True), play, evaluation and export never evaluate the critic and do not call this.)"""
    check_entry(entry, norm is not None, norm.eps if norm is not None else 0.0, ck)
    if norm is not None:
        norm.load_state_dict(entry)
