"""Empirical observation normalisation (algorithm.empirical_normalization; rsl_rl's `EmpiricalNormalization` with until=None, restated).

One set of statistics over the critic's real input columns, C = num_obs + num_privileged_obs: mean[C], var[C] (population variance), count; the
actor uses columns [0, num_obs) of the same vectors.  Initial state: mean 0, var 1, count 0.  A value enters a network as

    y = (x - mean) / (sqrt(var) + eps)                     (eps = algorithm.normalization_eps, 1e-2; no clipping)

The statistics change ONCE per PPO iteration, after the last optimiser step of Runner.update(), from the T x N rows [0, T) of that iteration's
observation buffers (rsl_rl updates at every `act`): the rollout and all mini-epochs of an iteration see the same statistics, and the first
importance ratio of an update stays exactly 1.  Batches are merged with Chan et al.'s rule (`merge_moments`), kept in float64 on the host; the
device holds fp32 copies of mean and 1 / (sqrt(var) + eps) for the two kernels of csrc/bg_obs_norm.hip.  The experience buffer keeps raw
observations.

The merge rule, the fold into a first Linear layer and the state are plain numpy / torch-CPU code: the CPU tests, export_model.py and
tools/play_oracle.py use them without a device.
"""
import numpy as np
import torch

from .. import _lib

KEY = "algorithm.empirical_normalization"


def normalization_cfg(cfg):
    """(on, eps) of a config: algorithm.empirical_normalization (absent = false) and algorithm.normalization_eps (default 1e-2; <= 0: ValueError)."""
    alg = cfg.get("algorithm", {}) or {}
    on = alg.get("empirical_normalization", False)
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


def merge_moments(mean, var, count, m_b, v_b, n):
    """Chan et al.'s merge of (mean, population variance, count) with a batch of n rows of mean m_b and biased variance v_b, float64:
        count' = count + n; r = n / count'; d = m_b - mean; mean' = mean + r d; var' = var + r (v_b - var + d (m_b - mean')).
    Returns (mean', var', count').  n = 0 changes nothing."""
    mean, var, m_b, v_b = (np.asarray(a, dtype=np.float64) for a in (mean, var, m_b, v_b))
    n = float(n)
    if n <= 0:
        return mean.copy(), var.copy(), float(count)
    total = float(count) + n
    r = n / total
    d = m_b - mean
    new_mean = mean + r * d
    new_var = var + r * (v_b - var + d * (m_b - new_mean))
    return new_mean, np.maximum(new_var, 0.0), total


def moments_from_sums(s, ss, n):
    """(mean, biased variance) of n rows from their float64 column sums and sums of squares (what bg_obs_moments writes and the ranks exchange)."""
    s, ss = np.asarray(s, dtype=np.float64), np.asarray(ss, dtype=np.float64)
    m = s / float(n)
    return m, np.maximum(ss / float(n) - m * m, 0.0)


class ObsNormalizer:
    """The float64 state, its fp32 device copies and the two launches.  device=None: host only (no library call is made)."""

    def __init__(self, cols, eps=1.0e-2, device=None):
        if eps <= 0:
            raise ValueError(f"algorithm.normalization_eps must be > 0, got {eps!r}")
        self.cols, self.eps, self.device = int(cols), float(eps), device
        self.mean, self.var, self.count = np.zeros(self.cols), np.ones(self.cols), 0.0
        if device is not None:
            self.mean_dev = torch.zeros(self.cols, dtype=torch.float32, device=device)
            self.inv_std_dev = torch.zeros(self.cols, dtype=torch.float32, device=device)
            # one float64 vector [sum (C), sumsq (C), rows (1)]: written by bg_obs_moments, exchanged by the ranks as it is
            self._sums = torch.zeros(2 * self.cols + 1, dtype=torch.float64, device=device)
            self._scratch = torch.zeros(_lib.OBS_MOMENTS_MAX_GROUPS * 2 * self.cols, dtype=torch.float64, device=device)
        self.refresh()

    # ---- state
    def inv_std(self):
        """1 / (sqrt(var) + eps), float64."""
        return 1.0 / (np.sqrt(self.var) + self.eps)

    def refresh(self):
        """The device's fp32 copies from the float64 state (after every change of it)."""
        self.mean32 = self.mean.astype(np.float32)
        self.inv_std32 = self.inv_std().astype(np.float32)
        if self.device is not None:
            self.mean_dev.copy_(torch.from_numpy(self.mean32))
            self.inv_std_dev.copy_(torch.from_numpy(self.inv_std32))

    def merge(self, m_b, v_b, n):
        self.mean, self.var, self.count = merge_moments(self.mean, self.var, self.count, m_b, v_b, n)
        self.refresh()

    def merge_sums(self, sums):
        """sums: [sum (C), sumsq (C), rows] float64, of all ranks' rows together."""
        sums = np.asarray(sums, dtype=np.float64)
        C, n = self.cols, float(sums[-1])
        self.merge(*moments_from_sums(sums[:C], sums[C : 2 * C], n), n)

    def state_dict(self):
        return {"mean": torch.from_numpy(self.mean.copy()), "var": torch.from_numpy(self.var.copy()), "count": float(self.count), "eps": float(self.eps)}

    def load_state_dict(self, sd):
        mean, var = (np.asarray(torch.as_tensor(sd[k]).detach().cpu().double().numpy(), dtype=np.float64).reshape(-1) for k in ("mean", "var"))
        if mean.shape != (self.cols,) or var.shape != (self.cols,):
            raise ValueError(f"{KEY}: the checkpoint's normaliser has {mean.shape[0]} columns, the config's networks read {self.cols} "
                             "(env.num_observations + env.num_privileged_obs)")
        if float(sd["eps"]) != self.eps:  # (a policy trained with one eps and fed through another sees other inputs; not replaced silently)
            raise ValueError(f"{KEY}: the checkpoint's normaliser was trained with algorithm.normalization_eps = {float(sd['eps'])!r}, the config has "
                             f"{self.eps!r}: set algorithm.normalization_eps to the checkpoint's value")
        self.mean, self.var, self.count = mean.copy(), var.copy(), float(sd["count"])
        self.refresh()

    def scalars(self):
        """The three log scalars: obs_norm/count, obs_norm/max_abs_mean, obs_norm/min_std."""
        return {"obs_norm/count": float(self.count), "obs_norm/max_abs_mean": float(np.abs(self.mean).max()), "obs_norm/min_std": float(np.sqrt(self.var).min())}

    # ---- host arithmetic
    def normalize_host(self, x, col0=0):
        """What bg_obs_normalize computes, on the host in the dtype of x (float64 in, float64 out), from the fp32 copies the device holds."""
        x = np.asarray(x)
        c = x.shape[-1]
        return (x - self.mean32[col0 : col0 + c].astype(x.dtype)) * self.inv_std32[col0 : col0 + c].astype(x.dtype)

    def fold_into_first_layer(self, weight, bias, col0=0, dtype=torch.float32):
        """A first Linear layer that takes raw rows: W' = W diag(inv_std), b' = b - W' mean, computed in float64 and returned as fp32 tensors (or as
        `dtype`), so that W' x + b' = W ((x - mean) inv_std) + b.  From the fp32 copies the kernels use: the folded layer reproduces the trained
        policy's inputs."""
        w = torch.as_tensor(weight).detach().cpu().double().numpy()
        b = torch.as_tensor(bias).detach().cpu().double().numpy()
        k = w.shape[1]
        w2 = w * self.inv_std32[col0 : col0 + k].astype(np.float64)[None, :]
        b2 = b - w2 @ self.mean32[col0 : col0 + k].astype(np.float64)
        return torch.from_numpy(w2).to(dtype), torch.from_numpy(b2).to(dtype)

    # ---- device launches
    def moments_into(self, obs, priv):
        """bg_obs_moments on the rows of obs [..., no] and priv [..., npv] (views of whole leading rows of the buffers): leaves
        [sum, sumsq, rows] in self._sums on the current stream and returns it."""
        no, npv = obs.shape[-1], priv.shape[-1]
        rows = obs.numel() // no
        if no + npv != self.cols or priv.numel() // max(npv, 1) != rows or not (obs.is_contiguous() and priv.is_contiguous()):
            raise ValueError("ObsNormalizer.moments_into: contiguous row blocks of num_obs and num_privileged_obs columns and equal rows")
        C = self.cols
        _lib.check(_lib.load().bg_obs_moments(rows, _lib.ptr(obs), no, no, _lib.ptr(priv), npv, npv, _lib.ptr(self._sums), _lib.ptr(self._sums[C:]),
                                              _lib.ptr(self._scratch), _lib.current_stream_ptr()), "bg_obs_moments")
        self._sums[2 * C :].fill_(float(rows))
        return self._sums

    def update_from(self, obs, priv, dp=None):
        """Once per iteration: moments of this rank's rows (one launch pair), ONE float64 exchange over the ranks (dp.sum_), the merge on the host and
        the refresh of the device copies.  Reads the sums back: the one host synchronisation the feature adds per iteration."""
        self.merge_exchanged(self.moments_into(obs, priv), dp)

    def merge_exchanged(self, sums, dp=None):
        """sums: this rank's [sum (C), sumsq (C), rows] as ONE float64 tensor (device or host); summed over the ranks in place, then merged: every rank
        ends with the statistics of all ranks' rows."""
        if dp is not None:
            dp.sum_(sums, tag="obs_norm")
        self.merge_sums(sums.cpu().numpy())

    def normalize_into(self, src, dst, col0=0, dst_cols=None):
        """bg_obs_normalize: dst[..., c] = (src[..., c] - mean[col0 + c]) * inv_std[col0 + c] for the columns of src, zeros in dst's columns up to
        dst_cols (default: the columns of src).  src / dst: equal leading shapes, unit stride in the last dimension, one common stride between
        consecutive rows (views of padded network inputs: dst's row stride may exceed dst_cols)."""
        cols = src.shape[-1]
        rows = src.numel() // cols
        dst_cols = cols if dst_cols is None else int(dst_cols)
        if tuple(dst.shape[:-1]) != tuple(src.shape[:-1]) or dst.shape[-1] < dst_cols:
            raise ValueError(f"normalize_into: src {tuple(src.shape)} and dst {tuple(dst.shape)} must have equal leading shapes and dst at least "
                             f"dst_cols = {dst_cols} columns")
        _lib.check(_lib.load().bg_obs_normalize(rows, cols, _lib.ptr(src), _row_stride(src), _lib.ptr(dst), dst_cols, _row_stride(dst), _lib.ptr(self.mean_dev),
                                                _lib.ptr(self.inv_std_dev), int(col0), _lib.current_stream_ptr()), "bg_obs_normalize")
        return dst


def _row_stride(t):
    """Floats between consecutive rows of t seen as [rows][cols]: every leading dimension must continue the one behind it."""
    if t.stride(-1) != 1:
        raise ValueError("normalize_into: unit stride in the last dimension")
    if t.dim() == 1:
        return t.shape[0]
    rs = t.stride(-2)
    for d in range(t.dim() - 2, 0, -1):
        if t.shape[d - 1] != 1 and t.stride(d - 1) != t.stride(d) * t.shape[d]:
            raise ValueError("normalize_into: rows must lie at one common stride")
    return rs


def check_checkpoint(ck, entry, norm):
    """Runner._load: `entry` = the checkpoint's "obs_normalizer" (or None), `norm` = the runner's ObsNormalizer (or None).  A policy fed inputs it was
    not trained on must not load silently: key and entry must agree, and so must the column count (ValueError naming the key); loads the state."""
    if entry is None and norm is not None:
        raise ValueError(f"checkpoint {ck} has no observation normaliser but the config sets {KEY}: true; its policy was trained on raw observations: "
                         f"set {KEY}: false")
    if entry is not None and norm is None:
        raise ValueError(f"checkpoint {ck} carries an observation normaliser but the config has {KEY}: false (or no such key); its policy was trained on "
                         f"normalised observations: set {KEY}: true")
    if norm is not None:
        norm.load_state_dict(entry)
