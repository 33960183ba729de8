"""Host-side mirrors of reference `utils/utils.py` on top of the HIP kernels.

  apply_randomization   reference utils/utils.py:5-30   (set-up time randomisation; same arguments,
                        same ValueError behaviour; per-step noise is drawn inside the HIP env kernel)
  discount_values       reference utils/utils.py:33-44  -> bg_gae (one backward scan, HBM-bound)
  ppo_loss_fused        reference utils/runner.py:144-174 + utils/utils.py:47-52 -> bg_ppo_loss
There is no torch/CPU fallback: CUDA tensors are required and the native library must load.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib


def apply_randomization(tensor, params, return_noise=False):
    if params is None:
        return tensor
    dist, op = params["distribution"], params["operation"]
    if dist == "gaussian":
        mu, std = params["range"]  # (mean, std): SURVEY Q8
        noise = torch.randn_like(tensor) if isinstance(tensor, torch.Tensor) else np.random.randn()
        value = mu + std * noise
    elif dist == "uniform":
        lo, hi = params["range"]
        noise = torch.rand_like(tensor) if isinstance(tensor, torch.Tensor) else np.random.rand()
        value = lo + (hi - lo) * noise
    else:
        raise ValueError(f"Invalid randomization distribution: {dist}")
    if op == "additive":
        out = tensor + value
    elif op == "scaling":
        out = tensor * value
    else:
        raise ValueError(f"Invalid randomization operation: {op}")
    return (out, noise) if return_noise else out


def rand_spec(params):
    """yaml randomisation entry -> (mode, a, b) of `bg_rand` (include/booster_gym_amd.h)."""
    if params is None:
        return (0, 0.0, 0.0)
    dist, op = params["distribution"], params["operation"]
    if dist not in ("gaussian", "uniform"):
        raise ValueError(f"Invalid randomization distribution: {dist}")
    if op not in ("additive", "scaling"):
        raise ValueError(f"Invalid randomization operation: {op}")
    mode = (1 if dist == "gaussian" else 3) + (0 if op == "additive" else 1)
    return (mode, float(params["range"][0]), float(params["range"][1]))


def _need_cuda(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("booster_gym_amd kernels need CUDA (ROCm) tensors; there is no CPU path")
        if not t.is_contiguous():
            raise RuntimeError("booster_gym_amd kernels need contiguous tensors")


def gae(rewards, dones, time_outs, values, last_values, gamma, lam, advantages=None, returns=None, sums=None):
    """Fused timeout-overwrite + GAE + returns + moments.  rewards is modified in place (runner.py:135).

    Returns (advantages [T,N], returns [T,N], sums float64[3] = (sum, sum of squares, count))."""
    T, N = rewards.shape
    advantages = torch.empty_like(values) if advantages is None else advantages
    returns = torch.empty_like(values) if returns is None else returns
    if sums is None:
        sums = torch.zeros(3, dtype=torch.float64, device=rewards.device)
    else:
        sums.zero_()
    d8 = dones.view(torch.uint8) if dones.dtype == torch.bool else dones
    t8 = time_outs.view(torch.uint8) if time_outs.dtype == torch.bool else time_outs
    _need_cuda(rewards, d8, t8, values, last_values, advantages, returns, sums)
    lib = _lib.load()
    _lib.check(lib.bg_gae(T, N, _lib.ptr(rewards), _lib.ptr(d8), _lib.ptr(t8), _lib.ptr(values), _lib.ptr(last_values), gamma, lam,
                          _lib.ptr(advantages), _lib.ptr(returns), _lib.ptr(sums), _lib.current_stream_ptr()), "bg_gae")
    return advantages, returns, sums


def critic_values_gae(h, w, b, rewards, dones, time_outs, gamma, lam, values_all, advantages, returns, sums, scratch):
    """Output layer of the critic on all (T + 1) N rows of h, then `gae` on the result, in one launch (bg_critic_values_gae); h = None: values_all is
    given (the chained forward kernel's value head wrote it) and only the GAE half runs.  rewards [T, N] is
    modified in place as in `gae`; values_all [(T + 1) N], advantages / returns [T, N] and sums float64[3] are written; scratch: float64
    [3 * ceil(N / 16) + 1] whose last element the caller zeroed once."""
    T, N = rewards.shape
    d8 = dones.view(torch.uint8) if dones.dtype == torch.bool else dones
    t8 = time_outs.view(torch.uint8) if time_outs.dtype == torch.bool else time_outs
    _need_cuda(rewards, d8, t8, values_all, advantages, returns, sums, scratch, *([] if h is None else [h, w, b]))
    if (h is not None and h.shape[0] != (T + 1) * N) or values_all.numel() != (T + 1) * N or scratch.numel() < 3 * ((N + 15) // 16) + 1:
        raise ValueError("critic_values_gae: h / values_all must have (T + 1) N rows, scratch 3 ceil(N / 16) + 1 float64")
    _lib.check(_lib.load().bg_critic_values_gae(T, N, _lib.ptr(h), _lib.ptr(w), _lib.ptr(b), _lib.ptr(rewards), _lib.ptr(d8), _lib.ptr(t8), gamma, lam,
                                                _lib.ptr(values_all), _lib.ptr(advantages), _lib.ptr(returns), _lib.ptr(sums), _lib.ptr(scratch),
                                                _lib.current_stream_ptr()), "bg_critic_values_gae")
    return values_all


def critic_values_gae_norm(h, w, b, rewards, dones, time_outs, gamma, lam, values_all, advantages, returns, value_stats, sums, scratch):
    """critic_values_gae under algorithm.normalize_value (bg_critic_values_gae_norm): values_all holds the critic's standardised output u (h = None:
    given; else written), the scan runs on v = fmaf(sigma, u, m) with value_stats = fp32 [3] (m, sigma, 1 / sigma), returns receives
    (R - m) * (1 / sigma); sums float64[6]: the advantage moments, then (sum R, sum R^2, count) of the un-normalised returns; scratch: float64
    [6 * ceil(N / 16) + 1] whose last element the caller zeroed once."""
    T, N = rewards.shape
    d8 = dones.view(torch.uint8) if dones.dtype == torch.bool else dones
    t8 = time_outs.view(torch.uint8) if time_outs.dtype == torch.bool else time_outs
    _need_cuda(rewards, d8, t8, values_all, advantages, returns, value_stats, sums, scratch, *([] if h is None else [h, w, b]))
    if (h is not None and h.shape[0] != (T + 1) * N) or values_all.numel() != (T + 1) * N or scratch.numel() < 6 * ((N + 15) // 16) + 1 or sums.numel() < 6:
        raise ValueError("critic_values_gae_norm: h / values_all must have (T + 1) N rows, sums 6 and scratch 6 ceil(N / 16) + 1 float64")
    if value_stats.dtype != torch.float32 or value_stats.numel() != 3 or sums.dtype != torch.float64 or scratch.dtype != torch.float64:
        raise ValueError("critic_values_gae_norm: value_stats is fp32 [3], sums and scratch are float64")
    _lib.check(_lib.load().bg_critic_values_gae_norm(T, N, _lib.ptr(h), _lib.ptr(w), _lib.ptr(b), _lib.ptr(rewards), _lib.ptr(d8), _lib.ptr(t8), gamma, lam,
                                                     _lib.ptr(values_all), _lib.ptr(advantages), _lib.ptr(returns), _lib.ptr(value_stats), _lib.ptr(sums),
                                                     _lib.ptr(scratch), _lib.current_stream_ptr()), "bg_critic_values_gae_norm")
    return values_all


def value_denormalize(values, value_stats):
    """values = fmaf(sigma, values, m) in place (bg_value_denormalize): fp32, contiguous; value_stats fp32 [3] = (m, sigma, 1 / sigma)."""
    _need_cuda(values, value_stats)
    if values.dtype != torch.float32 or value_stats.dtype != torch.float32 or value_stats.numel() != 3:
        raise ValueError("value_denormalize: fp32 values and value_stats fp32 [3]")
    if values.numel():
        _lib.check(_lib.load().bg_value_denormalize(values.numel(), _lib.ptr(values), _lib.ptr(value_stats), _lib.current_stream_ptr()), "bg_value_denormalize")
    return values


def value_norm_update(sums, state, value_stats, eps):
    """Chan's merge of state float64 [3] (mean, variance, count) with sums[3:6] = (sum, sum of squares, count) on the device, then the fp32 triple
    (bg_value_norm_update)."""
    _need_cuda(sums, state, value_stats)
    if sums.dtype != torch.float64 or sums.numel() < 6 or state.dtype != torch.float64 or state.numel() != 3 or value_stats.dtype != torch.float32 or value_stats.numel() != 3:
        raise ValueError("value_norm_update: sums float64 [6], state float64 [3], value_stats fp32 [3]")
    _lib.check(_lib.load().bg_value_norm_update(_lib.ptr(sums), _lib.ptr(state), _lib.ptr(value_stats), float(eps), _lib.current_stream_ptr()), "bg_value_norm_update")


def discount_values(rewards, dones, values, last_values, gamma, lam):
    """Reference signature (utils/utils.py:33): `dones` already includes the time-outs; rewards are not touched."""
    zeros = torch.zeros_like(dones, dtype=torch.uint8)
    adv, _, _ = gae(rewards.clone(), dones.contiguous(), zeros, values.contiguous(), last_values.contiguous(), gamma, lam)
    return adv


def gaussian_logp(mu, logstd, actions, out=None):
    B, A = mu.shape
    out = torch.empty(B, dtype=torch.float32, device=mu.device) if out is None else out
    _need_cuda(mu, logstd, actions, out)
    _lib.check(_lib.load().bg_gaussian_logp(B, A, _lib.ptr(mu), _lib.ptr(logstd), _lib.ptr(actions), _lib.ptr(out), _lib.current_stream_ptr()),
               "bg_gaussian_logp")
    return out


def ppo_loss_fused(mu, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, values, returns, e_clip, bound_coef, entropy_coef,
                   grad_mu, grad_values, grad_logstd, stats):
    """One pass over B samples: loss statistics and d(loss)/d(mu, values, logstd).  Outputs are caller-owned:
    grad_logstd float64[A] and stats float64[5] are zeroed here and accumulated with atomics."""
    B, A = mu.shape
    _need_cuda(mu, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, values, returns, grad_mu, grad_values, grad_logstd, stats)
    grad_logstd.zero_()
    stats.zero_()
    _lib.check(_lib.load().bg_ppo_loss(B, A, _lib.ptr(mu), _lib.ptr(logstd), _lib.ptr(actions), _lib.ptr(old_mu), _lib.ptr(old_logstd),
                                       _lib.ptr(old_logp), _lib.ptr(adv), _lib.ptr(adv_stats), _lib.ptr(values), _lib.ptr(returns), e_clip,
                                       bound_coef, entropy_coef, _lib.ptr(grad_mu), _lib.ptr(grad_values), _lib.ptr(grad_logstd), _lib.ptr(stats),
                                       _lib.current_stream_ptr()), "bg_ppo_loss")


def head_scratch(device):
    """Workspace of one fused head call (per-workgroup partial sums); calls that may run concurrently need their own."""
    return torch.empty(_lib.HEAD_SCRATCH_FLOATS, dtype=torch.float32, device=device)


def critic_head_forward(h, weight, bias, values_out):
    """values = h @ weight.T + bias for the 128 -> 1 output layer (model.py:21), one pass over h [rows, 128]."""
    _need_cuda(h, weight, bias, values_out)
    _lib.check(_lib.load().bg_critic_head_forward(h.shape[0], _lib.ptr(h), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(values_out),
                                                  _lib.current_stream_ptr()), "bg_critic_head_forward")
    return values_out


def actor_head_forward(h, weight, bias, mu_out):
    """mu = h @ weight.T + bias for the 128 -> 12 output layer (model.py:13) with the arithmetic of the fused loss kernel."""
    _need_cuda(h, weight, bias, mu_out)
    z = None
    _lib.check(_lib.load().bg_actor_head(h.shape[0], 0, _lib.ptr(h), _lib.ptr(weight), _lib.ptr(bias), z, z, z, z, z, z, z, 0.0, 0.0, 0.0,
                                         _lib.ptr(mu_out), z, z, z, z, z, z, z, _lib.current_stream_ptr()), "bg_actor_head")
    return mu_out


def actor_head_loss_backward(h, weight, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, e_clip, bound_coef, entropy_coef,
                             g_hidden, grad_weight, grad_bias, grad_bias_hidden, grad_logstd, stats, scratch, mu_out=None, finish=None):
    """Output layer + PPO actor loss (runner.py:145-174) + output-layer backward in one pass over h [B, 128].  grad_logstd float64[12] and
    stats float64[5] (entries 1..4) are ACCUMULATED with atomics: the caller zeroes them (the critic head adds entry 0 concurrently).
    finish (a _lib.ReduceProblem): only the main kernel runs; the sums over its workgroups (grad_weight, grad_bias, grad_bias_hidden, grad_logstd,
    stats) are left to a later bg_reduce_group call on the descriptor written into `finish`; g_hidden is complete either way."""
    _need_cuda(h, weight, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, g_hidden, grad_weight, grad_bias, grad_bias_hidden,
               grad_logstd, stats, scratch)
    args = [_lib.ptr(t) for t in (h, weight, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats)] + [e_clip, bound_coef, entropy_coef]
    args += [_lib.ptr(t) for t in (mu_out, g_hidden, grad_weight, grad_bias, grad_bias_hidden, grad_logstd, stats, scratch)]
    if finish is not None:
        _lib.check(_lib.load().bg_actor_head_partial(h.shape[0], *args, finish, _lib.current_stream_ptr()), "bg_actor_head_partial")
    else:
        _lib.check(_lib.load().bg_actor_head(h.shape[0], 1, *args, _lib.current_stream_ptr()), "bg_actor_head")


def actor_head_sym_loss_backward(h, weight, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, e_clip, bound_coef, entropy_coef,
                                 sym_coef, act_mirror, g_hidden, grad_weight, grad_bias, grad_bias_hidden, grad_logstd, stats, scratch, mu_out=None,
                                 finish=None):
    """actor_head_loss_backward plus the mirror-symmetry loss (bg_actor_head_sym): h [2B, 128] holds the batch's rows and then their mirror images,
    g_hidden [2B, 128] (and mu_out [2B, 12]) likewise; act_mirror = (src, sign) of M_a (int32 / float32 sequences of 12: (M_a v)[a] = sign[a]
    v[src[a]]).  stats float64[6]: entries 1..4 as actor_head_loss_backward, entry 5 += sum_r |mu(M_o x_r) - M_a mu(x_r)|^2.  The PPO terms see rows
    [0, B) only; the output-layer and bias gradients cover all 2B rows.  finish: as for actor_head_loss_backward."""
    _need_cuda(h, weight, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, g_hidden, grad_weight, grad_bias, grad_bias_hidden,
               grad_logstd, stats, scratch)
    if h.shape[0] % 2 or g_hidden.shape[0] != h.shape[0] or stats.numel() < 6 or (mu_out is not None and mu_out.shape[0] != h.shape[0]):
        raise ValueError("actor_head_sym_loss_backward: h, g_hidden (and mu_out) of 2B rows, stats of 6 entries")
    B = h.shape[0] // 2
    if actions.shape[0] != B or old_mu.shape[0] != B or old_logp.shape[0] != B or adv.shape[0] != B:
        raise ValueError("actor_head_sym_loss_backward: actions, old_mu, old_logp and adv of B rows")
    src, sign = (C.c_int32 * 12)(*[int(v) for v in act_mirror[0]]), (C.c_float * 12)(*[float(v) for v in act_mirror[1]])
    args = [h.shape[0] // 2] + [_lib.ptr(t) for t in (h, weight, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats)]
    args += [e_clip, bound_coef, entropy_coef, sym_coef, src, sign]
    args += [_lib.ptr(t) for t in (mu_out, g_hidden, grad_weight, grad_bias, grad_bias_hidden, grad_logstd, stats, scratch)]
    if finish is not None:
        _lib.check(_lib.load().bg_actor_head_sym_partial(*args, finish, _lib.current_stream_ptr()), "bg_actor_head_sym_partial")
    else:
        _lib.check(_lib.load().bg_actor_head_sym(*args, _lib.current_stream_ptr()), "bg_actor_head_sym")


def mirror_rows(x, y, src, sign):
    """y[r, c] = sign[c] * x[r, src[c]] (src[c] = -1: 0) on [rows, cols <= 64] row-major tensors (bg_mirror_rows): the mirror images of a batch of
    network inputs.  src / sign: sequences of cols, sign +-1."""
    _need_cuda(x, y)
    rows, cols = x.shape
    if y.shape != x.shape or len(src) != cols or len(sign) != cols:
        raise ValueError("mirror_rows: x and y of one shape, src / sign of its width")
    _lib.check(_lib.load().bg_mirror_rows(rows, cols, (C.c_int32 * cols)(*[int(v) for v in src]), (C.c_float * cols)(*[float(v) for v in sign]),
                                          _lib.ptr(x), _lib.ptr(y), _lib.current_stream_ptr()), "bg_mirror_rows")
    return y


def partner_rows(x, x_last, dones, time_outs, y, mode="next", seed=0, update=0, epoch=0):
    """The partner rows of the action-smoothness loss (bg_partner_rows): y[t, e] = x[t, e] + u (x+ - x[t, e]) on x / y [T, N, cols] and x_last [N, cols],
    x+ = x[t + 1, e] (x_last[e] behind the last step); where dones[t, e] or time_outs[t, e] (bool or uint8 [T, N]) is set, y[t, e] = x[t, e].  mode
    "next": u = 1, a bit-exact copy; "interpolate": u in [0, 1), one Philox draw per row on the key (seed) and the counter (t N + e, update, 30, epoch)."""
    _need_cuda(x, x_last, dones, time_outs, y)
    if mode not in ("next", "interpolate"):
        raise ValueError(f"partner_rows: mode must be \"next\" or \"interpolate\", got {mode!r}")
    T, N, cols = x.shape
    if y.shape != x.shape or x_last.shape != (N, cols) or dones.shape != (T, N) or time_outs.shape != (T, N):
        raise ValueError("partner_rows: x and y [T, N, cols], x_last [N, cols], dones and time_outs [T, N]")
    if not all(t.is_contiguous() for t in (x, x_last, dones, time_outs, y)) or x.dtype != torch.float32 or x_last.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("partner_rows: contiguous tensors, float32 rows")
    if any(t.dtype not in (torch.bool, torch.uint8) for t in (dones, time_outs)):
        raise ValueError("partner_rows: dones and time_outs of one byte per flag (bool or uint8)")
    _lib.check(_lib.load().bg_partner_rows(T, N, cols, _lib.ptr(x), _lib.ptr(x_last), _lib.ptr(dones), _lib.ptr(time_outs),
                                           _lib.PARTNER_INTERPOLATE if mode == "interpolate" else _lib.PARTNER_NEXT, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(update) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, _lib.ptr(y), _lib.current_stream_ptr()), "bg_partner_rows")
    return y


def critic_head_backward(h, weight, values, returns, g_hidden, grad_weight, grad_bias, grad_bias_hidden, stats, scratch, finish=None):
    """Backward of mean((values - returns)^2) (runner.py:148) through the 128 -> 1 output layer; stats[0] += sum of squared errors.
    finish: as for actor_head_loss_backward."""
    _need_cuda(h, weight, values, returns, g_hidden, grad_weight, grad_bias, grad_bias_hidden, stats, scratch)
    args = [h.shape[0]] + [_lib.ptr(t) for t in (h, weight, values, returns, g_hidden, grad_weight, grad_bias, grad_bias_hidden, stats, scratch)]
    if finish is not None:
        _lib.check(_lib.load().bg_critic_head_backward_partial(*args, finish, _lib.current_stream_ptr()), "bg_critic_head_backward_partial")
    else:
        _lib.check(_lib.load().bg_critic_head_backward(*args, _lib.current_stream_ptr()), "bg_critic_head_backward")


def reduce_group(problems):
    """Run the deferred reductions of a list of _lib.ReduceProblem descriptors in one launch on the current stream (bg_reduce_group)."""
    for k in range(0, len(problems), 8):  # the launch takes up to 8 descriptors (networks with more hidden layers than the reference's: several launches)
        part = problems[k : k + 8]
        arr = (_lib.ReduceProblem * len(part))(*part)
        _lib.check(_lib.load().bg_reduce_group(arr, len(part), _lib.current_stream_ptr()), "bg_reduce_group")


def surrogate_loss(old_actions_log_prob, actions_log_prob, advantages, e_clip=0.2):
    """Reference utils/utils.py:47-52, kept for API parity (plain torch ops on the caller's device; the
    training loop uses ppo_loss_fused instead)."""
    ratio = torch.exp(actions_log_prob - old_actions_log_prob)
    return torch.max(-advantages * ratio, -advantages * torch.clamp(ratio, 1.0 - e_clip, 1.0 + e_clip)).mean()
