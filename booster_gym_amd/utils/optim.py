"""FlatAdam: Adam on one flat fp32 buffer, the optimiser of every trained network of this build (PPO's critic / actor / logstd in utils/runner.py, the
estimator's in utils/estimator.py, the distilled student's in utils/distill.py)."""
import ctypes

import torch

from .. import _lib


class FlatAdam:
    """Adam state on one flat fp32 buffer, stepped by bg_adam_step.  Exposes a torch.optim.Adam-compatible state_dict."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0):
        self.params = list(params)
        dev = self.params[0].device
        self.sizes = [p.numel() for p in self.params]
        # every tensor starts on a 16-byte boundary of the flat buffer (the MFMA actor kernel reads weight rows with 16-byte loads);
        # the padding floats stay zero in params / grads / moments, so norms, Adam and the all-reduce are unaffected
        self.offsets, n = [], 0
        for k in self.sizes:
            self.offsets.append(n)
            n += (k + 3) // 4 * 4
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        for p, k, off in zip(self.params, self.sizes, self.offsets):
            self.flat[off : off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off : off + k].view_as(p)
            p.grad = self.grad[off : off + k].view_as(p)
        self.lr = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self.betas, self.eps, self.max_grad_norm = betas, eps, max_grad_norm
        self.step_count = 0
        self._gnorm = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)  # bg_optimizer_step's ticket
        self._tail_sync = torch.zeros(4, dtype=torch.int32, device=dev)  # bg_update_tail's ticket and squared-norm pieces
        self._tail_norm = torch.zeros(_lib.TAIL_MAX_BLOCKS, dtype=torch.float64, device=dev)

    def zero_grad(self):
        self.grad.zero_()

    def step(self):
        self.step_count += 1
        _lib.check(_lib.load().bg_adam_step(self.flat.numel(), _lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.exp_avg),
                                            _lib.ptr(self.exp_avg_sq), _lib.ptr(self.lr), self.step_count, self.betas[0], self.betas[1], self.eps,
                                            self.max_grad_norm, _lib.ptr(self._gnorm), _lib.current_stream_ptr()), "bg_adam_step")

    def _opt_args(self, stats, stats_acc, stats_last, kl_index, count, desired_kl, grad_logstd, ls_off, lr_min, lr_max):
        """The arguments bg_optimizer_step and bg_update_tail share, from `n` to `lr_max` (the step is counted by the caller)."""
        return [self.flat.numel(), _lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(self.lr), self.step_count,
                self.betas[0], self.betas[1], self.eps, self.max_grad_norm, _lib.ptr(grad_logstd), int(ls_off), 0 if grad_logstd is None else grad_logstd.numel(),
                _lib.ptr(stats), _lib.ptr(stats_acc), _lib.ptr(stats_last), stats.numel(), int(kl_index), float(count), desired_kl, lr_min, lr_max]

    @staticmethod
    def _sums_args(wgrad, reductions):
        """The two descriptor lists of bg_update_tail / bg_update_tail_sums: wgrad = (descriptor array, count) of a weight-gradient launch made without its
        finish (GroupedWeightGrad.run(..., partial=True)) or None, reductions = the deferred _lib.ReduceProblem descriptors."""
        warr, wn = wgrad if wgrad is not None else (None, 0)
        rarr = (_lib.ReduceProblem * len(reductions))(*reductions) if reductions else None
        return [warr, wn, rarr, len(reductions) if reductions else 0]

    def step_fused(self, stats, stats_acc, stats_last, kl_index, count, desired_kl, grad_logstd=None, ls_off=0, lr_min=1e-5, lr_max=1e-2, mirrors=None):
        """clip + Adam + KL learning-rate rule + statistics bookkeeping in one launch (bg_optimizer_step): what `step()`, `adapt_lr()` and the
        runner's `stats_acc += stats` / zero fills do as seven dependent launches."""
        self.step_count += 1
        args = self._opt_args(stats, stats_acc, stats_last, kl_index, count, desired_kl, grad_logstd, ls_off, lr_min, lr_max)
        _lib.check(_lib.load().bg_optimizer_step(*args, _lib.ptr(self._ticket), None if mirrors is None else ctypes.addressof(mirrors),
                                                 0 if mirrors is None else len(mirrors), _lib.current_stream_ptr()), "bg_optimizer_step")

    def step_tail(self, wgrad, reductions, stats, stats_acc, stats_last, kl_index, count, desired_kl, grad_logstd=None, ls_off=0, lr_min=1e-5, lr_max=1e-2,
                  mirrors=None):
        """`step_fused` together with the sums in front of it (bg_update_tail: two launches for four); wgrad, reductions: see _sums_args."""
        self.step_count += 1
        args = self._opt_args(stats, stats_acc, stats_last, kl_index, count, desired_kl, grad_logstd, ls_off, lr_min, lr_max)
        _lib.check(_lib.load().bg_update_tail(*self._sums_args(wgrad, reductions), *args, _lib.ptr(self._tail_sync), _lib.ptr(self._tail_norm),
                                              None if mirrors is None else ctypes.addressof(mirrors), 0 if mirrors is None else len(mirrors),
                                              _lib.current_stream_ptr()), "bg_update_tail")

    def step_separate(self, stats, stats_acc, stats_last, kl_index, count, desired_kl, grad_logstd=None, ls_off=0, lr_min=1e-5, lr_max=1e-2, lr_restart=None):
        """What `step_fused` does, as separate launches: `step()` (bg_adam_step), `adapt_lr()` (bg_adapt_lr) and the bookkeeping of the kernels' last
        ticket in torch.  lr_restart: a learning rate to start the KL rule from instead of the stored one (the first step after a restore, which was
        taken at the stored rate)."""
        if grad_logstd is not None:
            self.grad[ls_off : ls_off + grad_logstd.numel()].copy_(grad_logstd)
        self.step()
        if lr_restart is not None:
            self.lr.fill_(float(lr_restart))
        self.adapt_lr(stats[kl_index : kl_index + 1], count, desired_kl, lr_min, lr_max)
        stats_acc += stats
        stats_last.copy_(stats)
        stats.zero_()
        if grad_logstd is not None:
            grad_logstd.zero_()

    def tail_sums(self, wgrad, reductions):
        """Launch (1) of `step_tail` alone (bg_update_tail_sums): the ranks of a multi-GPU job average the gradient between the sums and `step_fused`."""
        _lib.check(_lib.load().bg_update_tail_sums(*self._sums_args(wgrad, reductions), _lib.ptr(self._tail_norm), _lib.current_stream_ptr()),
                   "bg_update_tail_sums")

    def adapt_lr(self, kl_sum, count, desired_kl, lr_min=1e-5, lr_max=1e-2):
        _lib.check(_lib.load().bg_adapt_lr(_lib.ptr(kl_sum), float(count), desired_kl, lr_min, lr_max, _lib.ptr(self.lr), _lib.current_stream_ptr()),
                   "bg_adapt_lr")

    def state_dict(self):
        state = {}
        for i, (k, off) in enumerate(zip(self.sizes, self.offsets)):
            state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": self.exp_avg[off : off + k].view_as(self.params[i]).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off : off + k].view_as(self.params[i]).clone()}
        group = {"lr": float(self.lr.item()), "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(self.sizes)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        for i, (k, off) in enumerate(zip(self.sizes, self.offsets)):
            st = sd["state"].get(i)
            if st is not None:
                self.exp_avg[off : off + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off : off + k].copy_(st["exp_avg_sq"].reshape(-1))
                self.step_count = int(float(st["step"]))
        self.lr.fill_(float(sd["param_groups"][0]["lr"]))
