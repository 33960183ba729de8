"""The exploration noise of every sampling launch is the draw the header documents: actions = mu + exp(logstd) n with
n = rand4(seed, row, counter, RS_ACTOR + g).n[k] for action a = 4 g + k, against oracle/task_ref.py's Philox and Box-Muller -- the one stochastic
stream that was pinned only to other kernels so far.  With logstd = 0, actions - mu is the draw up to one rounding of the subtraction.

Entry points: bg_actor_sample (packed), bg_actor_sample_mlp, bg_actor_sample_mlp_scan, bg_actor_sample_est, bg_actor_sample_gru, bg_distill_act,
bg_distill_act_hist, bg_distill_act_mix (beta = 0.5, teacher_noise 1 and 0), bg_distill_act_gru (beta = 0.5); N in (17, 250); (seed, counter) in
((5, 3), (987654321 | 3 << 32, 2^32 - 1)): the second has the seed's high word and a full counter word in use.  In the mixed launches the mean behind
a row's action is the teacher's where tests/test_gpu_distill_dagger._choice, the host's restatement of the coin, says so, and with teacher_noise = 0
those rows carry no noise (asserted: their action is the teacher's mean, bit for bit).

BOUND.  The device evaluates Box-Muller with __sincosf and its own logf, the oracle with numpy's float32 functions.  Measured on an MI355X, the largest
|(actions - mu) - oracle draw| over all ten launches, both sizes and both pairs: MEASURED = 2.27e-6 (bg_actor_sample and its siblings at N = 250,
seed 5; 1.3e-6 to 1.6e-6 at N = 17; the subtraction's rounding is part of the figure), at draws of up to 3.9.
  BOUND = 4 x MEASURED (arguments near 2 pi that another N would reach) + one fp32 ulp of the call's largest |action| (the subtraction)
        = 9.1e-6 + 2.4e-7 .. 4.8e-7, a hundred times below the 1e-3 it has to stay under: a wrong row, group, entry or stream moves a draw by O(1).

Controls on the reference side, at N = 250 (at N = 17 the rows 0 .. 15 are their own row % 16): the oracle's draw at stream RS_ACTOR + g + 1, at row
row % 16, with k reversed, and with .u in place of .n each miss BOUND on more than 90 % of the entries.  Measured: 100 %, 93.6 % (the rows 16 .. 249 of
250), 100 % and 100 %.

With the model's own logstd: actions = mu + exp(logstd) * draw within 4 ulp of the largest |action|, the draw taken from the logstd = 0 call.
Measured: 1 ulp at most."""
import numpy as np
import pytest
import torch

from oracle.task_ref import RS_ACTOR, rand4
from test_action_noise_ref import action_noise
from test_gpu_distill import _descs
from test_gpu_distill_dagger import _choice
from test_gpu_distill_memory import _student

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 12
SIZES = (17, 250)
PAIRS = ((5, 3), (987654321 | 3 << 32, 2 ** 32 - 1))
MEASURED = 2.27e-6  # the largest |(actions - mu) - oracle draw| of any launch on an MI355X (the docstring)


def _ulp_of(x):
    """One fp32 ulp of |x|."""
    return float(np.spacing(np.float32(abs(x))))


def _bound(top):
    return 4.0 * MEASURED + _ulp_of(top)


def _with_logstd(model):
    with torch.no_grad():
        model.logstd.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    return model


def _net(num_obs, hidden, seed, **kw):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(seed)
    return _with_logstd(ActorCritic(A, num_obs, 14, hidden, **kw).to(DEV))


def _rows(n, width, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + n)
    return (torch.randn(n, width, generator=g) * 0.7).to(DEV)


def _outs(n, k=2):
    return [torch.full((n + 16, A), 7.0, device=DEV) for _ in range(k)]


def _done(outs, n):
    torch.cuda.synchronize()
    for t in outs:
        assert torch.all(t[n:] == 7.0), "rows past N were written"
    return [t[:n] for t in outs]


class _Through:
    """An entry point reached through ActorCritic.sample_actions: the packed launch, the descriptor launch, its scan form, the estimator's."""

    def __init__(self, entry, model, width, scan=0):
        self.entry, self.model, self.width, self.scan = entry, model, width, scan

    def __call__(self, n, seed, counter):
        from booster_gym_amd import _lib

        lib, seen = _lib.load(), []
        mu, act = _outs(n)
        kw = dict(est_out=torch.empty(n, A, device=DEV)) if self.model.has_estimator else {}
        inner = getattr(lib, self.entry)
        setattr(lib, self.entry, lambda *a: (seen.append(1), inner(*a))[1])
        try:
            self.model.sample_actions(_rows(n, self.width), act[:n], seed, counter, mu_out=mu[:n], scan=self.scan, **kw)
        finally:
            setattr(lib, self.entry, inner)
        assert seen == [1], f"sample_actions did not run {self.entry}"
        mu, act = _done([mu, act], n)
        return mu, act, torch.ones(n, dtype=torch.bool, device=DEV)


class _Gru:
    entry = "bg_actor_sample_gru"

    def __init__(self):
        self.model = _student(128)

    def __call__(self, n, seed, counter):
        from booster_gym_amd import _lib

        m, p = self.model, _lib.ptr
        sd, ns = _descs(m)
        h = _rows(n, 128, seed=3) * 0.5
        reset = (torch.arange(n, device=DEV) % 5 == 0).to(torch.uint8)
        h_out, mu, act = torch.empty(n, 128, device=DEV), *_outs(n)
        _lib.check(_lib.load().bg_actor_sample_gru(n, p(_rows(n, 47)), 47, m.gru_descriptor(), ns, sd, p(m.logstd), seed, counter, p(reset), p(h), p(h_out), p(mu), p(act),
                                                   _lib.current_stream_ptr()), self.entry)
        mu, act = _done([mu, act], n)
        return mu, act, torch.ones(n, dtype=torch.bool, device=DEV)


class _Distill:
    """The two-network launches: P = 45 scan points behind the teacher's 47 columns; the history form with a student of 3 frames on rows of its own;
    the mixed forms at beta = 0.5; the recurrent student's."""

    P = 45

    def __init__(self, entry, noise=1):
        self.entry, self.noise = entry, noise
        self.frames = 3 if entry == "bg_distill_act_hist" else 1
        self.teacher = _net(47 + self.P, (256, 128, 128), 9)
        self.model = _student(128, P=self.P) if entry == "bg_distill_act_gru" else _net(47 * self.frames, (256, 128, 128), 8)

    def __call__(self, n, seed, counter):
        from booster_gym_amd import _lib

        m, t, p, lib, P = self.model, self.teacher, _lib.ptr, _lib.load(), self.P
        (sd, ns), (td, nt) = _descs(m), _descs(t)
        tobs = _rows(n, 47 + P)
        sobs = tobs if self.frames == 1 else _rows(n, 47 * self.frames, seed=1)
        s_mu, act, t_mu = outs = _outs(n, 3)
        tail = [p(s_mu), p(act), p(t_mu), _lib.current_stream_ptr()]
        two = [n, p(tobs), tobs.shape[1], p(sobs), sobs.shape[1], ns, sd, nt, td, P, p(m.logstd), seed, counter]
        if self.entry == "bg_distill_act":
            rc = lib.bg_distill_act(n, p(tobs), tobs.shape[1], ns, sd, nt, td, P, p(m.logstd), seed, counter, *tail)
        elif self.entry == "bg_distill_act_hist":
            rc = lib.bg_distill_act_hist(*two, *tail)
        elif self.entry == "bg_distill_act_mix":
            rc = lib.bg_distill_act_mix(*two, 0.5, self.noise, *tail)
        else:
            h, h_out = _rows(n, 128, seed=3) * 0.5, torch.empty(n, 128, device=DEV)
            rc = lib.bg_distill_act_gru(n, p(tobs), tobs.shape[1], nt, td, P, m.gru_descriptor(), ns, sd, p(m.logstd), seed, counter, 0.5, self.noise, None, p(h),
                                        p(h_out), *tail)
        _lib.check(rc, self.entry)
        s_mu, act, t_mu = _done(outs, n)
        if self.entry in ("bg_distill_act", "bg_distill_act_hist"):
            return s_mu, act, torch.ones(n, dtype=torch.bool, device=DEV)
        teacher_acts = _choice(n, counter, 0.5, seed=seed)
        assert 0 < int(teacher_acts.sum()) < n
        mean = torch.where(teacher_acts.view(n, 1), t_mu, s_mu)
        if self.noise:
            return mean, act, torch.ones(n, dtype=torch.bool, device=DEV)
        assert torch.equal(act[teacher_acts], t_mu[teacher_acts]), "teacher_noise = 0: a teacher-driven row is the teacher's mean"
        return mean, act, ~teacher_acts


def _entry_points():
    from test_gpu_estimator import _model as est_model

    return {"bg_actor_sample": lambda: _Through("bg_actor_sample", _net(47, (256, 128, 128), 1), 47),
            "bg_actor_sample_mlp": lambda: _Through("bg_actor_sample_mlp", _net(47, (512, 256, 128), 2), 47),
            "bg_actor_sample_mlp_scan": lambda: _Through("bg_actor_sample_mlp_scan", _net(47 + 45, (256, 128, 128), 3), 47 + 45, scan=45),
            "bg_actor_sample_est": lambda: _Through("bg_actor_sample_est", _with_logstd(est_model(1, 4, (256, 128), (256, 128, 128))), 47),
            "bg_actor_sample_gru": _Gru,
            "bg_distill_act": lambda: _Distill("bg_distill_act"),
            "bg_distill_act_hist": lambda: _Distill("bg_distill_act_hist"),
            "bg_distill_act_mix:teacher_noise=1": lambda: _Distill("bg_distill_act_mix", 1),
            "bg_distill_act_mix:teacher_noise=0": lambda: _Distill("bg_distill_act_mix", 0),
            "bg_distill_act_gru": lambda: _Distill("bg_distill_act_gru", 1)}


ENTRY_POINTS = ("bg_actor_sample", "bg_actor_sample_mlp", "bg_actor_sample_mlp_scan", "bg_actor_sample_est", "bg_actor_sample_gru", "bg_distill_act",
                "bg_distill_act_hist", "bg_distill_act_mix:teacher_noise=1", "bg_distill_act_mix:teacher_noise=0", "bg_distill_act_gru")


def _controls(seed, n, counter):
    """name: [n][12] of what a sampler that addressed the generator wrongly would have drawn."""
    rows = np.arange(n)
    groups = lambda f: np.concatenate([f(g) for g in range(A // 4)], axis=1)
    return {"stream RS_ACTOR + g + 1": groups(lambda g: rand4(seed, rows, counter, RS_ACTOR + g + 1)[1]),
            "row % 16": action_noise(seed, rows % 16, counter),
            "k reversed": groups(lambda g: rand4(seed, rows, counter, RS_ACTOR + g)[1][:, ::-1]),
            ".u for .n": groups(lambda g: rand4(seed, rows, counter, RS_ACTOR + g)[0])}


def measure(name):
    """Per (N, seed, counter): the largest |(actions - mu) - oracle draw| over the rows that carry noise, the largest |action| of the logstd = 0 call,
    the share of entries on which each control differs from the launch by more than `unit`, and the error of the real-logstd call in ulps."""
    ep = _entry_points()[name]()
    model, out = ep.model, []
    saved = model.logstd.detach().clone()
    for n in SIZES:
        for seed, counter in PAIRS:
            mu, act, noisy = ep(n, seed, counter)
            with torch.no_grad():
                model.logstd.zero_()
            try:
                mu0, act0, noisy0 = ep(n, seed, counter)
            finally:
                with torch.no_grad():
                    model.logstd.copy_(saved)
            assert torch.equal(mu0, mu) and torch.equal(noisy0, noisy) and int(noisy.sum()) > 0
            draw = (act0 - mu0)[noisy]
            want = torch.from_numpy(action_noise(seed, np.arange(n), counter)).to(DEV)[noisy]
            err, top = (draw - want).abs().max().item(), act0.abs().max().item()
            rec = dict(n=n, seed=seed, counter=counter, err=err, top=top, draw=draw, noisy=noisy, controls={})
            if n == max(SIZES):
                rec["controls"] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)[noisy] for k, v in _controls(seed, n, counter).items()}
            real = (mu + torch.exp(saved) * (act0 - mu0))[noisy]
            rec["real_err"], rec["real_top"] = (act[noisy] - real).abs().max().item(), act.abs().max().item()
            print(f"{name} N {n} seed {seed} counter {counter}: |draw - oracle|max {err:.3e} (|action|max {top:.3f}, |draw|max {draw.abs().max().item():.3f}); "
                  f"with the model's logstd {rec['real_err']:.3e} = {rec['real_err'] / _ulp_of(rec['real_top']):.2f} ulp of |action|max {rec['real_top']:.3f}")
            out.append(rec)
    return out


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_sampled_actions_carry_the_documented_draw(name):
    assert MEASURED is not None and MEASURED <= 2.5e-4 and 4.0 * MEASURED <= 1e-3
    for rec in measure(name):
        bound = _bound(rec["top"])
        assert bound <= 1e-3
        assert rec["err"] <= bound, (name, rec["n"], rec["seed"], rec["counter"], rec["err"], bound)
        assert rec["draw"].abs().max().item() > 1.0
        for k, wrong in rec["controls"].items():
            missed = ((rec["draw"] - wrong).abs() > bound).float().mean().item()
            print(f"{name} N {rec['n']} seed {rec['seed']}: control '{k}' misses the bound on {100 * missed:.1f} % of the entries")
            assert missed > 0.9, (name, k, missed)
        assert rec["real_err"] <= 4.0 * _ulp_of(rec["real_top"]), (name, rec["n"], rec["real_err"], rec["real_top"])
