"""Teacher-student distillation on the GPU: the behaviour-cloning head (bg_distill_head) against float64 autograd, the rollout's two-network launch
(bg_distill_act) against its stand-alone siblings (bitwise) and float64, one Distiller iteration against a float64 autograd restatement (clip + Adam),
the student checkpoint through Runner / play / export_model.py, and run-to-run reproducibility.

Bounds: tests/test_gpu_head.py's (outputs of 128-term dot products 2e-5, sums over the rows 1e-4 relative to the largest entry -- the critic head's
bound, the same form of loss -- float64 statistics 1e-5) and tests/test_gpu_actor_heights.py's (the actor's mean 2e-5 max(1, |ref|max); parameters
after an update rtol 1e-3, atol 2e-6 at the learning rate 1e-5)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 12


def rel(x, r):
    return ((x.double() - r.double()).abs().max() / max(1e-30, r.double().abs().max())).item()


# ------------------------------------------------------------------ 1. the head
def _head_data(B, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    h = torch.nn.functional.elu(torch.randn(B, 128, generator=g)).to(DEV)
    W = (torch.randn(A, 128, generator=g) * 0.1).to(DEV)
    b = (torch.randn(A, generator=g) * 0.1).to(DEV)
    target = torch.randn(B, A, generator=g).to(DEV)  # drawn independently of mu: |mu - target| is O(1), the gradient no cancellation
    return h, W, b, target


def _run_head(B, h, W, b, target, partial=False):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import head_scratch, reduce_group

    pad = 70  # sentinel rows past B
    mu = torch.full((B + pad, A), 7.0, device=DEV)
    g_hidden = torch.full((B + pad, 128), 7.0, device=DEV)
    dW, db, dbh = (torch.full(s, float("nan"), device=DEV) for s in ((A, 128), (A,), (128,)))
    st = torch.zeros(1, dtype=torch.float64, device=DEV)
    scratch = head_scratch(DEV)
    args = [B] + [_lib.ptr(t) for t in (h, W, b, target, mu, g_hidden, dW, db, dbh, st, scratch)]
    lib = _lib.load()
    if partial:
        fin = _lib.ReduceProblem()
        _lib.check(lib.bg_distill_head_partial(*args, fin, _lib.current_stream_ptr()), "bg_distill_head_partial")
        torch.cuda.synchronize()
        assert torch.isnan(dW).all() and torch.isnan(db).all() and torch.isnan(dbh).all() and st.item() == 0.0  # nothing reduced yet
        reduce_group([fin])
    else:
        _lib.check(lib.bg_distill_head(*args, _lib.current_stream_ptr()), "bg_distill_head")
    torch.cuda.synchronize()
    assert torch.all(mu[B:] == 7.0) and torch.all(g_hidden[B:] == 7.0), "rows past B were written"
    return dict(mu=mu[:B], g_hidden=g_hidden[:B], dW=dW, db=db, dbh=dbh, st=st)


@pytest.mark.parametrize("B", [1, 129, 1000])
def test_head_matches_float64_autograd_and_is_deterministic(B):
    """B = 1: one row; 129: one row past 128 rows (two full 64-row tiles); 1000: a ragged many-tile case."""
    h, W, b, target = _head_data(B, 10 + B)
    out = _run_head(B, h, W, b, target)
    h64, W64, b64 = h.double().requires_grad_(), W.double().requires_grad_(), b.double().requires_grad_()
    mu_ref = h64 @ W64.t() + b64
    sse = ((mu_ref - target.double()) ** 2).sum()
    (sse / (A * B)).backward()
    g_ref = h64.grad * torch.where(h > 0, torch.ones_like(h), h + 1).double()  # dL/dz of the ELU layer, the derivative from its output
    errs = {"mu": rel(out["mu"], mu_ref.detach()), "g_hidden": rel(out["g_hidden"], g_ref), "grad_W": rel(out["dW"], W64.grad),
            "grad_b": rel(out["db"], b64.grad), "grad_b_hidden": rel(out["dbh"], g_ref.sum(0)),
            "stats[0]": abs(out["st"].item() - sse.item()) / sse.item()}
    print(f"B {B}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"; |mu|max / |mu - target|max = "
          f"{(mu_ref.abs().max() / (mu_ref - target.double()).abs().max()).item():.3f}")
    assert errs["mu"] < 2e-5
    for k in ("g_hidden", "grad_W", "grad_b", "grad_b_hidden"):
        assert errs[k] < 1e-4, (k, errs[k])
    assert errs["stats[0]"] < 1e-5
    again, later = _run_head(B, h, W, b, target), _run_head(B, h, W, b, target, partial=True)
    for k in out:
        assert torch.equal(out[k], again[k]), ("two calls", k)
        assert torch.equal(out[k], later[k]), ("_partial + bg_reduce_group", k)


# ------------------------------------------------------------------ 2. the rollout's launch
def _descs(model):
    from booster_gym_amd import _lib

    lin = [m for m in model.actor if isinstance(m, torch.nn.Linear)]
    return (_lib.MlpLayerDesc * len(lin))(*[_lib.MlpLayerDesc(l.weight.data_ptr(), l.bias.data_ptr(), l.in_features, l.out_features) for l in lin]), len(lin)


def _distill_act(student, teacher, obs, P, seed, counter, n=None):
    from booster_gym_amd import _lib

    n = obs.shape[0] if n is None else n
    outs = [torch.full((n + 16, A), 7.0, device=DEV) for _ in range(3)]  # student mu, actions, teacher mu
    (sd, ns), (td, nt) = _descs(student), _descs(teacher)
    _lib.check(_lib.load().bg_distill_act(n, _lib.ptr(obs), obs.shape[1], ns, sd, nt, td, P, _lib.ptr(student.logstd), seed, counter, *[_lib.ptr(t) for t in outs],
                                          _lib.current_stream_ptr()), "bg_distill_act")
    torch.cuda.synchronize()
    for t in outs:
        assert torch.all(t[n:] == 7.0), "rows past N were written"
    return [t[:n] for t in outs]


@pytest.mark.parametrize("H,P,s_hidden,t_hidden", [(1, 187, (256, 128, 128), (512, 256, 128)), (3, 45, (128, 128), (256, 128, 128))])
def test_distill_act_equals_its_stand_alone_launches_bitwise(H, P, s_hidden, t_hidden):
    """N = 130 is no multiple of the 16-row tile.  Case (a): the student alone runs the 256-wide LDS form, the teacher the 512-wide one."""
    from test_gpu_frame_stack import _actor_f64

    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(100 + H)
    N, F, seed, counter = 130, 47 * H, 987654321, 23
    teacher = ActorCritic(A, F + P, 14 + P, t_hidden).to(DEV)
    student = ActorCritic(A, F, 14 + P, s_hidden).to(DEV)
    with torch.no_grad():
        student.logstd.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    obs = torch.randn(N, F + P, device=DEV)
    s_mu, act, t_mu = _distill_act(student, teacher, obs, P, seed, counter)
    # the teacher: bg_actor_sample_mlp_scan on the same rows, and float64
    mu_ref, tmp = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    teacher.sample_actions(obs, tmp, 1, 2, mu_out=mu_ref, scan=P)
    assert torch.equal(t_mu, mu_ref)
    ref = _actor_f64(teacher, obs)
    err = (t_mu.double() - ref).abs().max().item()
    print(f"H {H} P {P}: teacher max error {err:.3e}, |ref|max {ref.abs().max().item():.3f}")
    assert err <= 2e-5 * max(1.0, ref.abs().max().item())
    # the student: bg_actor_sample_mlp on a contiguous copy of the prefix columns, same seed and counter
    prefix = obs[:, :F].contiguous()
    (sd, ns) = _descs(student)
    mu2, act2 = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp(N, _lib.ptr(prefix), ns, sd, _lib.ptr(student.logstd), seed, counter, _lib.ptr(mu2), _lib.ptr(act2),
                                               _lib.current_stream_ptr()), "bg_actor_sample_mlp")
    torch.cuda.synchronize()
    assert torch.equal(s_mu, mu2) and torch.equal(act, act2)
    assert (s_mu.double() - _actor_f64(student, prefix)).abs().max().item() <= 2e-5 * max(1.0, _actor_f64(student, prefix).abs().max().item())
    assert not torch.equal(act, s_mu)  # (the noise is on)
    # the student does not see the scan; the teacher does
    obs2 = obs.clone(); obs2[:, F:] += 1.0
    s_mu3, act3, t_mu3 = _distill_act(student, teacher, obs2, P, seed, counter)
    assert torch.equal(s_mu3, s_mu) and torch.equal(act3, act) and not torch.equal(t_mu3, t_mu)
    # student_mu may be NULL
    (td, nt), a4, t4 = _descs(teacher), torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_distill_act(N, _lib.ptr(obs), F + P, ns, sd, nt, td, P, _lib.ptr(student.logstd), seed, counter, None, _lib.ptr(a4), _lib.ptr(t4),
                                          _lib.current_stream_ptr()), "bg_distill_act")
    torch.cuda.synchronize()
    assert torch.equal(a4, act) and torch.equal(t4, t_mu)


def test_distill_act_argument_errors():
    from booster_gym_amd import _lib

    lib, o = _lib.load(), torch.zeros(4, 600, device=DEV)
    p = o.data_ptr()
    net = lambda k_in: (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(p, p, k_in, 128), _lib.MlpLayerDesc(p, p, 128, 128), _lib.MlpLayerDesc(p, p, 128, 12))
    call = lambda stride, s, t, scan: lib.bg_distill_act(4, _lib.ptr(o), stride, 3, net(s), 3, net(t), scan, _lib.ptr(o), 0, 0, None, _lib.ptr(o), _lib.ptr(o), None)
    assert call(235, 47, 234, 187) == -4 and b"obs_stride" in lib.bg_last_error()   # obs_stride is not the teacher's `in`
    assert call(234, 48, 234, 187) == -4 and b"student" in lib.bg_last_error()      # a student `in` that is not 47 H
    assert call(234, 94, 234, 187) == -4 and b"student" in lib.bg_last_error()      # ... or not the teacher's 47 H
    assert call(484, 470, 484, 14) == -4 and b"teacher" in lib.bg_last_error()      # a teacher `in` above BG_ACTOR_MAX_INPUT


# ------------------------------------------------------------------ 3. - 5. the Distiller
GRID_5x3 = {"terrain.measured_points_x": [-0.2, -0.1, 0.0, 0.1, 0.2], "terrain.measured_points_y": [-0.1, 0.0, 0.1]}
H, P, N, T = 2, 15, 64, 4


def _cfg(teacher=None, frames=H, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "env.frame_stack": frames,
          "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 * frames + P, "env.num_privileged_obs": 14 + P,
          "distillation.num_epochs": 3, "distillation.learning_rate": 1.0e-5, "distillation.teacher_checkpoint": teacher, **GRID_5x3}
    ov.update(over)
    return load_cfg("T1", ov)


def _save_teacher(path, frames=H, **extra):
    """A seeded perceptive ActorCritic saved as a checkpoint of the test's config (47 `frames` + 15 observations, 29 privileged)."""
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.terrain import height_scan_points

    torch.manual_seed(5)
    m = ActorCritic(A, 47 * frames + P, 14 + P)
    pts = torch.tensor(height_scan_points(_cfg()["terrain"])[1], dtype=torch.float).reshape(P, 2)
    torch.save({"model": m.state_dict(), "height_points": pts, **extra}, path)
    return path


@pytest.fixture(scope="module")
def teacher_ck(tmp_path_factory):
    return _save_teacher(str(tmp_path_factory.mktemp("teacher") / "teacher.pth"))


class _Rec:
    def __init__(self):
        self.stats, self.saved = {}, []

    def record_episode_statistics(self, env, names, it, stats=None):
        env.episode_stats(reset=True)

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        self.saved.append(it)


def _distiller(teacher, frames=H, **over):
    from booster_gym_amd.utils.distill import Distiller

    d = Distiller(cfg=_cfg(teacher, frames, **over))
    d.begin(recorder=_Rec())
    return d


def _check_one_iteration(d, frames, kin, plan, wgrad):
    """rollout() against bg_actor_sample_mlp_scan, update() against float64 autograd + clip_grad_norm_ + torch.optim.Adam on the same rows and labels."""
    F = 47 * frames
    assert (d.student_obs, d.scan, d.env.num_obs) == (F, P, F + P) and d.student.actor[0].in_features == F and d.student.critic[0].in_features == F + 14 + P
    assert d._student_in.shape == (T * N, kin) and (d._sup.mlp.plan.fwd, d._sup.mlp.plan.bwd) == (plan, plan) and all(d._sup.mlp.plan.grouped[:-1])
    assert d._sup.wgrad_terms == wgrad
    assert abs(d.student.logstd[0, 0].item() - math.log(0.1)) < 1e-7
    frozen = lambda: {**{"student." + k: v.clone() for k, v in d.student.state_dict().items() if not k.startswith("actor.")},
                      **{"teacher." + k: v.clone() for k, v in d.teacher.state_dict().items()}}
    before = frozen()
    c0 = d._act_counter
    d.rollout()
    torch.cuda.synchronize()
    assert d._act_counter == c0 + T  # (a step counter as Runner's)
    obses, labels = d.buffer["obses"], d.buffer["teacher_mu"]
    assert tuple(obses.shape) == (T + 1, N, F + P) and tuple(labels.shape) == (T, N, A) and obses[1:, :, F:].std() > 1e-3
    mu, tmp = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    for t in range(T):
        d.teacher.sample_actions(obses[t], tmp, 0, 0, mu_out=mu, scan=P)  # bg_actor_sample_mlp_scan
        assert torch.equal(labels[t], mu), t
    # the restatement: float64 autograd + clip_grad_norm_ + torch.optim.Adam on the same rows and labels
    from booster_gym_amd.utils.model import ActorCritic

    B = T * N
    rows, y = obses[:T].reshape(B, -1)[:, :F].double(), labels.reshape(B, A).double()
    ref = ActorCritic(A, F, 14 + P, d.dcfg.student_hidden).to(DEV)
    ref.load_state_dict(d.student.state_dict())
    ref = ref.double()
    opt, ref_losses = torch.optim.Adam(ref.actor.parameters(), lr=1.0e-5), []
    for _ in range(3):
        opt.zero_grad()
        loss = ((ref.actor(rows) - y) ** 2).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.actor.parameters(), 1.0)
        opt.step()
        ref_losses.append(loss.item())
    assert ref_losses[0] > ref_losses[1] > ref_losses[2] > 0, ref_losses  # (the set-up trains: a failure below points at the code)
    p_start = {k: p.detach().clone() for k, p in d.student.actor.named_parameters()}
    losses = d.update().cpu().tolist()
    torch.cuda.synchronize()
    print("losses", losses, "restatement", ref_losses)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 1e-4 * abs(b), (losses, ref_losses)
    for (k, p), (k2, q) in zip(d.student.actor.named_parameters(), ref.actor.named_parameters()):
        assert k == k2 and not torch.equal(p, p_start[k]), k
        print(k, "max |p - restatement|", (p.double() - q).abs().max().item(), "moved", (q - p_start[k].double()).abs().max().item())
        assert torch.allclose(p.double(), q, rtol=1e-3, atol=2e-6), (k, (p.double() - q).abs().max().item())
    after = frozen()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)  # critic, logstd and the teacher: not a bit moved


def test_one_iteration_matches_the_float64_restatement(teacher_ck):
    """H = 2: the student's 94 columns are padded to 128, so its layers run one by one, and the weight gradients in fp32."""
    _check_one_iteration(_distiller(teacher_ck), H, 128, "layer", 0)


def test_one_iteration_on_the_default_plan_matches_the_float64_restatement(tmp_path):
    """H = 1, the shipped configuration's plan: 47 columns padded to 64 and 256-128-128 run the chained split-bf16 forward and backward launches with the
    9-product bf16 weight gradients (B = 256 rows: whole 128-row slabs).  Same bounds: they are the ones tests/test_gpu_ppo.py takes of these very
    kernels for up to 5 optimiser steps at this learning rate (test_full_update_matches_reference_loop: rtol 1e-3, atol 2e-6)."""
    _check_one_iteration(_distiller(_save_teacher(str(tmp_path / "teacher_h1.pth"), 1), 1), 1, 64, "chain_split", 9)


def test_student_checkpoint_re_enters_runner_play_and_export(teacher_ck, tmp_path):
    from booster_gym_amd.utils.distill import student_cfg_overrides
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import Runner

    d = _distiller(teacher_ck, **{"runner.save_interval": 1})
    d.train_iteration(0)
    assert d.recorder.saved == [1] and set(d.recorder.stats[0]) == {"distill/behaviour_loss"} and np.isfinite(d.recorder.stats[0]["distill/behaviour_loss"])
    ck = d.checkpoint_dict()
    assert set(ck) == {"model", "curriculum", "distillation"}  # no "height_points", no "optimizer" (no terrain curriculum here: no "terrain_levels")
    assert ck["distillation"]["teacher"] == teacher_ck and ck["distillation"]["iteration"] == 1 and ck["distillation"]["loss"] == d.last_loss
    assert set(ck["model"]) == {f"{n}.{i}.{w}" for n in ("actor", "critic") for i in (0, 2, 4, 6) for w in ("weight", "bias")} | {"logstd"}
    path = str(tmp_path / "student.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in d.student.state_dict().items()}
    over = student_cfg_overrides(d.cfg)
    assert over == {"terrain.actor_heights": False, "env.num_observations": 94}
    del d
    r = Runner(test=True, cfg=_cfg(**over, **{"basic.checkpoint": path}))  # everything else unchanged
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert r.play(max_steps=3) == 3
    del r
    with pytest.raises(ValueError, match=r"terrain\.actor_heights"):  # the teacher's config still on
        Runner(test=True, cfg=_cfg(**{"basic.checkpoint": path}))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={path}"], cwd=str(tmp_path), env=env, check=True, timeout=300,
                   capture_output=True, text=True)
    actor = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    m = ActorCritic(A, 94, 14 + P)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    x = torch.linspace(-1, 1, 94).reshape(1, 94)
    y = actor(x)
    assert tuple(y.shape) == (1, A) and torch.allclose(y, m.actor(x), atol=1e-6)


def test_terrain_levels_and_command_curriculum_pass_from_teacher_to_student_checkpoint(tmp_path):
    """With terrain.curriculum the teacher checkpoint's "terrain_levels" and "curriculum" are restored into the env, and the student checkpoint
    carries the env's own on to Runner."""
    from booster_gym_amd.utils.distill import student_cfg_overrides
    from booster_gym_amd.utils.runner import Runner

    L = 6
    cur = {"terrain.curriculum": True, "terrain.num_levels": L, "terrain.max_init_level": 3}
    c = _cfg(**cur)["commands"]
    lv = (torch.arange(N) * 5 % L).to(torch.int32)  # every level, and not the initial draw (levels 0 .. 3)
    prob = torch.linspace(0.05, 0.95, (1 + 2 * c["lin_vel_levels"]) * (1 + 2 * c["ang_vel_levels"])).reshape(1 + 2 * c["lin_vel_levels"], -1)
    teacher = _save_teacher(str(tmp_path / "teacher.pth"), terrain_levels=lv, curriculum=prob)
    d = _distiller(teacher, **cur)
    assert torch.equal(d.env.terrain_levels.cpu().to(torch.int32), lv) and int(d.env.terrain_level_sum().item()) == int(lv.sum())
    assert torch.equal(d.env.curriculum_prob.cpu(), prob)
    d.train_iteration(0)
    assert set(d.recorder.stats[0]) == {"distill/behaviour_loss", "terrain/mean_level"}
    ck, lv1, prob1 = d.checkpoint_dict(), d.env.terrain_levels.clone(), d.env.curriculum_prob.clone()
    assert set(ck) == {"model", "curriculum", "terrain_levels", "distillation"}
    assert torch.equal(ck["terrain_levels"], lv1) and torch.equal(ck["curriculum"], prob1)
    assert abs(d.recorder.stats[0]["terrain/mean_level"] - float(lv1.double().mean())) < 1e-9
    path = str(tmp_path / "student.pth")
    torch.save(ck, path)
    over = student_cfg_overrides(d.cfg)
    del d
    r = Runner(test=True, cfg=_cfg(**over, **cur, **{"basic.checkpoint": path}))
    assert torch.equal(r.env.terrain_levels, lv1) and torch.equal(r.env.curriculum_prob, prob1)
    # a teacher from another env count: the initial draw stays, as in Runner
    bad = _save_teacher(str(tmp_path / "teacher_96.pth"), terrain_levels=lv[:32])
    d = _distiller(bad, **cur)
    assert torch.equal(d.env.terrain_levels.cpu(), torch.from_numpy(d.env._terrain_init[0]).to(d.env.terrain_levels.dtype))


def test_teacher_of_another_config_is_a_value_error(teacher_ck, tmp_path):
    from booster_gym_amd.utils.distill import Distiller

    d = torch.load(teacher_ck, weights_only=True)
    for name, edit, match in (("norm", lambda c: c.update(obs_normalizer={"mean": torch.zeros(3)}), r"empirical_normalization"),
                              ("points", lambda c: c.update(height_points=c["height_points"] + 0.05), r"height_points"),
                              ("nopoints", lambda c: c.pop("height_points"), r"height_points.*terrain\.actor_heights")):
        c = dict(d)
        edit(c)
        path = str(tmp_path / f"{name}.pth")
        torch.save(c, path)
        with pytest.raises(ValueError, match=match):
            Distiller(cfg=_cfg(path))
    with pytest.raises(ValueError, match=r"109"):  # the teacher's first layer against the env's row (H = 1 here: 62 columns)
        Distiller(cfg=_cfg(teacher_ck, **{"env.frame_stack": 1, "env.num_observations": 47 + P}))
    with pytest.raises(ValueError, match=r"distillation\.teacher_checkpoint"):
        Distiller(cfg=_cfg(None))


def test_two_distillers_with_one_seed_end_bit_equal(teacher_ck):
    runs = []
    for _ in range(2):
        d = _distiller(teacher_ck)
        for it in range(2):
            d.train_iteration(it)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in d.student.state_dict().items()}, d.buffer["actions"].clone(), d.buffer["teacher_mu"].clone(), d.last_loss))
        del d
    (p0, a0, m0, l0), (p1, a1, m1, l1) = runs
    assert p0.keys() == p1.keys() and all(torch.equal(p0[k], p1[k]) for k in p0)
    assert torch.equal(a0, a1) and torch.equal(m0, m1) and l0 == l1
