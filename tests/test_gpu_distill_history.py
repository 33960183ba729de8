"""distillation.student_frame_stack on the GPU: the env's third output (the student's row [47 Hs], bg_obs_assemble) against a host restatement of the
frame-stack rule and against the same env without the key (bitwise: the kernel only copies), the rollout's launch with the student on its own buffer
(bg_distill_act_hist) against its stand-alone siblings (bitwise) and float64, one Distiller iteration with Hs > H against float64 autograd + clip +
Adam, the saved student through Runner and export_model.py, and the unchanged calls with the key absent or equal to H.

Bounds are tests/test_gpu_distill.py's: the actor's mean 2e-5 max(1, |ref|max) against float64; losses 1e-4 relative and parameters rtol 1e-3 /
atol 2e-6 after three Adam steps at the learning rate 1e-5."""
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
GRID_5x3 = {"terrain.measured_points_x": [-0.2, -0.1, 0.0, 0.1, 0.2], "terrain.measured_points_y": [-0.1, 0.0, 0.1]}


# ------------------------------------------------------------------ 1. the env's rows
def _env(n, H, P, Hs=None, **over):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV, "env.frame_stack": H, "terrain.measure_heights": True,
          "terrain.actor_heights": True, "env.num_observations": 47 * H + P, "env.num_privileged_obs": 14 + P}
    if Hs is not None:
        ov["env.student_frame_stack"] = Hs
    ov.update(over)
    return T1(load_cfg("T1", ov))


@pytest.mark.parametrize("H,Hs,P,over", [(2, 5, 15, GRID_5x3), (1, 6, 187, {"sim.state_dtype": "fp16"})])
def test_student_rows_are_exact_and_the_other_outputs_are_those_without_the_key(H, Hs, P, over):
    """n = 130 is no multiple of the block's 4 envs.  Env A has the key, env B is the same config without it."""
    from test_gpu_frame_stack import HostStack, _actions

    from booster_gym_amd import _lib

    n, F, W, Ws = 130, 47 * H, 47 * H + P, 47 * Hs
    ea, eb = _env(n, H, P, Hs, **over), _env(n, H, P, **over)
    assert (ea.student_frame_stack, ea.num_student_obs, tuple(ea.student_obs_buf.shape)) == (Hs, Ws, (n, Ws)) and ea._cfg_c.student_frame_stack == Hs
    assert (eb.student_frame_stack, eb.num_student_obs, eb.student_obs_buf) == (0, 0, None) and eb._cfg_c.student_frame_stack == 0
    host = HostStack(n, Hs)
    for rep in range(2):  # (the second reset-all forgets the frame of the first)
        oa, xa = ea.reset()
        ob, xb = eb.reset()
        torch.cuda.synchronize()
        st = xa["student_obs"]
        assert st is ea.student_obs_buf and "student_obs" not in xb
        assert torch.equal(oa, ob) and torch.equal(xa["privileged_obs"], xb["privileged_obs"])
        assert torch.equal(st, host.push(oa[:, F - 47 : F])) and torch.equal(st[:, -F:], oa[:, :F]) and not st[:, :-47].any()

    def outs():
        return (torch.full((n + 7, W), float("nan"), device=DEV), torch.full((n + 7, 14 + P), float("nan"), device=DEV), torch.empty(n, device=DEV),
                torch.empty(n, dtype=torch.bool, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV))

    resets, lay, oldest_in_use, zero_again = 0, Hs + 2, False, False
    for k in range(3 * Hs + 10):
        if k == lay:  # some robots lying on their side: reset at the end of this step, in both envs alike
            assert oldest_in_use
            for e in (ea, eb):
                root = e.root_states.cpu().numpy().copy()
                root[:32, 2] -= 0.4
                root[:32, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
                e.set_field("root_states", torch.from_numpy(root).float())
        a = _actions(n, k)
        (oa, pa, ra, da, ta), (ob, pb, rb, db, tb) = outs(), outs()
        sa = torch.full((n + 7, Ws), float("nan"), device=DEV)  # a different destination at every step, as the rows of a rollout buffer
        ea.step_to(a, oa[:n], pa[:n], ra, da, ta, student_obs=sa[:n])
        eb.step_to(a, ob[:n], pb[:n], rb, db, tb)
        torch.cuda.synchronize()
        assert torch.isfinite(oa[:n]).all() and torch.isfinite(pa[:n]).all() and torch.isfinite(sa[:n]).all(), k
        assert torch.isnan(oa[n:]).all() and torch.isnan(pa[n:]).all() and torch.isnan(sa[n:]).all(), k  # nothing past row n
        assert torch.equal(oa[:n], ob[:n]) and torch.equal(pa[:n], pb[:n]) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ta, tb), k
        assert torch.equal(sa[:n], host.push(oa[:n, F - 47 : F], da)), k
        assert torch.equal(sa[:n, -F:], oa[:n, :F]), k
        if k < lay:
            oldest_in_use = oldest_in_use or bool(sa[:n, :47].abs().sum() > 0)
        if k >= lay and bool(da.any()):
            assert not sa[:n][da][:, :-47].any(), k  # a reset env: Hs - 1 zero frames and its new observation
            zero_again = True
        if k >= lay:
            resets += int(da.sum())
    assert resets >= 32 and zero_again, resets
    # a step with no student destination on A is an error, not a skipped write; the new entry points on B are errors naming the field
    (oa, pa, ra, da, ta) = outs()
    with pytest.raises(RuntimeError, match="student"):
        ea.step_to(a, oa[:n], pa[:n], ra, da, ta)
    with pytest.raises(RuntimeError, match=rf"student_obs of {n} x {Ws}"):
        ea.step_to(a, oa[:n], pa[:n], ra, da, ta, student_obs=torch.empty(n, 47, device=DEV))
    with pytest.raises(RuntimeError, match="student_frame_stack"):
        eb.step_to(a, oa[:n], pa[:n], ra, da, ta, student_obs=torch.empty(n, Ws, device=DEV))
    lib = _lib.load()
    assert lib.bg_env_bind_student_obs(eb._env, _lib.ptr(sa)) == -1 and b"student_frame_stack" in lib.bg_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(oa).all()  # (none of the refused calls launched anything)


# ------------------------------------------------------------------ 2. the rollout's launch
def _descs(model):
    from booster_gym_amd import _lib

    lin = [m for m in model.actor if isinstance(m, torch.nn.Linear)]
    return (_lib.MlpLayerDesc * len(lin))(*[_lib.MlpLayerDesc(l.weight.data_ptr(), l.bias.data_ptr(), l.in_features, l.out_features) for l in lin]), len(lin)


def _act_hist(student, teacher, tobs, sobs, P, seed, counter):
    from booster_gym_amd import _lib

    n = tobs.shape[0]
    outs = [torch.full((n + 16, A), 7.0, device=DEV) for _ in range(3)]  # student mu, actions, teacher mu
    (sd, ns), (td, nt) = _descs(student), _descs(teacher)
    _lib.check(_lib.load().bg_distill_act_hist(n, _lib.ptr(tobs), tobs.shape[1], _lib.ptr(sobs), sobs.shape[1], ns, sd, nt, td, P, _lib.ptr(student.logstd), seed,
                                               counter, *[_lib.ptr(t) for t in outs], _lib.current_stream_ptr()), "bg_distill_act_hist")
    torch.cuda.synchronize()
    for t in outs:
        assert torch.all(t[n:] == 7.0), "rows past N were written"
    return [t[:n] for t in outs]


@pytest.mark.parametrize("H,P,Hs,s_hidden,t_hidden", [(1, 187, 6, (256, 128, 128), (512, 256, 128)), (2, 15, 3, (128, 128), (256, 128, 128))])
def test_distill_act_hist_equals_its_stand_alone_launches_bitwise(H, P, Hs, s_hidden, t_hidden):
    """N = 130 is no multiple of the 16-row tile.  Case (a): the student's 282 columns pad to 288 and force the 512-wide LDS form whatever the widths;
    case (b): both tiles (109 -> 144, 141 -> 144) and all widths stay within the 256-wide form."""
    from test_gpu_frame_stack import _actor_f64

    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(200 + Hs)
    N, F, Fs, seed, counter = 130, 47 * H, 47 * Hs, 987654321, 23
    teacher = ActorCritic(A, F + P, 14 + P, t_hidden).to(DEV)
    student = ActorCritic(A, Fs, 14 + P, s_hidden).to(DEV)
    with torch.no_grad():
        student.logstd.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    tobs, sobs = torch.randn(N, F + P, device=DEV), torch.randn(N, Fs, device=DEV)  # (independent rows: nothing can come from the wrong buffer unnoticed)
    s_mu, act, t_mu = _act_hist(student, teacher, tobs, sobs, P, seed, counter)
    # the teacher: bg_actor_sample_mlp_scan on the same rows, and float64
    mu_ref, tmp = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    teacher.sample_actions(tobs, tmp, 1, 2, mu_out=mu_ref, scan=P)
    assert torch.equal(t_mu, mu_ref)
    ref = _actor_f64(teacher, tobs)
    err = (t_mu.double() - ref).abs().max().item()
    print(f"H {H} P {P} Hs {Hs}: teacher max error {err:.3e}, |ref|max {ref.abs().max().item():.3f}")
    assert err <= 2e-5 * max(1.0, ref.abs().max().item())
    # the student: bg_actor_sample_mlp on the student buffer, same seed and counter, and float64
    (sd, ns) = _descs(student)
    mu2, act2 = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp(N, _lib.ptr(sobs), ns, sd, _lib.ptr(student.logstd), seed, counter, _lib.ptr(mu2), _lib.ptr(act2),
                                               _lib.current_stream_ptr()), "bg_actor_sample_mlp")
    torch.cuda.synchronize()
    assert torch.equal(s_mu, mu2) and torch.equal(act, act2)
    sref = _actor_f64(student, sobs)
    serr = (s_mu.double() - sref).abs().max().item()
    print(f"student max error {serr:.3e}, |ref|max {sref.abs().max().item():.3f}")
    assert serr <= 2e-5 * max(1.0, sref.abs().max().item())
    assert not torch.equal(act, s_mu)  # (the noise is on)
    # the student reads its own buffer: other prefix columns in the teacher's change the teacher's outputs only
    tobs2 = tobs.clone(); tobs2[:, :F] += 1.0
    s_mu3, act3, t_mu3 = _act_hist(student, teacher, tobs2, sobs, P, seed, counter)
    assert torch.equal(s_mu3, s_mu) and torch.equal(act3, act) and not torch.equal(t_mu3, t_mu)
    # bg_distill_act is bg_distill_act_hist with the same buffer and stride on both sides
    same = ActorCritic(A, F, 14 + P, s_hidden).to(DEV)
    with torch.no_grad():
        same.logstd.copy_(student.logstd)
    (qd, nq), (td, nt) = _descs(same), _descs(teacher)
    old = [torch.full((N + 16, A), 7.0, device=DEV) for _ in range(3)]
    new = [torch.full((N + 16, A), 7.0, device=DEV) for _ in range(3)]
    lib = _lib.load()
    _lib.check(lib.bg_distill_act(N, _lib.ptr(tobs), F + P, nq, qd, nt, td, P, _lib.ptr(same.logstd), seed, counter, *[_lib.ptr(t) for t in old],
                                  _lib.current_stream_ptr()), "bg_distill_act")
    _lib.check(lib.bg_distill_act_hist(N, _lib.ptr(tobs), F + P, _lib.ptr(tobs), F + P, nq, qd, nt, td, P, _lib.ptr(same.logstd), seed, counter,
                                       *[_lib.ptr(t) for t in new], _lib.current_stream_ptr()), "bg_distill_act_hist")
    # ... and equally with the 47 H columns as a buffer of the student's own
    prefix, own = tobs[:, :F].contiguous(), [torch.full((N + 16, A), 7.0, device=DEV) for _ in range(3)]
    _lib.check(lib.bg_distill_act_hist(N, _lib.ptr(tobs), F + P, _lib.ptr(prefix), F, nq, qd, nt, td, P, _lib.ptr(same.logstd), seed, counter,
                                       *[_lib.ptr(t) for t in own], _lib.current_stream_ptr()), "bg_distill_act_hist")
    torch.cuda.synchronize()
    for o, w, x in zip(old, new, own):
        assert torch.equal(o, w) and torch.equal(o, x) and torch.all(o[N:] == 7.0)
    assert torch.equal(old[2][:N], t_mu)


def test_distill_act_hist_argument_errors():
    from booster_gym_amd import _lib

    lib, o = _lib.load(), torch.zeros(4, 600, device=DEV)
    p = o.data_ptr()
    net = lambda k_in: (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(p, p, k_in, 128), _lib.MlpLayerDesc(p, p, 128, 128), _lib.MlpLayerDesc(p, p, 128, 12))
    call = lambda ts, ss, s, t, scan: lib.bg_distill_act_hist(4, _lib.ptr(o), ts, _lib.ptr(o), ss, 3, net(s), 3, net(t), scan, _lib.ptr(o), 0, 0, None, _lib.ptr(o),
                                                              _lib.ptr(o), None)
    assert call(235, 235, 235, 234, 187) == -4 and b"teacher" in lib.bg_last_error()   # teacher_stride is not the teacher's `in`
    assert call(234, 236, 235, 234, 187) == -4 and b"student" in lib.bg_last_error()   # student_stride is not the student's `in`
    assert call(234, 240, 240, 234, 187) == -4 and b"student" in lib.bg_last_error()   # a student `in` that is not 47 Hs
    assert call(234, 517, 517, 234, 187) == -4 and b"student" in lib.bg_last_error()   # ... or Hs = 11
    assert call(109, 47, 47, 109, 15) == -4 and b"student" in lib.bg_last_error()      # 47 Hs below the teacher's 47 H
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. - 5. the Distiller
H, HS, P, N, T = 2, 4, 15, 64, 4


def _cfg(teacher=None, Hs=HS, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "env.frame_stack": H,
          "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 * H + P, "env.num_privileged_obs": 14 + P,
          "distillation.num_epochs": 3, "distillation.learning_rate": 1.0e-5, "distillation.teacher_checkpoint": teacher,
          "distillation.student_frame_stack": Hs, **GRID_5x3}
    ov.update(over)
    return load_cfg("T1", ov)


@pytest.fixture(scope="module")
def teacher_ck(tmp_path_factory):
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.terrain import height_scan_points

    torch.manual_seed(5)
    m = ActorCritic(A, 47 * H + P, 14 + P)
    pts = torch.tensor(height_scan_points(_cfg()["terrain"])[1], dtype=torch.float).reshape(P, 2)
    path = str(tmp_path_factory.mktemp("teacher") / "teacher.pth")
    torch.save({"model": m.state_dict(), "height_points": pts}, path)
    return path


class _Rec:
    def __init__(self):
        self.stats, self.saved = {}, []

    def record_episode_statistics(self, env, names, it, stats=None):
        env.episode_stats(reset=True)

    def record_statistics(self, summary, it):
        self.stats[it] = dict(summary)

    def save(self, d, it):
        self.saved.append(it)


def _distiller(teacher, Hs=HS, **over):
    from booster_gym_amd.utils.distill import Distiller

    d = Distiller(cfg=_cfg(teacher, Hs, **over))
    d.begin(recorder=_Rec())
    return d


def test_one_iteration_with_a_longer_history_matches_the_float64_restatement(teacher_ck):
    """H = 2, Hs = 4: the student's 188 columns are padded to 256; B = 256 rows."""
    from booster_gym_amd.utils.model import ActorCritic

    d = _distiller(teacher_ck)
    F, Fs = 47 * H, 47 * HS
    assert d.history and (d.student_obs, d.scan, d.env.num_obs, d.env.student_frame_stack) == (Fs, P, F + P, HS)
    assert d.student.actor[0].in_features == Fs and d.student.critic[0].in_features == Fs + 14 + P and d._student_in.shape == (T * N, 256)
    assert all(d._sup.mlp.plan.grouped[:-1]) and "library" not in (d._sup.mlp.plan.fwd, d._sup.mlp.plan.bwd)
    assert abs(d.student.logstd[0, 0].item() - math.log(0.1)) < 1e-7
    sob = d.buffer["student_obses"]
    assert tuple(sob.shape) == (T + 1, N, Fs) and torch.equal(sob[0, :, -F:], d.buffer["obses"][0, :, :F]) and not sob[0, :, :-47].any()
    frozen = lambda: {**{"student." + k: v.clone() for k, v in d.student.state_dict().items() if not k.startswith("actor.")},
                      **{"teacher." + k: v.clone() for k, v in d.teacher.state_dict().items()}}
    before, c0 = frozen(), d._act_counter
    d.rollout()
    torch.cuda.synchronize()
    assert d._act_counter == c0 + T
    obses, labels = d.buffer["obses"], d.buffer["teacher_mu"]
    mu, tmp = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    for t in range(T):
        d.teacher.sample_actions(obses[t], tmp, 0, 0, mu_out=mu, scan=P)  # bg_actor_sample_mlp_scan
        assert torch.equal(labels[t], mu), t
        assert torch.equal(sob[t + 1, :, -F:], obses[t + 1, :, :F]), t  # the student's newest H frames are the teacher's
        keep = ~d.buffer["dones"][t]
        assert torch.equal(sob[t + 1, keep, : Fs - 47], sob[t, keep, 47:]), t  # ... and its older ones the previous row's, shifted by a frame
    assert sob[T, :, :47].abs().sum() > 0  # (the reset's frame and T = 4 steps' make 5 >= Hs: the oldest frame is in use)
    # the actions came from the student's own buffer: bg_actor_sample_mlp on student_obses[0], the rollout's seed and first counter
    from booster_gym_amd import _lib
    (sd, ns) = _descs(d.student)
    act0 = torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp(N, _lib.ptr(sob[0]), ns, sd, _lib.ptr(d.student.logstd), int(d.cfg["basic"]["seed"]) + 1000003, c0, None,
                                               _lib.ptr(act0), _lib.current_stream_ptr()), "bg_actor_sample_mlp")
    torch.cuda.synchronize()
    assert torch.equal(act0, d.buffer["actions"][0])
    # the restatement: float64 autograd + clip_grad_norm_ + torch.optim.Adam on student_obses[:T] and the labels
    B = T * N
    rows, y = sob[:T].reshape(B, Fs).double(), labels.reshape(B, A).double()
    ref = ActorCritic(A, Fs, 14 + P, d.dcfg.student_hidden).to(DEV)
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


def test_two_distillers_with_a_longer_history_and_one_seed_end_bit_equal(teacher_ck):
    runs = []
    for _ in range(2):
        d = _distiller(teacher_ck)
        for it in range(2):
            d.train_iteration(it)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in d.student.state_dict().items()}, d.buffer["actions"].clone(), d.buffer["teacher_mu"].clone(),
                     d.buffer["student_obses"].clone(), d.last_loss))
        del d
    (p0, a0, m0, s0, l0), (p1, a1, m1, s1, l1) = runs
    assert p0.keys() == p1.keys() and all(torch.equal(p0[k], p1[k]) for k in p0)
    assert torch.equal(a0, a1) and torch.equal(m0, m1) and torch.equal(s0, s1) and l0 == l1


def test_student_with_a_longer_history_re_enters_runner_and_export(teacher_ck, tmp_path):
    from booster_gym_amd.utils.distill import student_cfg_overrides
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.runner import Runner

    d = _distiller(teacher_ck, **{"runner.save_interval": 1})
    d.train_iteration(0)
    assert d.recorder.saved == [1] and np.isfinite(d.recorder.stats[0]["distill/behaviour_loss"])
    ck = d.checkpoint_dict()
    assert set(ck) == {"model", "curriculum", "distillation"} and ck["distillation"]["student_frame_stack"] == HS
    path = str(tmp_path / "student.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in d.student.state_dict().items()}
    over = student_cfg_overrides(d.cfg)
    assert over == {"terrain.actor_heights": False, "env.frame_stack": HS, "env.num_observations": 47 * HS}
    del d
    r = Runner(test=True, cfg=_cfg(**over, **{"basic.checkpoint": path}))
    assert r.env.frame_stack == HS and r.env.student_frame_stack == 0 and r.model.actor[0].in_features == 47 * HS
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert r.play(max_steps=1) == 1
    del r
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={path}"], cwd=str(tmp_path), env=env, check=True, timeout=300,
                   capture_output=True, text=True)
    actor = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    m = ActorCritic(A, 47 * HS, 14 + P)
    m.load_state_dict({k: v.cpu() for k, v in sd.items()})
    x = torch.linspace(-1, 1, 47 * HS).reshape(1, 47 * HS)
    y = actor(x)
    assert tuple(y.shape) == (1, A) and torch.allclose(y, m.actor(x), atol=1e-6)


@pytest.mark.parametrize("Hs", [None, H])
def test_key_absent_or_equal_to_the_teachers_keeps_todays_calls(monkeypatch, teacher_ck, Hs):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.distill import student_cfg_overrides

    cfg = _cfg(teacher_ck, Hs)
    if Hs is None:
        del cfg["distillation"]["student_frame_stack"]  # the key absent, as in a yaml written before it existed
    from booster_gym_amd.utils.distill import Distiller

    d = Distiller(cfg=cfg)
    d.begin(recorder=_Rec())
    assert not d.history and "student_obses" not in d.buffer._streams and d.env.student_frame_stack == 0 and d.env._cfg_c.student_frame_stack == 0
    assert "student_frame_stack" not in d.cfg["env"] and d.student_obs == 47 * H and d.student.actor[0].in_features == 47 * H
    lib, counts = _lib.load(), {"bg_distill_act": 0, "bg_distill_act_hist": 0, "bg_env_step_to": 0, "bg_env_step_to_student": 0}
    for name in counts:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    d.train_iteration(0)
    torch.cuda.synchronize()
    assert counts == {"bg_distill_act": T, "bg_distill_act_hist": 0, "bg_env_step_to": T, "bg_env_step_to_student": 0}
    assert "student_frame_stack" not in d.checkpoint_dict()["distillation"]
    assert student_cfg_overrides(d.cfg) == {"terrain.actor_heights": False, "env.num_observations": 47 * H}
