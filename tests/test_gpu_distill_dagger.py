"""distillation.teacher_action_prob on the GPU (DAgger's mixing): the rollout's third two-network launch, bg_distill_act_mix, against bg_distill_act /
bg_distill_act_hist (beta = 0, bitwise), against the teacher's stand-alone launch under the student's logstd (beta = 1, bitwise), and row by row
against the host's restatement of the choice u < beta (oracle/task_ref.py's generator on stream 29); then the Distiller: the schedule of beta, what
is logged and saved, the keys off against the keys absent (no new entry point runs), reproducibility with both new keys on, and the checkpoint's way
back into Runner.

Every comparison of outputs is bitwise; the one statistical bound is the issue's: the teacher's share of 4,096 rows at beta = 0.5 within 5 sigma of
Binomial(4096, 0.5), 2048 +- 160."""
import numpy as np
import pytest
import torch

from test_gpu_distill import _Rec, _cfg, _descs, _save_teacher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 12
RS_DAGGER = 29  # booster_gym_amd/csrc/bg_rng.h
SEED, COUNTER = 987654321, 23
NEW_ENTRY_POINTS = ("bg_distill_act_mix", "bg_distill_head_sym", "bg_distill_head_sym_partial")


# ------------------------------------------------------------------ 1. the launch
def _nets(case):
    """(student, teacher, teacher rows, student rows or None, P): (a) H = 1 / P = 187, both 256-128-128 on one buffer; (b) H = 1 / P = 45 with Hs = 3 on a
    student buffer of its own; (c) a 512-wide student (the 512-wide LDS form for both halves)."""
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed({"a": 1, "b": 2, "c": 3}[case])
    P, Hs, s_hidden = {"a": (187, 1, (256, 128, 128)), "b": (45, 3, (256, 128, 128)), "c": (187, 1, (512, 256, 128))}[case]
    teacher = ActorCritic(A, 47 + P, 14 + P).to(DEV)
    student = ActorCritic(A, 47 * Hs, 14 + P, s_hidden).to(DEV)
    with torch.no_grad():
        student.logstd.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    return student, teacher, P, Hs


def _rows(N, P, Hs, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    tobs = torch.randn(N, 47 + P, generator=g).to(DEV)
    if Hs == 1:
        return tobs, tobs
    sobs = torch.randn(N, 47 * Hs, generator=g).to(DEV)
    sobs[:, -47:] = tobs[:, :47]
    return tobs, sobs


def _launch(name, student, teacher, tobs, sobs, P, counter, N, beta=None, noise=1):
    """student mu, actions, teacher mu ([N] rows each, the 16 sentinel rows behind them checked) of one of the three launches."""
    from booster_gym_amd import _lib

    outs = [torch.full((N + 16, A), 7.0, device=DEV) for _ in range(3)]
    (sd, ns), (td, nt) = _descs(student), _descs(teacher)
    p, lib = _lib.ptr, _lib.load()
    tail = [p(student.logstd), SEED, counter] + ([] if beta is None else [beta, noise]) + [p(t) for t in outs] + [_lib.current_stream_ptr()]
    if name == "bg_distill_act":
        rc = lib.bg_distill_act(N, p(tobs), tobs.shape[1], ns, sd, nt, td, P, *tail)
    else:
        rc = getattr(lib, name)(N, p(tobs), tobs.shape[1], p(sobs), sobs.shape[1], ns, sd, nt, td, P, *tail)
    _lib.check(rc, name)
    torch.cuda.synchronize()
    for t in outs:
        assert torch.all(t[N:] == 7.0), "rows past N were written"
    return [t[:N] for t in outs]


def _choice(N, counter, beta, seed=SEED):
    """The host's restatement of who acts: u < beta in fp32, u = entry 0 of rand4(seed, row, counter, 29)."""
    from oracle.task_ref import rand4

    u, _ = rand4(seed, np.arange(N), counter, RS_DAGGER)
    assert u.dtype == np.float32
    return torch.from_numpy(u[:, 0] < np.float32(beta)).to(DEV)


@pytest.mark.parametrize("N", [272, 5])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_mix_launch_is_its_siblings_row_by_row(case, N):
    """N = 272: 17 workgroups of 16 rows per half (no power of two); N = 5: a ragged last workgroup."""
    from booster_gym_amd import _lib

    student, teacher, P, Hs = _nets(case)
    tobs, sobs = _rows(N, P, Hs)
    base = _launch("bg_distill_act" if Hs == 1 else "bg_distill_act_hist", student, teacher, tobs, sobs, P, COUNTER, N)
    mix = lambda beta, noise=1, counter=COUNTER: _launch("bg_distill_act_mix", student, teacher, tobs, sobs, P, counter, N, beta, noise)
    # beta = 0: the student always acts
    zero = mix(0.0)
    for x, y, what in zip(zero, base, ("student_mu", "actions", "teacher_mu")):
        assert torch.equal(x, y), ("beta = 0", what)
    assert torch.equal(mix(0.0, 0)[1], base[1])  # (teacher_noise is the teacher's business)
    # beta = 1: the teacher always acts, with the student's logstd and the student's draw
    one, (td, nt) = mix(1.0), _descs(teacher)
    mu_t, act_t = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp_scan(N, _lib.ptr(tobs), nt, td, P, _lib.ptr(student.logstd), SEED, COUNTER, _lib.ptr(mu_t), _lib.ptr(act_t),
                                                    _lib.current_stream_ptr()), "bg_actor_sample_mlp_scan")
    torch.cuda.synchronize()
    assert torch.equal(one[1], act_t) and torch.equal(one[2], mu_t) and not torch.equal(act_t, mu_t)
    assert torch.equal(one[0], zero[0]) and torch.equal(one[2], zero[2])
    quiet = mix(1.0, 0)
    assert torch.equal(quiet[1], quiet[2]) and torch.equal(quiet[0], zero[0]) and torch.equal(quiet[2], zero[2])
    # beta = 0.5: every row is one of the two, and which one is u < 0.5
    half, teacher_acts = mix(0.5), _choice(N, COUNTER, 0.5)
    assert torch.equal(half[0], zero[0]) and torch.equal(half[2], zero[2])
    from_teacher, from_student = (half[1] == one[1]).all(1), (half[1] == zero[1]).all(1)
    assert not ((one[1] == zero[1]).all(1)).any()  # (no row on which the two candidates coincide: the choice can be read off the output)
    assert torch.all(from_teacher | from_student) and torch.equal(from_teacher, teacher_acts), (from_teacher.sum().item(), teacher_acts.sum().item())
    quiet_half = mix(0.5, 0)[1]
    assert torch.equal(quiet_half[teacher_acts], zero[2][teacher_acts]) and torch.equal(quiet_half[~teacher_acts], zero[1][~teacher_acts])
    other = _choice(N, COUNTER + 1, 0.5)
    got = (mix(0.5, 1, COUNTER + 1)[1] == mix(1.0, 1, COUNTER + 1)[1]).all(1)
    assert torch.equal(got, other)
    if N == 272:
        assert 0 < int(teacher_acts.sum()) < N and not torch.equal(other, teacher_acts)  # another counter, another choice vector


def test_teachers_share_of_4096_rows_is_binomial():
    student, teacher, P, Hs = _nets("a")
    N = 4096
    tobs, sobs = _rows(N, P, Hs)
    half = _launch("bg_distill_act_mix", student, teacher, tobs, sobs, P, COUNTER, N, 0.5, 0)
    share = int((half[1] == half[2]).all(1).sum())  # (teacher_noise = 0: a teacher-driven row is the teacher's mean)
    print(f"teacher-driven rows of {N} at beta = 0.5: {share}")
    assert share == int(_choice(N, COUNTER, 0.5).sum()) and abs(share - 2048) <= 160
    quarter = _launch("bg_distill_act_mix", student, teacher, tobs, sobs, P, COUNTER, N, 0.25, 0)
    assert int((quarter[1] == quarter[2]).all(1).sum()) == int(_choice(N, COUNTER, 0.25).sum())


def test_mix_launch_argument_errors_name_the_entry_point():
    from booster_gym_amd import _lib

    lib, o = _lib.load(), torch.zeros(4, 600, device=DEV)
    p = o.data_ptr()
    net = lambda k_in: (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(p, p, k_in, 128), _lib.MlpLayerDesc(p, p, 128, 128), _lib.MlpLayerDesc(p, p, 128, 12))
    call = lambda ts, ss, s, t, scan, beta=0.5: lib.bg_distill_act_mix(4, _lib.ptr(o), ts, _lib.ptr(o), ss, 3, net(s), 3, net(t), scan, _lib.ptr(o), 0, 0, beta, 1, None,
                                                                       _lib.ptr(o), _lib.ptr(o), None)
    for args, word in (((235, 235, 235, 234, 187), b"teacher"), ((234, 236, 235, 234, 187), b"student"), ((234, 240, 240, 234, 187), b"student"),
                       ((109, 47, 47, 109, 15), b"student")):
        assert call(*args) == -4 and word in lib.bg_last_error() and b"bg_distill_act_mix" in lib.bg_last_error(), (args, lib.bg_last_error())
    for beta in (1.5, -0.5, float("nan")):
        assert call(234, 234, 47, 234, 187, beta) == -1 and b"bg_distill_act_mix" in lib.bg_last_error() and b"beta" in lib.bg_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the Distiller (128 envs, T = 24)
BIG = {"env.num_envs": 128, "runner.horizon_length": 24}
H = 2


@pytest.fixture(scope="module")
def teacher_ck(tmp_path_factory):
    return _save_teacher(str(tmp_path_factory.mktemp("teacher") / "teacher.pth"))


def _distiller(teacher, frames=H, **over):
    from booster_gym_amd.utils.distill import Distiller

    d = Distiller(cfg=_cfg(teacher, frames, **BIG, **over))
    d.begin(recorder=_Rec())
    return d


def _count(monkeypatch, lib, names, record=None):
    counts = dict.fromkeys(names, 0)
    for name in names:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            if record is not None:
                record.append((_name, a))
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


def test_beta_follows_its_schedule_and_is_logged(monkeypatch, teacher_ck):
    from booster_gym_amd import _lib

    d = _distiller(teacher_ck, **{"distillation.teacher_action_prob": 1.0, "distillation.teacher_action_iterations": 2})
    lib, calls = _lib.load(), []
    counts = _count(monkeypatch, lib, ("bg_distill_act_mix", "bg_distill_act", "bg_distill_act_hist", "bg_distill_head_partial", "bg_distill_head_sym_partial"), calls)
    T, N, P = d.T, d.N, d.scan
    obs0, c0 = d.buffer["obses"][0].clone(), d._act_counter
    for it in range(3):
        d.train_iteration(it)
    torch.cuda.synchronize()
    assert counts == {"bg_distill_act_mix": 3 * T, "bg_distill_act": 0, "bg_distill_act_hist": 0, "bg_distill_head_partial": 3 * d.dcfg.num_epochs,
                      "bg_distill_head_sym_partial": 0}
    betas = [a[13] for name, a in calls if name == "bg_distill_act_mix"]
    assert betas == [1.0] * T + [0.5] * T + [0.0] * T and all(a[14] == 1 for name, a in calls if name == "bg_distill_act_mix")
    assert [d.recorder.stats[it]["distill/teacher_action_prob"] for it in range(3)] == [1.0, 0.5, 0.0]
    assert all(set(d.recorder.stats[it]) == {"distill/behaviour_loss", "distill/teacher_action_prob"} for it in range(3))
    entry = d.checkpoint_dict()["distillation"]
    assert entry["teacher_action_prob"] == [1.0, 2] and "symmetric_coef" not in entry
    # iteration 0 was the teacher's: its first actions are the teacher's sample on the first rows, under the student's logstd
    d2 = _distiller(teacher_ck, **{"distillation.teacher_action_prob": 1.0, "distillation.teacher_action_iterations": 2})
    assert torch.equal(d2.buffer["obses"][0], obs0)
    d2.rollout()
    (td, nt), act = _descs(d2.teacher), torch.empty(N, A, device=DEV)
    _lib.check(lib.bg_actor_sample_mlp_scan(N, _lib.ptr(obs0), nt, td, P, _lib.ptr(d2.student.logstd), int(d2.cfg["basic"]["seed"]) + 1000003, c0, None, _lib.ptr(act),
                                            _lib.current_stream_ptr()), "bg_actor_sample_mlp_scan")
    torch.cuda.synchronize()
    assert torch.equal(d2.buffer["actions"][0], act)


def _state(d):
    return ({k: v.clone() for k, v in d.student.state_dict().items()}, {k: d.buffer[k].clone() for k in ("actions", "teacher_mu", "obses", "rewards", "dones")},
            d.last_loss)


def test_keys_absent_or_at_their_defaults_run_todays_calls_alone(monkeypatch, teacher_ck):
    """Two iterations with the four keys absent and with them at their defaults: the same bits, the launches of a Distiller without the keys (T x
    bg_distill_act and num_epochs x bg_distill_head_partial per iteration), today's log names and checkpoint keys; the new entry points raise if touched."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.distill import DEFAULTS, Distiller

    lib = _lib.load()

    def forbidden(*a):
        raise AssertionError("a new entry point ran with the keys off")

    for name in NEW_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, forbidden)
    counts = _count(monkeypatch, lib, ("bg_distill_act", "bg_distill_act_hist", "bg_distill_head_partial", "bg_env_step_to", "bg_mirror_rows"))
    runs = []
    for absent in (True, False):
        cfg = _cfg(teacher_ck, H, **BIG)
        keys = ("symmetric_coef", "teacher_action_prob", "teacher_action_iterations", "teacher_action_noise")
        assert all(cfg["distillation"][k] == DEFAULTS[k] for k in keys)
        if absent:
            for k in keys:
                del cfg["distillation"][k]
        d = Distiller(cfg=cfg)
        d.begin(recorder=_Rec())
        assert not d.symmetry and d.beta0 == 0 and d._student_in.shape[0] == d.B and d._sup.stats.numel() == 1
        for it in range(2):
            d.train_iteration(it)
        torch.cuda.synchronize()
        assert all(set(d.recorder.stats[it]) == {"distill/behaviour_loss"} for it in range(2))
        ck = d.checkpoint_dict()
        assert set(ck) == {"model", "curriculum", "distillation"} and set(ck["distillation"]) == {"teacher", "iteration", "loss"}
        runs.append(_state(d))
        T, E = d.T, d.dcfg.num_epochs
        del d
    assert counts == {"bg_distill_act": 4 * T, "bg_distill_act_hist": 0, "bg_distill_head_partial": 4 * E, "bg_env_step_to": 4 * T, "bg_mirror_rows": 0}
    (p0, b0, l0), (p1, b1, l1) = runs
    assert all(torch.equal(p0[k], p1[k]) for k in p0) and all(torch.equal(b0[k], b1[k]) for k in b0) and l0 == l1


def test_two_runs_with_both_keys_on_end_bit_equal_and_the_student_re_enters_runner(teacher_ck, tmp_path):
    """symmetric_coef = 10, beta_0 = 0.5 over 4 iterations, and a student history of 3 frames above the teacher's 2: the three additions together."""
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides
    from booster_gym_amd.utils.runner import Runner

    over = {"distillation.symmetric_coef": 10.0, "distillation.teacher_action_prob": 0.5, "distillation.teacher_action_iterations": 4,
            "distillation.student_frame_stack": 3}
    runs = []
    for _ in range(2):
        d = _distiller(teacher_ck, **over)
        assert d.symmetry and d.history and d._student_in.shape == (2 * d.B, 256)
        for it in range(2):
            d.train_iteration(it)
        torch.cuda.synchronize()
        runs.append(_state(d) + (d.last_symmetry_loss, d.buffer["student_obses"].clone()))
        stats, ck, cfg = d.recorder.stats, d.checkpoint_dict(), d.cfg
        del d
    (p0, b0, l0, s0, o0), (p1, b1, l1, s1, o1) = runs
    assert all(torch.equal(p0[k], p1[k]) for k in p0) and all(torch.equal(b0[k], b1[k]) for k in b0) and l0 == l1 and s0 == s1 and torch.equal(o0, o1)
    assert [stats[it]["distill/teacher_action_prob"] for it in range(2)] == [0.5, 0.375]
    assert set(stats[1]) == {"distill/behaviour_loss", "distill/symmetry_loss", "distill/teacher_action_prob"}
    assert np.isfinite(l0) and np.isfinite(s0) and s0 > 0 and stats[1]["distill/symmetry_loss"] == s0
    assert ck["distillation"]["symmetric_coef"] == 10.0 and ck["distillation"]["teacher_action_prob"] == [0.5, 4] and ck["distillation"]["student_frame_stack"] == 3
    path = str(tmp_path / "student.pth")
    torch.save(ck, path)
    ov = student_cfg_overrides(cfg)
    assert ov == {"terrain.actor_heights": False, "env.frame_stack": 3, "env.num_observations": 141}
    assert checkpoint_student_overrides(torch.load(path, map_location="cpu", weights_only=True)) == ov
    r = Runner(test=True, cfg=_cfg(**BIG, **ov, **{"basic.checkpoint": path}))
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, p0[k]), k
    assert r.play(max_steps=2) == 2
