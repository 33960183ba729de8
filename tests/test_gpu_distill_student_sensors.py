"""distillation.student_sensors through the Distiller: the key absent against null (the same launches in the same order, the same bits), an empty
section at Hs = H against the key absent (bit-equal through bg_distill_act_hist, and through bg_distill_act_gru_own with a recurrent student), a
full section (finite, other bits, labels from the teacher's clean row; with DAgger's mixing, the symmetry loss and a longer history), the new
entry point of the recurrent student alone against bg_distill_act_gru, and the checkpoint's round trip into Runner(test=True) and evaluate.py.

Shapes: 128 envs, horizon_length 8, num_epochs 2, two iterations, a seeded untrained teacher with H = 1 and a scan of 3 x 2 points."""
import hashlib

import numpy as np
import pytest
import torch

from test_gpu_distill_history import _Rec, _descs
from test_sensors import FULL_BIAS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, P, N, T, ITERS = 12, 6, 128, 8, 2
GRID = {"terrain.measured_points_x": [-0.2, 0.0, 0.2], "terrain.measured_points_y": [-0.1, 0.1]}
FULL = {"bias": FULL_BIAS, "latency_steps": [0.0, 1.5]}
ABSENT = "absent"


def _cfg(teacher=None, sensors=ABSENT, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "basic.sim_device": DEV, "basic.rl_device": DEV, "runner.horizon_length": T, "terrain.measure_heights": True,
          "terrain.actor_heights": True, "env.num_observations": 47 + P, "env.num_privileged_obs": 14 + P, "distillation.num_epochs": 2,
          "distillation.teacher_checkpoint": teacher, **GRID}
    ov.update(over)
    cfg = load_cfg("T1", ov)
    if isinstance(sensors, str) and sensors == ABSENT:
        del cfg["distillation"]["student_sensors"]  # the key absent, as in a yaml written before it existed
    else:
        cfg["distillation"]["student_sensors"] = sensors
    return cfg


@pytest.fixture(scope="module")
def teacher_ck(tmp_path_factory):
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.terrain import height_scan_points

    torch.manual_seed(5)
    m = ActorCritic(A, 47 + P, 14 + P)
    pts = torch.tensor(height_scan_points(_cfg()["terrain"])[1], dtype=torch.float).reshape(P, 2)
    path = str(tmp_path_factory.mktemp("teacher") / "teacher.pth")
    torch.save({"model": m.state_dict(), "height_points": pts}, path)
    return path


def _sha(d):
    """SHA-256 over the student's parameters and Adam moments (and a recurrent student's rollout state)."""
    o, h = d.optimizer, hashlib.sha256()
    for t in list(d.student.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq] + ([d.state] if d.memory else []):
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


_DONE = {}


def _train(teacher, sensors, spy=None, keep=False, **over):
    """Two iterations; (sha, losses, launch names in order when spied, the Distiller when kept).  Runs without a spy are shared by the tests."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.distill import Distiller

    key = (repr(sensors), tuple(sorted(over.items())))
    if spy is None and not keep and key in _DONE:
        return _DONE[key]
    names, lib = [], _lib.load()
    if spy is not None:
        for name in _lib.SYMBOLS:
            if name in ("bg_last_error", "bg_version"):
                continue

            def wrap(*a, _fn=getattr(lib, name), _name=name):
                names.append(_name)
                return _fn(*a)

            spy.setattr(lib, name, wrap)
    d = Distiller(cfg=_cfg(teacher, sensors, **over))
    d.begin(recorder=_Rec())
    losses = []
    for it in range(ITERS):
        d.train_iteration(it)
        losses.append(d.last_loss)
    torch.cuda.synchronize()
    out = (_sha(d), losses, names, d if keep else None)
    if spy is not None:
        spy.undo()
    elif not keep:
        _DONE[key] = out
    return out


# ------------------------------------------------------------------ 1. the key absent against null
@pytest.mark.parametrize("over", [{}, {"distillation.student_frame_stack": 3}], ids=["Hs=H", "Hs=3"])
def test_absent_and_null_run_the_same_launches_and_end_bit_equal(monkeypatch, teacher_ck, over):
    sha_a, loss_a, names_a, _ = _train(teacher_ck, ABSENT, spy=monkeypatch, **over)
    sha_n, loss_n, names_n, _ = _train(teacher_ck, None, spy=monkeypatch, **over)
    act = "bg_distill_act_hist" if over else "bg_distill_act"
    assert names_a.count(act) == ITERS * T and names_a.count("bg_distill_act_gru_own") == 0 and len(names_a) > ITERS * (2 * T + 2)
    assert names_a == names_n and sha_a == sha_n and loss_a == loss_n and np.isfinite(loss_a).all()
    assert _train(teacher_ck, ABSENT, **over)[0] == sha_a  # (the spy changes nothing)


# ------------------------------------------------------------------ 2. an empty section at Hs = H
def test_an_empty_section_is_the_key_absent_through_the_students_own_row(monkeypatch, teacher_ck):
    sha_a, loss_a = _train(teacher_ck, ABSENT)[:2]
    sha_e, loss_e, names, _ = _train(teacher_ck, {}, spy=monkeypatch)
    assert names.count("bg_distill_act_hist") == ITERS * T and names.count("bg_distill_act") == 0
    assert names.count("bg_env_step_to_student") == ITERS * T and names.count("bg_env_step_to") == 0
    assert sha_e == sha_a and loss_e == loss_a


def test_an_empty_section_is_the_key_absent_for_a_recurrent_student(monkeypatch, teacher_ck):
    mem = {"distillation.student_memory": 128}
    sha_a, loss_a, names_a, _ = _train(teacher_ck, ABSENT, spy=monkeypatch, **mem)
    sha_e, loss_e, names_e, _ = _train(teacher_ck, {}, spy=monkeypatch, **mem)
    assert names_a.count("bg_distill_act_gru") == ITERS * T and names_a.count("bg_distill_act_gru_own") == 0
    assert names_e.count("bg_distill_act_gru_own") == ITERS * T and names_e.count("bg_distill_act_gru") == 0
    assert sha_e == sha_a and loss_e == loss_a and np.isfinite(loss_a).all()


# ------------------------------------------------------------------ 3. a full section
def test_a_full_section_trains_on_other_rows_and_the_labels_are_the_clean_teachers(teacher_ck):
    sha_a = _train(teacher_ck, ABSENT)[0]
    sha, losses, _, d = _train(teacher_ck, FULL, keep=True)
    assert np.isfinite(losses).all() and all(l > 0 for l in losses) and sha != sha_a
    assert d.history and d.env.student_sensor_model and not d.env.sensor_model and d.env.sensor_launches == 0 and d.env._cfg_c.sensor_model == 2
    assert d.cfg["env"]["student_frame_stack"] == 1 and d.cfg["env"]["student_sensors"] == d.student_sensors
    obses, sob, labels = d.buffer["obses"], d.buffer["student_obses"], d.buffer["teacher_mu"]
    assert tuple(sob.shape) == (T + 1, N, 47) and not torch.equal(sob[:T], obses[:T, :, :47])
    mu, tmp = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    for t in range(1, T):  # the labels come from the clean row: the teacher's mean on its own stored rows (bg_actor_sample_mlp_scan; row 0 has been rolled)
        d.teacher.sample_actions(obses[t], tmp, 0, 0, mu_out=mu, scan=P)
        assert torch.equal(labels[t], mu), t
    # the update regressed on the student's rows
    assert torch.equal(d._student_in[N : T * N, :47], sob[1:T].reshape((T - 1) * N, 47))  # (row 0 has been rolled: the next iteration's first)
    assert _train(teacher_ck, FULL)[0] == sha  # deterministic


@pytest.mark.parametrize("over", [{"distillation.teacher_action_prob": 0.5}, {"distillation.symmetric_coef": 1.0}, {"distillation.student_frame_stack": 3},
                                  {"distillation.student_memory": 128}], ids=["dagger", "symmetry", "Hs=3", "memory"])
def test_a_full_section_composes_with_the_other_keys(teacher_ck, over):
    sha, losses, _, d = _train(teacher_ck, FULL, keep=True, **over)
    assert np.isfinite(losses).all() and torch.isfinite(d.optimizer.flat).all()
    assert d.history and tuple(d.buffer["student_obses"].shape) == (T + 1, N, 47 * over.get("distillation.student_frame_stack", 1))
    assert sha != _train(teacher_ck, ABSENT, **over)[0]
    del d
    assert _train(teacher_ck, FULL, **over)[0] == sha  # deterministic


# ------------------------------------------------------------------ 4. the new entry point alone
@pytest.mark.parametrize("n", [37, 16])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_distill_act_gru_own_on_the_teachers_columns_equals_distill_act_gru(n, beta):
    from test_gpu_distill_memory import _distill_gru, _inputs, _student

    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    H = 128
    student = _student(H, P=P)
    torch.manual_seed(9)
    teacher = ActorCritic(A, 47 + P, 14 + P).to(DEV)
    tobs, h_in, reset = _inputs(n, H, width=47 + P)
    want = _distill_gru(student, teacher, tobs, P, reset, h_in, n, beta)  # h_out, student mu, actions, teacher mu

    def own(sobs):
        h_out = torch.full((n + 16, H), 7.0, device=DEV)
        outs = [torch.full((n + 16, A), 7.0, device=DEV) for _ in range(3)]
        (sd, ns), (td, nt), p = _descs(student), _descs(teacher), _lib.ptr
        from test_gpu_distill_memory import COUNTER, SEED

        _lib.check(_lib.load().bg_distill_act_gru_own(n, p(tobs), tobs.shape[1], p(sobs), sobs.shape[1], nt, td, P, student.gru_descriptor(), ns, sd, p(student.logstd),
                                                      SEED, COUNTER, beta, 1, p(reset), p(h_in), p(h_out), *[p(t) for t in outs], _lib.current_stream_ptr()),
                   "bg_distill_act_gru_own")
        torch.cuda.synchronize()
        for t in outs + [h_out]:
            assert torch.all(t[n:] == 7.0), "rows past N were written"
        return [h_out[:n]] + [t[:n] for t in outs]

    copy = tobs[:, :47].contiguous()
    for x, y, what in zip(own(copy), want, ("h_out", "student_mu", "actions", "teacher_mu")):
        assert torch.equal(x, y), what
    wide = torch.cat([copy, torch.full((n, 9), float("nan"), device=DEV)], dim=1)  # a stride above 47: the cell reads the first 47 columns alone
    for x, y, what in zip(own(wide), want, ("h_out", "student_mu", "actions", "teacher_mu")):
        assert torch.equal(x, y), what
    other = own(copy + 1.0)  # the cell reads the student's rows: other rows move the student's half and leave the teacher's
    assert torch.equal(other[3], want[3]) and not torch.equal(other[0], want[0]) and not torch.equal(other[1], want[1])
    lib, p = _lib.load(), _lib.ptr
    (sd, ns), (td, nt) = _descs(student), _descs(teacher)
    rc = lib.bg_distill_act_gru_own(n, p(tobs), tobs.shape[1], p(copy), 46, nt, td, P, student.gru_descriptor(), ns, sd, p(student.logstd), 0, 0, beta, 1, None, p(h_in),
                                    p(h_in), None, p(want[2]), p(want[3]), None)
    assert rc == -1 and b"bg_distill_act_gru_own" in lib.bg_last_error() and b"student_stride" in lib.bg_last_error()
    rc = lib.bg_distill_act_gru_own(n, p(tobs), tobs.shape[1], None, 47, nt, td, P, student.gru_descriptor(), ns, sd, p(student.logstd), 0, 0, beta, 1, None, p(h_in),
                                    p(h_in), None, p(want[2]), p(want[3]), None)
    assert rc == -1 and b"bg_distill_act_gru_own" in lib.bg_last_error()


# ------------------------------------------------------------------ 5. the checkpoint's round trip
def test_the_checkpoint_carries_the_section_and_the_student_re_enters_under_it(teacher_ck, tmp_path):
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides
    from booster_gym_amd.utils.evaluate import Evaluator
    from booster_gym_amd.utils.runner import Runner
    from booster_gym_amd.utils.sensors import GROUPS

    _, _, _, d = _train(teacher_ck, FULL, keep=True)
    ck = d.checkpoint_dict()
    want = {"bias": FULL_BIAS, "latency_steps": [0.0, 1.5]}
    assert set(ck["distillation"]) == {"teacher", "iteration", "loss", "student_sensors"} and ck["distillation"]["student_sensors"] == want
    path = str(tmp_path / "student.pth")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)  # (plain lists, dicts and floats: the safe loader takes the entry)
    sd = {k: v.clone() for k, v in d.student.state_dict().items()}
    over = checkpoint_student_overrides(ck)
    assert over == {"terrain.actor_heights": False, "env.num_observations": 47, "sensors.enabled": True, "sensors.bias": FULL_BIAS,
                    "sensors.latency_steps": [0.0, 1.5]} == student_cfg_overrides(d.cfg)
    del d
    r = Runner(test=True, cfg=_cfg(None, **over, **{"basic.checkpoint": path}))
    env = r.env
    assert env.sensor_model and not env.student_sensor_model and env._cfg_c.sensor_model == 1
    assert env.sensors.bias == tuple(FULL_BIAS[g] for g in GROUPS) and env.sensors.latency_steps == (0.0, 1.5)
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert r.play(max_steps=2) == 2 and env.sensor_launches >= 3
    del r, env
    ev = Evaluator(checkpoint=path, cfg=_cfg(None))
    assert ev.env.sensor_model and ev.env.sensors.latency_steps == (0.0, 1.5)
    rep = ev.run(steps=4)
    assert rep["overrides"]["sensors.enabled"] is True and rep["overrides"]["sensors.bias"] == FULL_BIAS and rep["overrides"]["sensors.latency_steps"] == [0.0, 1.5]
    del ev
    # a checkpoint without the entry yields no sensors.* override
    plain = _train(teacher_ck, ABSENT, keep=True)[3].checkpoint_dict()
    assert set(plain["distillation"]) == {"teacher", "iteration", "loss"}
    assert checkpoint_student_overrides(plain) == {"terrain.actor_heights": False, "env.num_observations": 47}
