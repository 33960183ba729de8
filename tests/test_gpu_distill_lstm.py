"""distillation.student_cell: "lstm" on the GPU: the rollout's launch against the stand-alone launches it fuses (bitwise), one Distiller update
against float64 torch.nn.LSTMCell with autograd, and the checkpoint's way back into Runner.  Bounds: tests/test_gpu_lstm.py's: 2e-5
max(1, |ref|max) forward, 1e-4 of the tensor's largest entry on gradients.  N = 40 = two 16-row tiles and a tail of 8 (nb = 3), T = 5."""
import pytest
import torch

from test_gpu_distill import _Rec, _cfg, _descs, _distiller
from test_gpu_distill_memory import _bound, _grad_bound, teacher_ck  # noqa: F401  (teacher_ck: the module's fixture)

pytestmark = pytest.mark.gpu
DEV, A, N, P, SEED, COUNTER = "cuda:0", 12, 40, 5, 987654321, 23
# an LSTM student of width H; an episode of 7 control steps: every env times out on its 8th step, so the second horizon meets resets
LSTM = lambda H, envs, T: {"distillation.student_memory": H, "distillation.student_cell": "lstm", "env.num_envs": envs, "runner.horizon_length": T,
                           "rewards.episode_length_s": 0.13}


@pytest.mark.parametrize("own", [False, True], ids=["teacher_rows", "own_rows"])
@pytest.mark.parametrize("H", [128, 256])
def test_rollout_launch_equals_the_stand_alone_launches_bitwise(H, own):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic
    torch.manual_seed(5)
    student, teacher = ActorCritic(A, 47, 14 + P, (256, 128, 128), memory_hidden=H, memory_cell="lstm").to(DEV), ActorCritic(A, 47 + P, 14 + P).to(DEV)
    student.logstd.data.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    tobs, state, reset = torch.randn(N, 47 + P, device=DEV), torch.randn(2, N, H, device=DEV) * 0.5, (torch.arange(N, device=DEV) % 5 == 1).to(torch.uint8)
    rows = torch.randn(N, 50, device=DEV) if own else tobs  # (own: a buffer of the student's, at a stride of its own)
    lib, p, st, (sd, ns), (td, nt), cell, logstd = _lib.load(), _lib.ptr, _lib.current_stream_ptr(), _descs(student), _descs(teacher), student.gru_descriptor(), student.logstd

    def launch(beta):  # (state_out [2][N][H], student mu, actions, teacher mu); the 16 sentinel rows behind every output are checked
        out, outs = torch.full((2 * N * H + 16 * H,), 7.0, device=DEV), [torch.full((N + 16, A), 7.0, device=DEV) for _ in range(3)]
        name, mid = ("bg_distill_act_lstm_own", (p(rows), rows.shape[1])) if own else ("bg_distill_act_lstm", ())
        _lib.check(getattr(lib, name)(N, p(tobs), tobs.shape[1], *mid, nt, td, P, cell, ns, sd, p(logstd), SEED, COUNTER, beta, 1, p(reset), p(state), p(out),
                                      *[p(t) for t in outs], st), name)
        torch.cuda.synchronize()
        assert all(torch.all(t[N:] == 7.0) for t in outs) and torch.all(out[2 * N * H :] == 7.0), "rows past N were written"
        return [out[: 2 * N * H].view(2, N, H)] + [t[:N] for t in outs]

    plain = launch(0.0)
    want, mu, a, mu_t, act_t = torch.empty(2, N, H, device=DEV), *(torch.empty(N, A, device=DEV) for _ in range(4))
    _lib.check(lib.bg_actor_sample_lstm(N, p(rows), rows.shape[1], cell, ns, sd, p(logstd), SEED, COUNTER, p(reset), p(state[0]), p(want[0]), p(state[1]), p(want[1]),
                                        p(mu), p(a), st), "bg_actor_sample_lstm")
    _lib.check(lib.bg_actor_sample_mlp_scan(N, p(tobs), nt, td, P, p(logstd), SEED, COUNTER, p(mu_t), p(act_t), st), "bg_actor_sample_mlp_scan")  # (the student's logstd: beta = 1 below)
    torch.cuda.synchronize()
    assert [torch.equal(x, y) for x, y in zip(plain, (want, mu, a, mu_t))] == [True] * 4 and not torch.equal(want, state)  # state, student mu, actions, teacher mu
    # the mix kernel at beta = 0 (the host picks the plain kernel at 0 itself: the smallest beta above it draws no teacher row) is the plain launch
    assert all(torch.equal(x, y) for x, y in zip(launch(1e-30), plain))
    one = launch(1.0)  # the teacher's mean plus the student's noise; both states advance all the same
    assert torch.equal(one[2], act_t) and not torch.equal(act_t, mu_t) and all(torch.equal(one[i], plain[i]) for i in (0, 1, 3))


def test_one_update_matches_float64_autograd_through_time(teacher_ck):
    """Measured on an MI355X: means 3.8e-08, state 7.6e-08, gradients 6.1e-08 to 2.1e-07 of their largest entries."""
    from booster_gym_amd.utils.model import ActorCritic, LSTMTrainer
    T, H = 5, 256
    d = _distiller(teacher_ck, 1, **LSTM(H, N, T))
    tr, mlp = d._sup.gru, d._sup.mlp
    assert isinstance(tr, LSTMTrainer) and isinstance(d.student.memory, torch.nn.LSTMCell) and tuple(d.state.shape) == (2, N, H)
    d.rollout(), d.buffer.roll(), d.rollout(), torch.cuda.synchronize()  # a rollout first: the second starts from a state that is not zero and meets resets
    resets = tr.resets
    assert min(tr.h0[0].abs().max().item(), tr.h0[1].abs().max().item()) > 1e-3 and 0 < int(resets.sum()) < T * N
    rows, y = d.buffer["obses"][:T, :, :47].double(), d.buffer["teacher_mu"].double()
    ref = ActorCritic(A, 47, d.env.num_privileged_obs, d.dcfg.student_hidden, memory_hidden=H, memory_cell="lstm").to(DEV)
    ref.load_state_dict(d.student.state_dict())
    ref, (h, c), means = ref.double(), tr.h0.double(), []
    for t in range(T):  # both states are zero behind a reset; the gradient is truncated at the stored state
        keep = (1 - resets[t].double()).view(-1, 1)
        h, c = ref.memory(rows[t], (h * keep, c * keep))
        means.append(ref.actor(h))
    means = torch.stack(means)
    ((means - y) ** 2).sum().div(y.numel()).backward()
    trained = lambda m: {k: q for k, q in m.named_parameters() if k.startswith(("memory.", "actor."))}
    first, step = {}, d.optimizer.step

    def spy():  # the first epoch's gradients and last hidden activations, read in front of the first optimiser step
        if not first:
            first.update({k: q.grad.clone() for k, q in trained(d.student).items()}, hidden=mlp.acts[len(mlp.layers) - 2].clone())
        step()

    d.optimizer.step = spy
    d.update(), torch.cuda.synchronize()
    got = (first.pop("hidden").double() @ ref.actor[-1].weight.detach().t() + ref.actor[-1].bias.detach()).view(T, N, A)
    _bound(got, means.detach(), "the student's means")
    _bound(d.state, torch.stack((h, c)).detach(), "the rollout's state against float64")
    assert set(first) == set(trained(ref)) and len(first) == 12 and first["memory.weight_hh"].shape == (4 * H, H)
    for k, q in trained(ref).items():
        _grad_bound(first[k], q.grad, f"grad {k}")


def test_the_checkpoint_re_enters_runner(teacher_ck, tmp_path):
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides
    from booster_gym_amd.utils.runner import Runner
    H, envs = 128, 128
    d = _distiller(teacher_ck, 1, **LSTM(H, envs, 4))
    d.train_iteration(0), d.train_iteration(1)
    ck, path = d.checkpoint_dict(), str(tmp_path / "student.pth")
    assert ck["distillation"]["student_cell"] == "lstm" and ck["model"]["memory.weight_hh"].shape == (4 * H, H)
    torch.save(ck, path)
    over = checkpoint_student_overrides(ck)
    assert over == student_cfg_overrides(d.cfg) and over["algorithm.actor_memory"] == H and over["algorithm.rnn_cell"] == "lstm"
    obs = torch.randn(envs, 47, generator=torch.Generator().manual_seed(3)).to(DEV)

    def mean(model):  # from the zero state, through bg_actor_sample_lstm
        model.reset_memory()
        mu, act = torch.empty(envs, A, device=DEV), torch.empty(envs, A, device=DEV)
        model.sample_actions(obs, act, SEED, COUNTER, mu_out=mu)
        torch.cuda.synchronize()
        return mu

    want = mean(d.student)
    del d
    cfg = lambda **more: _cfg(None, 1, **{**over, "env.num_envs": envs, "basic.checkpoint": path, **more})
    r = Runner(test=True, cfg=cfg())
    assert isinstance(r.model.memory, torch.nn.LSTMCell) and torch.equal(mean(r.model), want) and want.abs().max().item() > 0
    del r
    r = Runner(cfg=cfg(**{"algorithm.rnn_hidden_size": H}))  # fine-tuning: the same checkpoint under PPO's key, with the cell the overrides name
    r.begin_training(recorder=_Rec())
    assert r._rnn_cell == "lstm" and all(torch.equal(v, ck["model"][k].to(DEV)) for k, v in r.model.state_dict().items())
    assert r.optimizer.step_count == 0 and float(r.optimizer.exp_avg.abs().sum()) == 0.0  # fresh Adam moments
