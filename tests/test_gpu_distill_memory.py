"""distillation.student_memory on the GPU: the recurrent student's four launches against float64 restatements of torch.nn.GRUCell's equations and
against their memoryless siblings (bitwise where they share a body), then the Distiller with a GRU student: one update against float64 autograd of
the whole loss (back-propagation through the iteration's steps from the stored state) and a float64 Adam loop, the carried state across iterations,
reproducibility, the checkpoint's way back through Evaluator, Runner.play and export_model.py, and the key off against the key absent.

Bounds: tests/test_gpu_distill.py's for the actor kernels (2e-5 max(1, |ref|max)) on every forward quantity; gradients 1e-4 of the tensor's largest
entry (torch's own fp32 autograd of the recurrence sits at 4e-7 of it; a wrong or missing term moves a tensor by O(1)); parameters after an update
rtol 1e-3, atol 2e-6 at the learning rate 1e-5.  Shapes: N = 40 = two 16-row tiles and a tail of 8; T = 5; both widths of the cell (every other shape of the four launches:
tests/test_gpu_gru_shapes.py)."""
import copy
import functools
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_distill import _Rec, _cfg, _descs, _save_teacher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 12
SEED, COUNTER = 987654321, 23
TRUNK = (256, 128, 128)
NEW_ENTRY_POINTS = ("bg_actor_sample_gru", "bg_distill_act_gru", "bg_gru_sequence_forward", "bg_gru_sequence_backward")


def _bound(x, ref, what, rule=2e-5):
    err, top = (x.double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max error {err:.3e}, |ref|max {top:.3f}")
    assert err <= rule * max(1.0, top), what


def _grad_bound(x, ref, what):
    err, top = (x.double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max error {err:.3e} = {err / top:.3e} of |ref|max {top:.3e}")
    assert err <= 1e-4 * top, what


def _cell_f64(m, x, h):
    """torch.nn.GRUCell's equations in float64: (r, z, n, gh_n, h')."""
    H = m.hidden_size
    gi = x.double() @ m.weight_ih.double().t() + m.bias_ih.double()
    gh = h.double() @ m.weight_hh.double().t() + m.bias_hh.double()
    r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H : 2 * H] + gh[:, H : 2 * H])
    n = torch.tanh(gi[:, 2 * H :] + r * gh[:, 2 * H :])
    return r, z, n, gh[:, 2 * H :], (1 - z) * n + z * h.double()


def _student(H, seed=5, P=0, trunk=TRUNK):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(seed)
    s = ActorCritic(A, 47, 14 + P, trunk, memory_hidden=H).to(DEV)
    with torch.no_grad():
        s.logstd.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    return s


def _sample_gru(model, obs, reset, h_in, N, h_out=None, mu=True, counter=COUNTER):
    """(h_out, mu, actions) of bg_actor_sample_gru on the first N rows; the 16 sentinel rows behind every output are checked."""
    from booster_gym_amd import _lib

    H = model.memory_hidden
    inplace = h_out is not None
    if not inplace:
        h_out = torch.full((N + 16, H), 7.0, device=DEV)
    mu_t, act = torch.full((N + 16, A), 7.0, device=DEV), torch.full((N + 16, A), 7.0, device=DEV)
    sd, ns = _descs(model)
    gd = model.gru_descriptor()
    p = _lib.ptr
    _lib.check(_lib.load().bg_actor_sample_gru(N, p(obs), obs.shape[1], gd, ns, sd, p(model.logstd), SEED, counter, p(reset), p(h_in), p(h_out),
                                               p(mu_t) if mu else None, p(act), _lib.current_stream_ptr()), "bg_actor_sample_gru")
    torch.cuda.synchronize()
    assert torch.all(act[N:] == 7.0) and torch.all(mu_t[N:] == 7.0), "rows past N were written"
    if not inplace:
        assert torch.all(h_out[N:] == 7.0), "rows of h_out past N were written"
    return h_out[:N], mu_t[:N], act[:N]


def _inputs(N, H, width=47, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = torch.randn(N, width, generator=g).to(DEV)
    h_in = (torch.randn(N + 16, H, generator=g) * 0.5).to(DEV)
    reset = (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    assert 0 < int(reset.sum()) < N
    return obs, h_in, reset


# ------------------------------------------------------------------ 1. bg_actor_sample_gru
@pytest.mark.parametrize("H,trunk", [(128, TRUNK), (256, TRUNK), (128, (512, 128)), (256, (512, 128))])
def test_actor_sample_gru(H, trunk):
    """The trunk 512-128 takes the 512-wide LDS form of the launch at either width of the cell."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    N = 40
    model = _student(H, trunk=trunk)
    obs, h_in, reset = _inputs(N, H)
    h_out, mu, act = _sample_gru(model, obs, reset, h_in, N)
    h0 = h_in[:N] * (1 - reset.float()).view(N, 1)
    h_ref = _cell_f64(model.memory, obs, h0)[4]
    mu_ref = copy.deepcopy(model.actor).double()(h_ref).detach()
    _bound(h_out, h_ref.detach(), f"H {H} h_out")
    _bound(mu, mu_ref, f"H {H} mu")
    # a reset row is the row of a call whose h_in is zero there
    zeroed = h_in.clone()
    zeroed[:N][reset.bool()] = 0.0
    for x, y, what in zip(_sample_gru(model, obs, None, zeroed, N), (h_out, mu, act), ("h_out", "mu", "actions")):
        assert torch.equal(x, y), ("reset against a zeroed h_in", what)
    assert not torch.equal(_sample_gru(model, obs, None, h_in, N)[0], h_out)  # (the reset matters)
    # in place, twice, without mu
    h = h_in.clone()
    for x, y, what in zip(_sample_gru(model, obs, reset, h, N, h_out=h), (h_out, mu, act), ("h_out", "mu", "actions")):
        assert torch.equal(x, y), ("in place", what)
    assert torch.equal(h[N:], h_in[N:]), "rows of the state past N were written"
    again = _sample_gru(model, obs, reset, h_in, N)
    assert all(torch.equal(x, y) for x, y in zip(again, (h_out, mu, act)))
    assert torch.equal(_sample_gru(model, obs, reset, h_in, N, mu=False)[2], act)
    # the noise is bg_actor_sample_mlp's
    torch.manual_seed(1)
    plain = ActorCritic(A, 47, 14, TRUNK).to(DEV)
    with torch.no_grad():
        plain.logstd.copy_(model.logstd)
    sd, ns = _descs(plain)
    mu2, act2 = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp(N, _lib.ptr(obs), ns, sd, _lib.ptr(plain.logstd), SEED, COUNTER, _lib.ptr(mu2), _lib.ptr(act2),
                                               _lib.current_stream_ptr()), "bg_actor_sample_mlp")
    torch.cuda.synchronize()
    std = model.logstd.exp()
    noise, noise2 = (act - mu) / std, (act2 - mu2) / std
    print(f"H {H} noise difference {(noise - noise2).abs().max().item():.3e}, |noise|max {noise.abs().max().item():.3f}")
    assert noise.abs().max().item() > 1.0 and (noise - noise2).abs().max().item() <= 1e-6


def test_gru_argument_errors_name_the_entry_point():
    from booster_gym_amd import _lib

    lib, o = _lib.load(), torch.zeros(4, 1024, device=DEV)
    p = o.data_ptr()
    net = lambda k: (_lib.MlpLayerDesc * 3)(_lib.MlpLayerDesc(p, p, k, 128), _lib.MlpLayerDesc(p, p, 128, 128), _lib.MlpLayerDesc(p, p, 128, 12))
    gru = lambda i, h: _lib.GruDesc(p, p, p, p, i, h)
    call = lambda g, k, stride=47: lib.bg_actor_sample_gru(4, p, stride, g, 3, net(k), p, 0, 0, None, p, p, None, p, None)
    for args, rc in (((gru(47, 64), 64), -4), ((gru(48, 128), 128), -4), ((gru(47, 128), 256), -4), ((gru(47, 128), 128, 46), -1)):
        assert call(*args) == rc and b"bg_actor_sample_gru" in lib.bg_last_error(), (args, lib.bg_last_error())
    dcall = lambda beta, h=128: lib.bg_distill_act_gru(4, p, 52, 3, net(52), 5, gru(47, h), 3, net(128), p, 0, 0, beta, 1, None, p, p, None, p, p, None)
    for beta in (1.5, float("nan")):
        assert dcall(beta) == -1 and b"bg_distill_act_gru" in lib.bg_last_error() and b"beta" in lib.bg_last_error()
    assert dcall(0.5, 512) == -4 and b"bg_distill_act_gru" in lib.bg_last_error()
    for name in ("bg_gru_sequence_forward", "bg_gru_sequence_backward"):
        fn = getattr(lib, name)
        assert fn(2, 4, 64, *[p] * 9) == -4 and name.encode() in lib.bg_last_error()
        assert fn(0, 4, 128, *[p] * 9) == -1 and name.encode() in lib.bg_last_error()
        assert fn(2, 4, 128, None, *[p] * 8) == -1 and name.encode() in lib.bg_last_error()


# ------------------------------------------------------------------ 2. bg_distill_act_gru
def _distill_gru(student, teacher, tobs, P, reset, h_in, N, beta, noise=1):
    from booster_gym_amd import _lib

    H = student.memory_hidden
    h_out = torch.full((N + 16, H), 7.0, device=DEV)
    outs = [torch.full((N + 16, A), 7.0, device=DEV) for _ in range(3)]  # student mu, actions, teacher mu
    (sd, ns), (td, nt), p = _descs(student), _descs(teacher), _lib.ptr
    _lib.check(_lib.load().bg_distill_act_gru(N, p(tobs), tobs.shape[1], nt, td, P, student.gru_descriptor(), ns, sd, p(student.logstd), SEED, COUNTER, beta, noise,
                                              p(reset), p(h_in), p(h_out), *[p(t) for t in outs], _lib.current_stream_ptr()), "bg_distill_act_gru")
    torch.cuda.synchronize()
    for t in outs + [h_out]:
        assert torch.all(t[N:] == 7.0), "rows past N were written"
    return [h_out[:N]] + [t[:N] for t in outs]


@pytest.mark.parametrize("H,t_hidden", [(128, TRUNK), (256, TRUNK), (128, (512, 256, 128)), (256, (512, 256, 128))])
def test_distill_act_gru(H, t_hidden):
    """A 512-wide teacher puts both halves on the 512-wide LDS form."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    N, P = 40, 5
    student = _student(H, P=P)
    torch.manual_seed(9)
    teacher = ActorCritic(A, 47 + P, 14 + P, t_hidden).to(DEV)
    tobs, h_in, reset = _inputs(N, H, width=47 + P)  # (obs_stride = 52: the student reads the first 47 columns of each row)
    h_out, s_mu, act, t_mu = _distill_gru(student, teacher, tobs, P, reset, h_in, N, 0.0)
    # the teacher's half: bg_actor_sample_mlp_scan, under the student's logstd for the beta = 1 case below
    (td, nt) = _descs(teacher)
    mu_t, act_t = torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
    _lib.check(_lib.load().bg_actor_sample_mlp_scan(N, _lib.ptr(tobs), nt, td, P, _lib.ptr(student.logstd), SEED, COUNTER, _lib.ptr(mu_t), _lib.ptr(act_t),
                                                    _lib.current_stream_ptr()), "bg_actor_sample_mlp_scan")
    torch.cuda.synchronize()
    assert torch.equal(t_mu, mu_t)
    # the student's half: bg_actor_sample_gru on the same rows at the same stride
    for x, y, what in zip(_sample_gru(student, tobs, reset, h_in, N), (h_out, s_mu, act), ("h_out", "student_mu", "actions")):
        assert torch.equal(x, y), ("beta = 0 against bg_actor_sample_gru", what)
    # beta = 1: the teacher's mean plus the student's noise; the memory advances all the same
    one = _distill_gru(student, teacher, tobs, P, reset, h_in, N, 1.0)
    assert torch.equal(one[2], act_t) and not torch.equal(act_t, mu_t)
    assert torch.equal(one[0], h_out) and torch.equal(one[1], s_mu) and torch.equal(one[3], t_mu)
    # beta = 0.5: the teacher-driven rows are bg_distill_act_mix's at the same seed and counter
    torch.manual_seed(2)
    plain = ActorCritic(A, 47, 14 + P).to(DEV)
    with torch.no_grad():
        plain.logstd.copy_(student.logstd)
    mix = [torch.empty(N, A, device=DEV) for _ in range(3)]
    (pd, npl) = _descs(plain)
    _lib.check(_lib.load().bg_distill_act_mix(N, _lib.ptr(tobs), tobs.shape[1], _lib.ptr(tobs), tobs.shape[1], npl, pd, nt, td, P, _lib.ptr(plain.logstd), SEED, COUNTER,
                                              0.5, 0, *[_lib.ptr(t) for t in mix], _lib.current_stream_ptr()), "bg_distill_act_mix")
    torch.cuda.synchronize()
    picks = (mix[1] == mix[2]).all(1)  # (teacher_noise = 0: a teacher-driven row is the teacher's mean)
    half = _distill_gru(student, teacher, tobs, P, reset, h_in, N, 0.5, 0)
    assert 0 < int(picks.sum()) < N and torch.equal((half[2] == half[3]).all(1), picks)
    assert torch.equal(half[2][~picks], act[~picks]) and torch.equal(half[0], h_out) and torch.equal(half[1], s_mu)
    noisy = _distill_gru(student, teacher, tobs, P, reset, h_in, N, 0.5, 1)
    assert torch.equal(noisy[2][picks], act_t[picks]) and torch.equal(noisy[2][~picks], act[~picks])


# ------------------------------------------------------------------ 3. / 4. the update's recurrence
@functools.lru_cache(maxsize=None)
def _sequence(H):
    """Inputs of the two sequence launches, the forward launch's outputs and the float64 restatement with its autograd gradients (computed once):
    tests/parity_util.gru_sequence_case at this file's one shape."""
    from parity_util import gru_sequence_case

    T, N = 5, 40
    c = gru_sequence_case(T, N, H, device=DEV)
    cell, gi, h0, reset, dh_ext = c["cell"], c["gi"], c["h0"], c["reset"], c["dh_ext"]
    assert 0 < int(reset[0].sum()) < N and 0 < int(reset[1:].sum())
    pad = lambda w: torch.full((T * N + 16, w), 7.0, device=DEV)
    run = lambda: _run_forward(T, N, H, gi, h0, reset, cell, [pad(H), pad(H), pad(4 * H)])
    out, again = run(), run()
    return dict(T=T, N=N, cell=cell, gi=gi, h0=h0, reset=reset, dh_ext=dh_ext, out=out, again=again, ref=c["ref"])


def _run_forward(T, N, H, gi, h0, reset, cell, bufs):
    from booster_gym_amd import _lib

    p = _lib.ptr
    _lib.check(_lib.load().bg_gru_sequence_forward(T, N, H, p(gi), p(h0), p(reset), p(cell.weight_hh), p(cell.bias_hh), *[p(t) for t in bufs],
                                                   _lib.current_stream_ptr()), "bg_gru_sequence_forward")
    torch.cuda.synchronize()
    for t in bufs:
        assert torch.all(t[T * N :] == 7.0), "rows past the last step's row N were written"
    return [t[: T * N].view(T, N, -1) for t in bufs]


@pytest.mark.parametrize("H", [128, 256])
def test_gru_sequence_forward(H):
    s = _sequence(H)
    (h_prev, h, gates), ref = s["out"], s["ref"]
    for x, name in ((h_prev, "h_prev"), (h, "h"), (gates, "gates")):
        _bound(x, ref[name], f"H {H} {name}")
    on = s["reset"].bool()
    assert torch.all(h_prev[on] == 0.0) and torch.all((h_prev[~on] != 0.0).any(-1))
    assert torch.equal(h_prev[0][~on[0]], s["h0"][~on[0]]) and torch.equal(h_prev[1:][~on[1:]], h[:-1][~on[1:]])
    for x, y in zip(s["out"], s["again"]):
        assert torch.equal(x, y), "two calls differ"


@pytest.mark.parametrize("H", [128, 256])
def test_gru_sequence_backward(H):
    from booster_gym_amd import _lib

    s = _sequence(H)
    T, N, ref, p = s["T"], s["N"], s["ref"], _lib.ptr
    h_prev, _, gates = s["out"]

    def run():
        dgi, dgh = (torch.full((T * N + 16, 3 * H), 7.0, device=DEV) for _ in range(2))
        dh0 = torch.full((N + 16, H), 7.0, device=DEV)
        _lib.check(_lib.load().bg_gru_sequence_backward(T, N, H, p(s["dh_ext"]), p(gates), p(h_prev), p(s["reset"]), p(s["cell"].weight_hh), p(dgi), p(dgh), p(dh0),
                                                        _lib.current_stream_ptr()), "bg_gru_sequence_backward")
        torch.cuda.synchronize()
        assert torch.all(dgi[T * N :] == 7.0) and torch.all(dgh[T * N :] == 7.0) and torch.all(dh0[N:] == 7.0), "rows past N were written"
        return dgi[: T * N].view(T, N, -1), dgh[: T * N].view(T, N, -1), dh0[:N]

    out = run()
    for x, name in zip(out, ("dgi", "dgh", "dh0")):
        _grad_bound(x, ref[name], f"H {H} {name}")
    assert torch.all(out[2][s["reset"][0].bool()] == 0.0)
    for x, y in zip(out, run()):
        assert torch.equal(x, y), "two calls differ"
    # dh0 may be NULL (the trainer's call)
    dgi2, dgh2 = torch.empty_like(out[0]), torch.empty_like(out[1])
    _lib.check(_lib.load().bg_gru_sequence_backward(T, N, H, p(s["dh_ext"]), p(gates), p(h_prev), p(s["reset"]), p(s["cell"].weight_hh), p(dgi2), p(dgh2), None,
                                                    _lib.current_stream_ptr()), "bg_gru_sequence_backward")
    torch.cuda.synchronize()
    assert torch.equal(dgi2, out[0]) and torch.equal(dgh2, out[1])


# ------------------------------------------------------------------ 5. - 8. the Distiller with a recurrent student
from test_gpu_distill import N as NE, P as PS, T as TS  # 64 envs, 15 scan points, horizon 4

MEM = 128


@pytest.fixture(scope="module")
def teacher_ck(tmp_path_factory):
    return _save_teacher(str(tmp_path_factory.mktemp("teacher") / "teacher_h1.pth"), 1)


def _distiller(teacher, **over):
    from booster_gym_amd.utils.distill import Distiller

    d = Distiller(cfg=_cfg(teacher, 1, **{"distillation.student_memory": MEM, **over}))
    d.begin(recorder=_Rec())
    return d


def _trained(model):
    return [(k, p) for k, p in model.named_parameters() if k.startswith(("memory.", "actor."))]


def _loss_f64(ref, rows, y, h0, resets):
    """The update's loss in float64: the cell over the T steps from h0 (zero state behind a reset), the trunk on every state, the mean squared error."""
    h, sse = h0, 0.0
    for t in range(rows.shape[0]):
        h = ref.memory(rows[t], h * (1 - resets[t].double()).view(-1, 1))
        sse = sse + ((ref.actor(h) - y[t]) ** 2).sum()
    return sse / y.numel(), h


def test_one_update_matches_float64_autograd_through_time(teacher_ck):
    from booster_gym_amd.utils.model import ActorCritic

    d = _distiller(teacher_ck)
    tr = d._sup.gru
    assert d.memory == MEM and d.student.actor[0].in_features == MEM and (d._sup.mlp.plan.fwd, d._sup.mlp.plan.bwd) == ("layer", "layer")
    assert [k for k, _ in _trained(d.student)] == [k for k, p in d.student.named_parameters() if any(p is q for q in d.optimizer.params)]
    d.rollout()  # a rollout first: the one below starts from a state that is not zero (no update: Adam's moments start with the restatement's)
    d.buffer.roll()
    frozen = lambda: {**{"student." + k: v.clone() for k, v in d.student.state_dict().items() if not k.startswith(("actor.", "memory."))},
                      **{"teacher." + k: v.clone() for k, v in d.teacher.state_dict().items()}}
    before = frozen()
    d.rollout()
    torch.cuda.synchronize()
    assert tr.h0.abs().max().item() > 1e-3 and torch.equal(tr.resets[1:].bool(), d.buffer["dones"][: TS - 1])
    rows, y = d.buffer["obses"][:TS, :, :47].double(), d.buffer["teacher_mu"].double()
    ref = ActorCritic(A, 47, 14 + PS, d.dcfg.student_hidden, memory_hidden=MEM).to(DEV)
    ref.load_state_dict(d.student.state_dict())
    ref = ref.double()
    params = [p for _, p in _trained(ref)]
    opt, ref_losses, ref_grads, h_last = torch.optim.Adam(params, lr=1.0e-5), [], None, None
    for _ in range(3):
        opt.zero_grad()
        loss, h_end = _loss_f64(ref, rows, y, tr.h0.double(), tr.resets)
        loss.backward()
        if ref_grads is None:
            ref_grads, h_last = {k: p.grad.clone() for k, p in _trained(ref)}, h_end.detach()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        ref_losses.append(loss.item())
    assert ref_losses[0] > ref_losses[1] > ref_losses[2] > 0, ref_losses
    # the first epoch's gradients, and the state its recurrence ends in, read in front of the first optimiser step
    first, step = {}, d.optimizer.step

    def spy():
        if not first:
            first.update({k: p.grad.clone() for k, p in _trained(d.student)}, h=tr.h[-NE:].clone())
        step()

    d.optimizer.step = spy
    p_start = {k: p.detach().clone() for k, p in _trained(d.student)}
    losses = d.update().cpu().tolist()
    torch.cuda.synchronize()
    print("losses", losses, "restatement", ref_losses)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 1e-4 * abs(b), (losses, ref_losses)
    _bound(first.pop("h"), h_last, "the update's last state against float64")
    _bound(d.state, h_last, "the rollout's state against float64")  # (the rollout and the update walk the same steps from the same h0)
    assert set(first) == set(ref_grads) and len(first) == 12
    for k in ref_grads:
        _grad_bound(first[k], ref_grads[k], f"grad {k}")
    for (k, p), (k2, q) in zip(_trained(d.student), _trained(ref)):
        assert k == k2 and not torch.equal(p, p_start[k]), k
        print(k, "max |p - restatement|", (p.double() - q).abs().max().item(), "moved", (q - p_start[k].double()).abs().max().item())
        assert torch.allclose(p.double(), q, rtol=1e-3, atol=2e-6), (k, (p.double() - q).abs().max().item())
    after = frozen()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)  # critic, logstd and the teacher: not a bit moved


def _digest(d):
    h = hashlib.sha256()
    for t in list(d.student.state_dict().values()) + [d.state]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_the_state_carries_over_iterations_and_runs_reproduce(teacher_ck):
    digests = []
    for run in range(2):
        d = _distiller(teacher_ck)
        tr = d._sup.gru
        assert torch.all(d.state == 0)
        for it in range(3):
            state, last = d.state.clone(), d._last_dones.clone()
            d.train_iteration(it)
            torch.cuda.synchronize()
            assert torch.equal(tr.h0, state) and torch.equal(tr.resets[0], last), it  # h0 of this iteration = the state the one before ended in
            assert torch.equal(d._last_dones.bool(), d.buffer["dones"][TS - 1]) and not torch.equal(d.state, state)
        assert set(d.recorder.stats[2]) == {"distill/behaviour_loss"} and d.recorder.stats[2]["distill/behaviour_loss"] > 0
        digests.append(_digest(d))
        del d
    assert digests[0] == digests[1]


def test_dagger_mixing_with_a_recurrent_student(monkeypatch, teacher_ck):
    from booster_gym_amd import _lib

    d = _distiller(teacher_ck, **{"distillation.teacher_action_prob": 0.5})
    calls, lib = [], _lib.load()

    def wrap(*a, _fn=lib.bg_distill_act_gru):
        calls.append(a)
        return _fn(*a)

    monkeypatch.setattr(lib, "bg_distill_act_gru", wrap)
    for it in range(2):
        d.train_iteration(it)
    torch.cuda.synchronize()
    assert len(calls) == 2 * TS and all(a[12] == 0.5 and a[13] == 1 for a in calls)
    assert all(set(d.recorder.stats[it]) == {"distill/behaviour_loss", "distill/teacher_action_prob"} for it in range(2))
    assert d.recorder.stats[1]["distill/teacher_action_prob"] == 0.5 and d.recorder.stats[1]["distill/behaviour_loss"] > 0
    entry = d.checkpoint_dict()["distillation"]
    assert entry["student_memory"] == MEM and entry["teacher_action_prob"] == [0.5, 0]


def test_recurrent_student_re_enters_evaluator_play_and_export(teacher_ck, tmp_path):
    from booster_gym_amd.utils.distill import checkpoint_student_overrides, student_cfg_overrides
    from booster_gym_amd.utils.evaluate import Evaluator
    from booster_gym_amd.utils.runner import Runner

    d = _distiller(teacher_ck)
    d.train_iteration(0)
    ck = d.checkpoint_dict()
    assert ck["distillation"]["student_memory"] == MEM and {"memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"} <= set(ck["model"])
    path = str(tmp_path / "student.pth")
    torch.save(ck, path)
    sd = {k: v.clone() for k, v in d.student.state_dict().items()}
    over = student_cfg_overrides(d.cfg)
    assert over == {"terrain.actor_heights": False, "env.num_observations": 47, "algorithm.actor_memory": MEM} == checkpoint_student_overrides(ck)
    del d
    ev = Evaluator(checkpoint=path, cfg=_cfg(None, 1))
    assert ev.applied["algorithm.actor_memory"] == MEM and ev.model.memory_hidden == MEM
    rep = ev.run(steps=8)
    assert rep["steps"] == 8 and ev.model._memory_state.abs().max().item() > 0
    del ev
    r = Runner(test=True, cfg=_cfg(None, 1, **over, **{"basic.checkpoint": path}))
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    obs_seen, act_seen, done_seen, env = [], [], [], r.env
    reset, step = env.reset, env.step

    def spy_reset():
        out = reset()
        obs_seen.append(out[0].clone())
        return out

    def spy_step(act):
        act_seen.append(act.clone())
        out = step(act)
        obs_seen.append(out[0].clone())
        done_seen.append(out[2].clone())
        return out

    env.reset, env.step = spy_reset, spy_step
    assert r.play(max_steps=4) == 4 and len(act_seen) == 4
    del r
    # a config and a checkpoint that disagree about the memory
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory"):
        Runner(test=True, cfg=_cfg(None, 1, **{**over, "algorithm.actor_memory": 0, "basic.checkpoint": path}))
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory"):
        Runner(test=True, cfg=_cfg(None, 1, **{**over, "algorithm.actor_memory": 256, "basic.checkpoint": path}))
    plain = str(tmp_path / "plain.pth")
    torch.save({"model": {k: v for k, v in ck["model"].items() if not k.startswith("memory.")}}, plain)
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory"):
        Runner(test=True, cfg=_cfg(None, 1, **over, **{"basic.checkpoint": plain}))
    with pytest.raises(ValueError, match=r"algorithm\.actor_memory.*out of scope"):
        Runner(test=False, cfg=_cfg(None, 1, **over))
    # the exported stateful module on the rows play saw
    envv = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={path}"], cwd=str(tmp_path), env=envv, check=True,
                         timeout=300, capture_output=True, text=True)
    assert "STATEFUL" in out.stdout and "reset()" in out.stdout
    mod = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"), map_location="cpu")
    for attempt in range(2):  # ... and again behind reset()
        for t in range(4):
            y = mod(obs_seen[t].cpu())
            err = (y - act_seen[t].cpu()).abs().max().item()
            print(f"pass {attempt} step {t}: TorchScript against play {err:.3e}")
            assert tuple(y.shape) == (NE, A) and err <= 1e-5
            if bool(done_seen[t].any()):  # an env that reset enters the next step with a zero state
                h = mod.h.clone()
                h[done_seen[t].cpu().bool()] = 0.0
                mod.h = h
        assert mod.h.abs().max().item() > 0
        mod.reset()
        assert torch.all(mod.h == 0)


def test_key_off_or_absent_runs_todays_calls_alone(monkeypatch, teacher_ck):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.distill import DEFAULTS, Distiller

    lib = _lib.load()

    def forbidden(*a):
        raise AssertionError("a new entry point ran with the key off")

    for name in NEW_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, forbidden)
    names = ("bg_distill_act", "bg_distill_act_hist", "bg_distill_act_mix", "bg_distill_head_partial", "bg_env_step_to", "bg_mlp_chain_forward_split",
             "bg_mlp_chain_backward_split", "bg_mlp_layer_forward", "bg_elu_backward_colsum", "bg_mlp_weight_grad_group_split", "bg_mlp_weight_grad_group",
             "bg_reduce_group", "bg_adam_step")
    runs, entry = [], {name: getattr(lib, name) for name in names}
    for absent in (True, False):
        counts = dict.fromkeys(names, 0)
        for name in names:
            def wrap(*a, _fn=entry[name], _name=name, _counts=counts):
                _counts[_name] += 1
                return _fn(*a)
            monkeypatch.setattr(lib, name, wrap)
        cfg = _cfg(teacher_ck, 1)
        assert cfg["distillation"]["student_memory"] == DEFAULTS["student_memory"] == 0
        if absent:
            del cfg["distillation"]["student_memory"]
        d = Distiller(cfg=cfg)
        d.begin(recorder=_Rec())
        assert d.memory == 0 and not hasattr(d, "state") and not hasattr(d.student, "memory")
        assert [k for k, _ in d.student.named_parameters()] == ["logstd"] + [f"{n}.{i}.{w}" for n in ("critic", "actor") for i in (0, 2, 4, 6) for w in ("weight", "bias")]
        for it in range(2):
            d.train_iteration(it)
        torch.cuda.synchronize()
        e = d.dcfg.num_epochs
        assert counts == {"bg_distill_act": 2 * TS, "bg_distill_act_hist": 0, "bg_distill_act_mix": 0, "bg_distill_head_partial": 2 * e, "bg_env_step_to": 2 * TS,
                          "bg_mlp_chain_forward_split": 2 * e, "bg_mlp_chain_backward_split": 2 * e, "bg_mlp_layer_forward": 0, "bg_elu_backward_colsum": 0,
                          "bg_mlp_weight_grad_group_split": 2 * e, "bg_mlp_weight_grad_group": 0, "bg_reduce_group": 2 * e, "bg_adam_step": 2 * e}, counts
        assert set(d.recorder.stats[1]) == {"distill/behaviour_loss"}
        ck = d.checkpoint_dict()
        assert set(ck["distillation"]) == {"teacher", "iteration", "loss"} and not any(k.startswith("memory.") for k in ck["model"])
        runs.append(({k: v.clone() for k, v in d.student.state_dict().items()}, d.buffer["actions"].clone(), d.last_loss))
        del d
    (p0, a0, l0), (p1, a1, l1) = runs
    assert p0.keys() == p1.keys() and all(torch.equal(p0[k], p1[k]) for k in p0) and torch.equal(a0, a1) and l0 == l1
