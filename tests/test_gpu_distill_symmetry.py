"""distillation.symmetric_coef on the GPU: the student's output layer with the mirror-symmetry loss (bg_distill_head_sym) against float64 autograd,
its invariants (two calls, the deferred finish, rows past 2B, bg_distill_head's mean bits), then the Distiller: one iteration against a float64
restatement (the behaviour-cloning loop of tests/test_gpu_distill.py plus the symmetric term, clip and Adam) on the per-layer plan, on the default
student's chained plan and with a longer student history, and what forty epochs of the loss do to the student's asymmetry.

Bounds are the ones tests/test_gpu_distill.py holds bg_distill_head to (mu 2e-5, sums over the rows 1e-4 of the largest entry, float64 statistics 1e-5;
parameters after three Adam steps at the learning rate 1e-5 rtol 1e-3 / atol 2e-6, losses 1e-4).  The data follow its _head_data: the mirrored half of
the activations is drawn independently of the original half and the targets independently of mu, so d = mu(M_o x) - M_a mu(x) and mu - label are O(1)
and no gradient is a cancellation."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_distill import P, _Rec, _cfg, _head_data, _save_teacher, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 12
COEF = 10.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    from booster_gym_amd.envs.mirror import mirror_maps

    m = json.load(open(os.path.join(ROOT, "booster_gym_amd", "resources", "T1", "T1_locomotion.flat.json")))
    return mirror_maps(m["dof_names"], [a for a in m["joint_axis"] if a], [-0.2, 0, 0, 0.4, -0.25, 0] * 2, 47)


# ------------------------------------------------------------------ 1. the head
def _sym_data(B, seed):
    """_head_data on 2B rows of activations (the mirrored half its own draw) with B rows of targets."""
    h, W, b, target = _head_data(2 * B, seed)
    return h, W, b, target[:B].contiguous()


def _run_head(B, h, W, b, target, coef, act_mirror, partial=False):
    import ctypes as C

    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import head_scratch, reduce_group

    pad = 70  # sentinel rows past 2B
    mu = torch.full((2 * B + pad, A), 7.0, device=DEV)
    g_hidden = torch.full((2 * B + pad, 128), 7.0, device=DEV)
    dW, db, dbh = (torch.full(s, float("nan"), device=DEV) for s in ((A, 128), (A,), (128,)))
    st = torch.zeros(2, dtype=torch.float64, device=DEV)
    src, sign = (C.c_int32 * A)(*[int(v) for v in act_mirror[0]]), (C.c_float * A)(*[float(v) for v in act_mirror[1]])
    args = [B] + [_lib.ptr(t) for t in (h, W, b, target)] + [coef, src, sign] + [_lib.ptr(t) for t in (mu, g_hidden, dW, db, dbh, st, head_scratch(DEV))]
    lib = _lib.load()
    if partial:
        fin = _lib.ReduceProblem()
        _lib.check(lib.bg_distill_head_sym_partial(*args, fin, _lib.current_stream_ptr()), "bg_distill_head_sym_partial")
        torch.cuda.synchronize()
        assert torch.isnan(dW).all() and torch.isnan(db).all() and torch.isnan(dbh).all() and not st.any()  # nothing reduced yet
        reduce_group([fin])
    else:
        _lib.check(lib.bg_distill_head_sym(*args, _lib.current_stream_ptr()), "bg_distill_head_sym")
    torch.cuda.synchronize()
    assert torch.all(mu[2 * B :] == 7.0) and torch.all(g_hidden[2 * B :] == 7.0), "rows past 2B were written"
    return dict(mu=mu[: 2 * B], g_hidden=g_hidden[: 2 * B], dW=dW, db=db, dbh=dbh, st=st)


def _mirror_actions(mu, act_src, act_sign):
    return mu[:, torch.as_tensor(act_src, dtype=torch.long, device=mu.device)] * torch.as_tensor(act_sign, dtype=mu.dtype, device=mu.device)


@pytest.mark.parametrize("B", [1, 33, 1000, 24613])
def test_symmetric_head_matches_float64_autograd_and_is_deterministic(B):
    """B = 1: one pair; 33: one pair past a full tile of 32 pairs; 1000: ragged; 24,613 = 768 x 32 + 37: more tiles than workgroups, so a workgroup
    walks a second tile."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import head_scratch

    _, _, act_src, act_sign = _maps()
    assert not np.array_equal(act_src, np.arange(A)) and (act_sign < 0).any()  # a non-trivial M_a: the model's own
    h, W, b, target = _sym_data(B, 20 + B)
    out = _run_head(B, h, W, b, target, COEF, (act_src, act_sign))
    h64, W64, b64 = h.double().requires_grad_(), W.double().requires_grad_(), b.double().requires_grad_()
    mu_ref = h64 @ W64.t() + b64
    sse = ((mu_ref[:B] - target.double()) ** 2).sum()
    d = mu_ref[B:] - _mirror_actions(mu_ref[:B], act_src, act_sign)
    asym = (d * d).sum()
    ((sse + COEF * asym) / (A * B)).backward()
    g_ref = h64.grad * torch.where(h > 0, torch.ones_like(h), h + 1).double()  # dL/dz of the ELU layer, the derivative from its output
    errs = {"mu": rel(out["mu"], mu_ref.detach()), "g_hidden": rel(out["g_hidden"], g_ref), "grad_W": rel(out["dW"], W64.grad),
            "grad_b": rel(out["db"], b64.grad), "grad_b_hidden": rel(out["dbh"], g_ref.sum(0)),
            "stats[0]": abs(out["st"][0].item() - sse.item()) / sse.item(), "stats[1]": abs(out["st"][1].item() - asym.item()) / asym.item()}
    print(f"B {B}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"; |d|max {d.abs().max().item():.3f}, |mu - target|max "
          f"{(mu_ref[:B] - target.double()).abs().max().item():.3f}, |mu|max {mu_ref.abs().max().item():.3f}")
    assert errs["mu"] < 2e-5
    for k in ("g_hidden", "grad_W", "grad_b", "grad_b_hidden"):
        assert errs[k] < 1e-4, (k, errs[k])
    assert rel(out["g_hidden"][B:], g_ref[B:]) < 1e-4 and rel(out["g_hidden"][:B], g_ref[:B]) < 1e-4  # each half against its own largest entry
    assert errs["stats[0]"] < 1e-5 and errs["stats[1]"] < 1e-5
    again, later = _run_head(B, h, W, b, target, COEF, (act_src, act_sign)), _run_head(B, h, W, b, target, COEF, (act_src, act_sign), partial=True)
    for k in out:
        assert torch.equal(out[k], again[k]), ("two calls", k)
        assert torch.equal(out[k], later[k]), ("_partial + bg_reduce_group", k)
    # the original rows' means are bg_distill_head's bits on the same h, W, b
    mu1, gh1 = torch.empty(B, A, device=DEV), torch.empty(B, 128, device=DEV)
    dW, db, dbh, st = torch.empty(A, 128, device=DEV), torch.empty(A, device=DEV), torch.empty(128, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().bg_distill_head(B, *[_lib.ptr(t) for t in (h, W, b, target, mu1, gh1, dW, db, dbh, st, head_scratch(DEV))], _lib.current_stream_ptr()),
               "bg_distill_head")
    torch.cuda.synchronize()
    assert torch.equal(out["mu"][:B], mu1)
    # coefficient 0: the original rows carry bg_distill_head's loss alone, the mirrored rows no gradient; the asymmetry is still measured
    off = _run_head(B, h, W, b, target, 0.0, (act_src, act_sign))
    assert not off["g_hidden"][B:].any() and rel(off["g_hidden"][:B], gh1) < 1e-6 and rel(off["dW"], dW) < 1e-4
    assert off["st"][1].item() == out["st"][1].item() and abs(off["st"][0].item() - st.item()) <= 1e-9 * st.item()


# ------------------------------------------------------------------ 2. the Distiller (128 envs, T = 24)
BIG = {"env.num_envs": 128, "runner.horizon_length": 24}
N, T = 128, 24


def _distiller(teacher, frames, **over):
    from booster_gym_amd.utils.distill import Distiller

    d = Distiller(cfg=_cfg(teacher, frames, **BIG, **over))
    d.begin(recorder=_Rec())
    return d


def _student_maps(d, frames):
    from booster_gym_amd.utils.distill import student_mirror_maps

    axes = [int(a) for a in d.env.model.joint_axis if int(a) != 0]
    return student_mirror_maps(d.env.dof_names, axes, d.env.default_dof_pos[0].cpu().numpy(), frames)


def _check_one_symmetric_iteration(d, s_frames, kin, plan, wgrad):
    """rollout(), then update() against float64 autograd of both terms + clip_grad_norm_ + torch.optim.Adam on the same rows and labels."""
    from booster_gym_amd.utils.model import ActorCritic

    B, Fs = T * N, 47 * s_frames
    assert d.symmetry and d.symmetric_coef == COEF and (d.T, d.N, d.B) == (T, N, B) and d.student_obs == Fs
    assert d._student_in.shape == (2 * B, kin) and (d._sup.mlp.plan.fwd, d._sup.mlp.plan.bwd) == (plan, plan) and all(d._sup.mlp.plan.grouped[:-1])
    assert d._sup.wgrad_terms == wgrad
    d.rollout()
    torch.cuda.synchronize()
    obs_src, obs_sign, act_src, act_sign = _student_maps(d, s_frames)
    src_rows = d.buffer["student_obses" if d.history else "obses"][:T].reshape(B, -1)[:, :Fs]
    rows, y = src_rows.double(), d.buffer["teacher_mu"].reshape(B, A).double()
    mrows = rows[:, torch.as_tensor(obs_src, dtype=torch.long, device=DEV)] * torch.as_tensor(obs_sign, dtype=torch.float64, device=DEV)
    ref = ActorCritic(A, Fs, 14 + P, d.dcfg.student_hidden).to(DEV)
    ref.load_state_dict(d.student.state_dict())
    ref = ref.double()
    opt, ref_bc, ref_sym = torch.optim.Adam(ref.actor.parameters(), lr=1.0e-5), [], []
    for _ in range(3):
        opt.zero_grad()
        mu = ref.actor(rows)
        bc, sym = ((mu - y) ** 2).mean(), ((ref.actor(mrows) - _mirror_actions(mu, act_src, act_sign)) ** 2).mean()
        (bc + COEF * sym).backward()
        torch.nn.utils.clip_grad_norm_(ref.actor.parameters(), 1.0)
        opt.step()
        ref_bc.append(bc.item()); ref_sym.append(sym.item())
    total = [a + COEF * s for a, s in zip(ref_bc, ref_sym)]
    assert total[0] > total[1] > total[2] > 0 and min(ref_sym) > 0, (ref_bc, ref_sym)  # (the set-up trains: a failure below points at the code)
    p_start = {k: p.detach().clone() for k, p in d.student.actor.named_parameters()}
    losses = d.update().cpu().tolist()
    sym_losses = d.symmetry_losses.cpu().tolist()
    torch.cuda.synchronize()
    # the input: the batch, then its mirror images, the padded columns zero
    x = d._student_in
    assert torch.equal(x[:B, :Fs], src_rows) and torch.equal(x[B:, :Fs].double(), mrows) and not x[:, Fs:].any()
    print("losses", losses, sym_losses, "restatement", ref_bc, ref_sym)
    for a, b in zip(losses + sym_losses, ref_bc + ref_sym):
        assert abs(a - b) <= 1e-4 * abs(b), (losses, sym_losses, ref_bc, ref_sym)
    for (k, p), (k2, q) in zip(d.student.actor.named_parameters(), ref.actor.named_parameters()):
        assert k == k2 and not torch.equal(p, p_start[k]), k
        print(k, "max |p - restatement|", (p.double() - q).abs().max().item(), "moved", (q - p_start[k].double()).abs().max().item())
        assert torch.allclose(p.double(), q, rtol=1e-3, atol=2e-6), (k, (p.double() - q).abs().max().item())


def test_one_symmetric_iteration_on_the_per_layer_plan_matches_the_float64_restatement(tmp_path):
    """H = 2: the student's 94 columns are padded to 128, so its layers run one by one on the 2B = 6,144 rows, and the weight gradients in fp32."""
    d = _distiller(_save_teacher(str(tmp_path / "teacher.pth")), 2, **{"distillation.symmetric_coef": COEF})
    _check_one_symmetric_iteration(d, 2, 128, "layer", 0)
    d.buffer.roll()
    d.iteration_count += 1
    d.train_iteration(1)  # what is logged and saved with the loss on
    assert set(d.recorder.stats[1]) == {"distill/behaviour_loss", "distill/symmetry_loss"} and d.recorder.stats[1]["distill/symmetry_loss"] == d.last_symmetry_loss > 0
    entry = d.checkpoint_dict()["distillation"]
    assert entry["symmetric_coef"] == COEF and "teacher_action_prob" not in entry and entry["loss"] == d.last_loss


def test_one_symmetric_iteration_on_the_default_student_matches_the_float64_restatement(tmp_path):
    """H = 1, the shipped student: 47 columns padded to 64 and 256-128-128 run the chained split-bf16 launches on the 2B rows, with the 9-product
    bf16 weight gradients."""
    d = _distiller(_save_teacher(str(tmp_path / "teacher_h1.pth"), 1), 1, **{"distillation.symmetric_coef": COEF})
    _check_one_symmetric_iteration(d, 1, 64, "chain_split", 9)


def test_one_symmetric_iteration_with_a_longer_student_history_matches_the_float64_restatement(tmp_path):
    """H = 2, Hs = 3: the mirror map is the single observation's tiled over the student's three frames (141 columns padded to 256)."""
    d = _distiller(_save_teacher(str(tmp_path / "teacher.pth")), 2, **{"distillation.symmetric_coef": COEF, "distillation.student_frame_stack": 3})
    assert d.history
    _check_one_symmetric_iteration(d, 3, 256, "layer", 0)


def _asymmetry(d):
    """sum_r |mu(M_o x_r) - M_a mu(x_r)|^2 / (A B) of the student as it stands on the rollout's rows: one head call, nothing stepped."""
    from booster_gym_amd.utils.utils import mirror_rows

    B, Fs = d.B, d.student_obs
    obs_src, obs_sign, act_src, act_sign = _student_maps(d, Fs // 47)
    x = d.buffer["obses"][: d.T].reshape(B, -1)[:, :Fs].contiguous()
    xx = torch.cat([x, mirror_rows(x, torch.empty_like(x), obs_src.tolist(), obs_sign.tolist())])
    with torch.no_grad():
        h = d.student.actor[:-1](xx).contiguous()
    out = d.student.actor[-1]
    st = _run_head(B, h, out.weight.detach(), out.bias.detach(), d.buffer["teacher_mu"].reshape(B, A), 0.0, (act_src, act_sign))["st"]
    return st[1].item() / (A * B), st[0].item() / (A * B)


def test_forty_epochs_of_the_loss_leave_a_more_symmetric_student(tmp_path):
    """One fixed buffer (one rollout of the untrained student, the same in both runs: one seed), forty epochs at the shipped learning rate."""
    teacher = _save_teacher(str(tmp_path / "teacher.pth"))
    res = {}
    for c in (COEF, 0.0):
        d = _distiller(teacher, 2, **{"distillation.symmetric_coef": c, "distillation.num_epochs": 40, "distillation.learning_rate": 1.0e-3})
        d.rollout()
        before = _asymmetry(d)
        losses = d.update().cpu().tolist()
        torch.cuda.synchronize()
        res[c] = dict(before=before, after=_asymmetry(d), losses=losses, logged=d.symmetry_losses.cpu().tolist() if c else None, actions=d.buffer["actions"].clone())
        del d
    on, off = res[COEF], res[0.0]
    print("symmetry loss before", on["before"][0], "after 40 epochs with c = 10", on["after"][0], "(last epoch's", on["logged"][-1], ") with c = 0", off["after"][0])
    assert torch.equal(on["actions"], off["actions"]) and on["before"] == off["before"]  # the same buffer, the same student
    assert abs(on["logged"][0] - on["before"][0]) <= 1e-4 * on["before"][0]  # (the first epoch's statistic is the untrained student's)
    assert on["after"][0] < off["after"][0] and on["logged"][-1] < off["after"][0]
    assert on["after"][0] < on["before"][0]  # and it fell
    assert on["losses"][-1] < on["losses"][0] and off["losses"][-1] < off["losses"][0]  # both still learn the labels
