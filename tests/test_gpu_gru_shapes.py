"""The recurrence's two launches (bg_gru_sequence_forward / _backward) and the rollout's cell (bg_actor_sample_gru, bg_distill_act_gru) at the shapes
tests/test_gpu_distill_memory.py's one shape (40 envs x 5 steps, reset rate 0.2, h0 and reset given) does not reach: one row, exact 16-row tiles, one row
past a tile, T = 1, the workload's horizon of 24, saturated gates, h0 == NULL, reset == NULL, three reset patterns, both parities of the forward's LDS
state tile, and the row counts of tests/test_gpu_actor_sample_packed.ROWS.

Reference: tests/parity_util.gru_sequence_case, the float64 restatement of torch.nn.GRUCell's recurrence with autograd's gradients of sum(h * dh_ext),
and an fp32 torch twin of the same loop whose error is printed beside the kernel's.  Bounds: the project's own, unchanged -- forward quantities
test_gpu_distill_memory._bound (2e-5 max(1, |ref|max)), gradients _grad_bound (1e-4 of the tensor's largest entry).  The twin stays between 1.1e-7 and
4.2e-7 of |ref|max on h, dgi, dgh and dh0 at every shape below (checked on the CPU), so the bounds keep 50 x or more over the reference's own fp32
error and no case has a bound of its own.

Every case also asserts: 16 guard rows in front of and behind every output untouched; a NaN in gi, h0, dh_ext, gates and h_prev just past the last
valid row reaches no output; two calls give equal bits.  The bitwise properties (a launch split in time, either direction; the leading rows of a
wider launch) use no bound at all.

Measured on an MI355X, error / |ref|max in units of 1e-7, the fp32 twin's in brackets (dh0 "0 (0)": the case's one row enters step 0 behind a reset):
  a:1x1              H 128  h 0.9 (0.7)  gates 0.8 (0.7)  dgi 0.8 (1.0)  dgh 1.2 (1.3)  dh0 0 (0)
  a:1x1              H 256  h 1.3 (0.8)  gates 1.8 (1.8)  dgi 0.9 (1.0)  dgh 1.3 (1.6)  dh0 1.2 (1.5)
  a:1x1_no_reset     H 128  h 0.5 (0.7)  gates 1.9 (0.9)  dgi 0.7 (1.4)  dgh 0.8 (0.8)  dh0 0.7 (1.0)
  a:1x1_no_reset     H 256  h 1.3 (0.8)  gates 1.8 (1.8)  dgi 0.9 (1.0)  dgh 1.3 (1.6)  dh0 1.2 (1.5)
  b:1x16             H 128  h 1.2 (1.0)  gates 1.9 (2.9)  dgi 0.8 (0.9)  dgh 1.1 (1.2)  dh0 1.2 (1.2)
  b:1x16             H 256  h 1.3 (1.0)  gates 2.3 (2.3)  dgi 1.1 (1.1)  dgh 1.2 (1.2)  dh0 1.3 (1.4)
  b:2x32             H 128  h 1.3 (1.0)  gates 2.2 (3.6)  dgi 1.2 (1.1)  dgh 1.2 (1.3)  dh0 1.4 (1.2)
  b:2x32             H 256  h 1.5 (1.3)  gates 3.2 (3.5)  dgi 0.9 (0.9)  dgh 1.4 (1.8)  dh0 0.9 (0.9)
  c:3x17             H 128  h 1.6 (1.2)  gates 2.2 (3.2)  dgi 1.0 (1.0)  dgh 1.4 (1.0)  dh0 1.0 (1.5)
  c:3x17             H 256  h 1.4 (1.9)  gates 2.9 (3.8)  dgi 1.1 (1.1)  dgh 1.6 (1.8)  dh0 1.2 (1.5)
  d:24x33            H 128  h 1.5 (1.6)  gates 2.3 (3.7)  dgi 2.3 (1.4)  dgh 1.8 (1.6)  dh0 1.1 (1.1)
  d:24x33            H 256  h 1.4 (1.4)  gates 4.3 (3.4)  dgi 1.0 (1.7)  dgh 1.9 (1.9)  dh0 1.6 (1.4)
  d:24x33_scale8     H 128  h 2.8 (3.2)  gates 3.0 (3.8)  dgi 1.2 (1.4)  dgh 1.2 (1.3)  dh0 1.2 (1.2)
  d:24x33_scale8     H 256  h 3.3 (3.8)  gates 3.2 (3.4)  dgi 1.6 (1.1)  dgh 1.7 (1.7)  dh0 1.6 (1.4)
  e:h0_null          H 128  h 1.8 (1.9)  gates 2.5 (3.9)  dgi 0.9 (1.3)  dgh 1.2 (1.3)  dh0 1.4 (1.3)
  e:h0_null          H 256  h 2.3 (1.5)  gates 3.4 (3.1)  dgi 1.3 (1.2)  dgh 1.4 (1.6)  dh0 1.2 (1.4)
  e:reset_null       H 128  h 1.4 (1.6)  gates 2.4 (4.4)  dgi 1.1 (1.1)  dgh 2.0 (1.7)  dh0 1.7 (1.1)
  e:reset_null       H 256  h 1.7 (1.3)  gates 5.1 (3.7)  dgi 1.4 (1.6)  dgh 1.5 (2.2)  dh0 1.9 (1.3)
  e:both_null        H 128  h 1.8 (1.9)  gates 2.5 (4.4)  dgi 1.0 (1.7)  dgh 1.4 (1.4)  dh0 1.3 (1.6)
  e:both_null        H 256  h 2.3 (1.8)  gates 3.4 (3.1)  dgi 1.2 (1.1)  dgh 1.5 (1.4)  dh0 1.2 (1.5)
  f:all_at_step2     H 128  h 1.4 (1.6)  gates 2.4 (4.4)  dgi 1.1 (1.3)  dgh 1.2 (1.0)  dh0 1.0 (1.3)
  f:all_at_step2     H 256  h 1.7 (1.1)  gates 5.1 (3.7)  dgi 0.9 (1.3)  dgh 1.2 (2.2)  dh0 1.3 (1.2)
  f:step0_only       H 128  h 1.6 (1.7)  gates 2.5 (4.5)  dgi 1.1 (1.5)  dgh 2.0 (1.7)  dh0 1.2 (1.2)
  f:step0_only       H 256  h 1.9 (1.2)  gates 5.1 (3.7)  dgi 1.4 (1.2)  dgh 1.5 (1.7)  dh0 1.9 (1.3)
  f:no_reset         H 128  h 1.4 (1.6)  gates 2.4 (4.4)  dgi 1.1 (2.0)  dgh 2.0 (1.7)  dh0 1.7 (1.2)
  f:no_reset         H 256  h 1.7 (1.3)  gates 5.1 (3.7)  dgi 1.4 (1.6)  dgh 1.5 (2.2)  dh0 1.9 (1.3)
At gi x 8, 78 % of the state entries have an n or z gate within 1e-3 of saturation and every output is finite.  The cell launches at the six row
counts: h_out within 2.2e-7 and mu within 1.2e-7 of float64 (|ref|max 1.5 / 0.27).  The rollout's 24 in-place cell launches against the update's one
launch, 33 envs: the two state sequences differ by at most 1.8e-7 (H = 128) and 1.5e-7 (H = 256), each within 2.0e-7 of float64.
No launch was found wrong."""
import copy
import functools

import pytest
import torch

from parity_util import gru_sequence_case
from test_gpu_actor_sample_packed import ROWS
from test_gpu_distill import _descs
from test_gpu_distill_memory import A, _bound, _cell_f64, _grad_bound, _student

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, CANARY = 16, 7.0
SEED, COUNTER = 987654321, 23
# name: (T, N, gi_scale, reset, h0 given) -- the issue's cases a .. f
CASES = {"a:1x1": (1, 1, 1.0, 0.2, True), "a:1x1_no_reset": (1, 1, 1.0, "none", True),  # (the rate's one flag is set: the second form reads h0 and leaves a dh0)
         "b:1x16": (1, 16, 1.0, 0.2, True), "b:2x32": (2, 32, 1.0, 0.2, True),
         "c:3x17": (3, 17, 1.0, 0.2, True),
         "d:24x33": (24, 33, 1.0, 0.2, True), "d:24x33_scale8": (24, 33, 8.0, 0.2, True),
         "e:h0_null": (5, 40, 1.0, 0.2, False), "e:reset_null": (5, 40, 1.0, None, True), "e:both_null": (5, 40, 1.0, None, False),
         "f:all_at_step2": (5, 40, 1.0, "step2", True), "f:step0_only": (5, 40, 1.0, "t0", True), "f:no_reset": (5, 40, 1.0, "none", True)}


@functools.lru_cache(maxsize=None)
def _case(T, N, H, scale=1.0, reset=0.2, h0=True):
    return gru_sequence_case(T, N, H, scale, reset, h0, device=DEV)


def _nan_tailed(x):
    """A contiguous copy of x's rows [rows][w] with one NaN row behind them: what a launch reads past its last valid row poisons its output."""
    if x is None:
        return None
    x = x.reshape(-1, x.shape[-1])
    out = torch.full((x.shape[0] + 1, x.shape[1]), float("nan"), device=DEV)
    out[:-1] = x
    return out


def _guarded(rows, w):
    full = torch.full((rows + 2 * GUARD, w), CANARY, device=DEV)
    return full, full[GUARD : GUARD + rows]


def _guards_untouched(full, rows, what):
    assert torch.all(full[:GUARD] == CANARY), f"{what}: rows in front of the output were written"
    assert torch.all(full[GUARD + rows :] == CANARY), f"{what}: rows behind the output were written"
    assert torch.isfinite(full).all(), f"{what}: a value past the last valid input row reached the output"


def _forward(T, N, H, gi, h0, reset, cell):
    """(h_prev, h, gates) [T][N][*] of one bg_gru_sequence_forward on contiguous gi [T][N][3H], h0 [N][H] or None, reset [T][N] or None."""
    from booster_gym_amd import _lib

    p = _lib.ptr
    gi_t, h0_t = _nan_tailed(gi), _nan_tailed(h0)
    bufs = [_guarded(T * N, w) for w in (H, H, 4 * H)]
    assert reset is None or (reset.is_contiguous() and tuple(reset.shape) == (T, N))
    _lib.check(_lib.load().bg_gru_sequence_forward(T, N, H, p(gi_t), p(h0_t), p(reset), p(cell.weight_hh), p(cell.bias_hh), *[p(v) for _, v in bufs],
                                                   _lib.current_stream_ptr()), "bg_gru_sequence_forward")
    torch.cuda.synchronize()
    for (full, _), name in zip(bufs, ("h_prev", "h", "gates")):
        _guards_untouched(full, T * N, name)
    return [v.view(T, N, -1) for _, v in bufs]


def _backward(T, N, H, dh_ext, gates, h_prev, reset, cell, want_dh0=True):
    """(dgi, dgh, dh0) of one bg_gru_sequence_backward on contiguous [T][N][*] inputs; dh0 is None where it is not requested."""
    from booster_gym_amd import _lib

    p = _lib.ptr
    ins = [_nan_tailed(x) for x in (dh_ext, gates, h_prev)]
    (dgi_f, dgi), (dgh_f, dgh), (dh0_f, dh0) = _guarded(T * N, 3 * H), _guarded(T * N, 3 * H), _guarded(N, H)
    _lib.check(_lib.load().bg_gru_sequence_backward(T, N, H, *[p(x) for x in ins], p(reset), p(cell.weight_hh), p(dgi), p(dgh), p(dh0) if want_dh0 else None,
                                                    _lib.current_stream_ptr()), "bg_gru_sequence_backward")
    torch.cuda.synchronize()
    _guards_untouched(dgi_f, T * N, "dgi")
    _guards_untouched(dgh_f, T * N, "dgh")
    if want_dh0:
        _guards_untouched(dh0_f, N, "dh0")
    else:
        assert torch.all(dh0_f == CANARY), "dh0 was written though not requested"
    return dgi.view(T, N, -1), dgh.view(T, N, -1), dh0 if want_dh0 else None


def _twin_error(c, name):
    ref, twin = c["ref"][name], c["twin"][name]
    return (twin.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _check_forward(x, c, name, what):
    print(f"{what} {name}: the fp32 twin's error {_twin_error(c, name):.3e} of |ref|max")
    _bound(x, c["ref"][name], f"{what} {name}")


def _check_gradient(x, c, name, what):
    ref = c["ref"][name]
    print(f"{what} {name}: the fp32 twin's error {_twin_error(c, name):.3e} of |ref|max")
    if ref.abs().max().item() == 0.0:  # (one row that enters step 0 behind a reset: dh0 is exactly zero)
        assert torch.all(x == 0.0), f"{what} {name}"
    else:
        _grad_bound(x, ref, f"{what} {name}")


# ------------------------------------------------------------------ 1. the cases a .. f
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("name", list(CASES))
def test_sequence_launches_match_float64(name, H):
    T, N, scale, reset, h0 = CASES[name]
    c = _case(T, N, H, scale, reset, h0)
    cell, what = c["cell"], f"{name} H {H}"
    fwd = lambda: _forward(T, N, H, c["gi"], c["h0"], c["reset"], cell)
    h_prev, h, gates = out = fwd()
    for x, k in zip(out, ("h_prev", "h", "gates")):
        assert torch.isfinite(x).all(), (what, k)
        _check_forward(x, c, k, what)
    for x, y in zip(out, fwd()):
        assert torch.equal(x, y), "two forward calls differ"
    bwd = lambda: _backward(T, N, H, c["dh_ext"], gates, h_prev, c["reset"], cell)
    grads = bwd()
    for x, k in zip(grads, ("dgi", "dgh", "dh0")):
        assert torch.isfinite(x).all(), (what, k)
        _check_gradient(x, c, k, what)
    for x, y in zip(grads, bwd()):
        assert torch.equal(x, y), "two backward calls differ"
    # the state entering a step: zero behind a reset, else h0 / the step before, bit for bit
    first = torch.zeros(N, H, device=DEV) if c["h0"] is None else c["h0"]
    entering = torch.cat((first.view(1, N, H), h[:-1]))
    on = torch.zeros(T, N, dtype=torch.bool, device=DEV) if c["reset"] is None else c["reset"].bool()
    assert torch.all(h_prev[on] == 0.0) and torch.equal(h_prev[~on], entering[~on])
    if name == "d:24x33_scale8":  # a large share of the gates is saturated: 1 - n n and z (1 - z) vanish in fp32
        z, n = gates[..., H : 2 * H], gates[..., 2 * H : 3 * H]
        share = ((n.abs() > 0.999) | (z < 1e-3) | (z > 0.999)).float().mean().item()
        print(f"{what}: state entries whose n or z gate is within 1e-3 of saturation: {share:.3f}")
        assert share > 0.25  # (gi_n ~ N(0, 8^2): |tanh| > 0.999 beyond |x| = 3.8, a share of 0.63 of the draws)
    if name.startswith("e:"):
        # NULL is a zero tensor: bit for bit
        zero_h0 = torch.zeros(N, H, device=DEV) if c["h0"] is None else c["h0"]
        zero_reset = torch.zeros(T, N, dtype=torch.uint8, device=DEV) if c["reset"] is None else c["reset"]
        full = _forward(T, N, H, c["gi"], zero_h0, zero_reset, cell)
        for x, y, k in zip(out, full, ("h_prev", "h", "gates")):
            assert torch.equal(x, y), (what, "NULL against a zero tensor", k)
        for x, y, k in zip(grads, _backward(T, N, H, c["dh_ext"], gates, h_prev, zero_reset, cell), ("dgi", "dgh", "dh0")):
            assert torch.equal(x, y), (what, "reset NULL against a zero tensor, backward", k)
    if name == "f:all_at_step2":
        # what flows to the steps before the reset is cut: they are the steps of a launch that ends there (dh0 with them)
        head = _backward(2, N, H, c["dh_ext"][:2].contiguous(), gates[:2].contiguous(), h_prev[:2].contiguous(), c["reset"][:2].contiguous(), cell)
        assert torch.equal(head[0], grads[0][:2]) and torch.equal(head[1], grads[1][:2]) and torch.equal(head[2], grads[2])
        assert grads[2].abs().max().item() > 0 and torch.all(h_prev[2] == 0.0)
    if name == "f:step0_only":
        on0 = c["reset"][0].bool()
        assert 0 < int(on0.sum()) < N and torch.all(grads[2][on0] == 0.0) and torch.all((grads[2][~on0] != 0.0).any(-1))
    # dh0 == NULL (the trainer's call) leaves the other two as they are
    no_dh0 = _backward(T, N, H, c["dh_ext"], gates, h_prev, c["reset"], cell, want_dh0=False)
    assert torch.equal(no_dh0[0], grads[0]) and torch.equal(no_dh0[1], grads[1])


# ------------------------------------------------------------------ 2. bitwise: a launch split in time, the leading rows of a wider launch
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("T1", [1, 2, 4])
def test_a_launch_split_in_time_reproduces_the_single_launch(T1, H):
    """An odd T1 starts the second forward launch on the LDS tile the single launch reads on even steps.  Backward: the kernel adds dh_ext + carry
    once, in fp32, and a launch starts from a zero carry, so the carry handed over as part of dh_ext[T1 - 1] gives the same bits."""
    T, N = 5, 40
    c = _case(T, N, H)
    cell, gi, reset, dh_ext = c["cell"], c["gi"], c["reset"], c["dh_ext"]
    h_prev, h, gates = whole = _forward(T, N, H, gi, c["h0"], reset, cell)
    first = _forward(T1, N, H, gi[:T1].contiguous(), c["h0"], reset[:T1].contiguous(), cell)
    second = _forward(T - T1, N, H, gi[T1:].contiguous(), first[1][T1 - 1].contiguous(), reset[T1:].contiguous(), cell)
    for a, b, w, k in zip(first, second, whole, ("h_prev", "h", "gates")):
        assert torch.equal(torch.cat((a, b)), w), ("forward", T1, k)
    dgi, dgh, dh0 = _backward(T, N, H, dh_ext, gates, h_prev, reset, cell)
    late = _backward(T - T1, N, H, dh_ext[T1:].contiguous(), gates[T1:].contiguous(), h_prev[T1:].contiguous(), reset[T1:].contiguous(), cell)
    handed = dh_ext[:T1].clone()
    handed[T1 - 1] += late[2]  # the fp32 sum of the original and the later steps' carry
    early = _backward(T1, N, H, handed, gates[:T1].contiguous(), h_prev[:T1].contiguous(), reset[:T1].contiguous(), cell)
    assert torch.equal(torch.cat((early[0], late[0])), dgi) and torch.equal(torch.cat((early[1], late[1])), dgh) and torch.equal(early[2], dh0), ("backward", T1)
    assert late[2].abs().max().item() > 0


@pytest.mark.parametrize("H", [128, 256])
def test_the_leading_rows_of_a_wider_launch_are_the_narrow_launch(H):
    """17 of 48 rows: the second workgroup's one valid row and 15 tail rows against a full tile of the same workgroup."""
    T, N, M = 5, 48, 17
    c = _case(T, N, H)
    cell = c["cell"]
    cut = lambda x: x[:, :M].contiguous()
    wide = _forward(T, N, H, c["gi"], c["h0"], c["reset"], cell)
    narrow = _forward(T, M, H, cut(c["gi"]), c["h0"][:M].contiguous(), cut(c["reset"]), cell)
    for a, b, k in zip(narrow, wide, ("h_prev", "h", "gates")):
        assert torch.equal(a, cut(b)), ("forward", k)
    wide_g = _backward(T, N, H, c["dh_ext"], wide[2], wide[0], c["reset"], cell)
    narrow_g = _backward(T, M, H, cut(c["dh_ext"]), narrow[2], narrow[0], cut(c["reset"]), cell)
    assert torch.equal(narrow_g[0], cut(wide_g[0])) and torch.equal(narrow_g[1], cut(wide_g[1])) and torch.equal(narrow_g[2], wide_g[2][:M])


# ------------------------------------------------------------------ 3. the rollout's cell launches
def _teacher(P, hidden=(256, 128, 128)):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(9)
    return ActorCritic(A, 47 + P, 14 + P, hidden).to(DEV)


def _cell_launch(kind, model, obs_store, reset, h_store, N, inplace=False, teacher=None, P=0):
    """One bg_actor_sample_gru / bg_distill_act_gru (beta = 0) on the first N rows of obs_store [N + 1][stride] and of the state h_store
    [GUARD + N + 1 + GUARD][H] (guard rows around the N states and the one NaN row behind them).  Returns (h_out, mu) [N][*]; every output's guard
    rows are checked on both sides.  inplace: h_out is h_in, on a copy of h_store."""
    from booster_gym_amd import _lib

    H, p, lib = model.memory_hidden, _lib.ptr, _lib.load()
    h_full = h_store.clone()
    h_in = h_full[GUARD : GUARD + N]
    if inplace:
        out_full, h_out = h_full, h_in
    else:
        out_full, h_out = _guarded(N, H)
    (mu_f, mu), (act_f, act), (tmu_f, tmu) = _guarded(N, A), _guarded(N, A), _guarded(N, A)
    sd, ns = _descs(model)
    if kind == "bg_actor_sample_gru":
        rc = lib.bg_actor_sample_gru(N, p(obs_store), obs_store.shape[1], model.gru_descriptor(), ns, sd, p(model.logstd), SEED, COUNTER, p(reset), p(h_in), p(h_out),
                                     p(mu), p(act), _lib.current_stream_ptr())
    else:
        td, nt = _descs(teacher)
        rc = lib.bg_distill_act_gru(N, p(obs_store), obs_store.shape[1], nt, td, P, model.gru_descriptor(), ns, sd, p(model.logstd), SEED, COUNTER, 0.0, 1, p(reset),
                                    p(h_in), p(h_out), p(mu), p(act), p(tmu), _lib.current_stream_ptr())
    _lib.check(rc, kind)
    torch.cuda.synchronize()
    for full, rows, name in ((mu_f, N, "mu"), (act_f, N, "actions")) + (((tmu_f, N, "teacher_mu"),) if teacher is not None else ()):
        _guards_untouched(full, rows, f"{kind} {name}")
    if inplace:  # the guard rows and the NaN row of the state are as they were
        assert torch.equal(h_full[:GUARD], h_store[:GUARD]) and torch.equal(h_full[GUARD + N + 1 :], h_store[GUARD + N + 1 :]) and torch.isnan(h_full[GUARD + N]).all()
        assert torch.isfinite(h_out).all()
    else:
        _guards_untouched(out_full, N, f"{kind} h_out")
    return h_out.clone(), mu.clone(), act.clone()


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("H,trunk", [(128, (256, 128, 128)), (256, (512, 128))])
def test_cell_launches_at_every_row_count(H, trunk, N):
    """H = 256 with the trunk 512-128: the 132 kB LDS form.  The observation row and the state row just past N hold NaN."""
    P = 5
    model, teacher = _student(H, P=P, trunk=trunk), _teacher(P)
    g = torch.Generator(device="cpu").manual_seed(1000 * H + N)
    obs = torch.randn(N + 1, 47 + P, generator=g).to(DEV)
    obs[N] = float("nan")
    h_store = torch.full((2 * GUARD + N + 1, H), CANARY, device=DEV)
    h_store[GUARD : GUARD + N] = (torch.randn(N, H, generator=g) * 0.5).to(DEV)
    h_store[GUARD + N] = float("nan")
    reset = (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    h0 = h_store[GUARD : GUARD + N] * (1 - reset.float()).view(N, 1)
    h_ref = _cell_f64(model.memory, obs[:N, :47], h0)[4].detach()
    mu_ref = copy.deepcopy(model.actor).double()(h_ref).detach()
    narrow = obs[:, :47].contiguous()  # (bg_actor_sample_gru on rows of its own stride 47; the distillation launch reads the teacher's rows of 52)
    narrow[N] = float("nan")
    got = {}
    for kind, rows, kw in (("bg_actor_sample_gru", narrow, {}), ("bg_distill_act_gru", obs, dict(teacher=teacher, P=P))):
        h_out, mu, act = got[kind] = _cell_launch(kind, model, rows, reset, h_store, N, **kw)
        _bound(h_out, h_ref, f"{kind} H {H} N {N} h_out")
        _bound(mu, mu_ref, f"{kind} H {H} N {N} mu")
        assert torch.isfinite(act).all()
        for x, y, k in zip(_cell_launch(kind, model, rows, reset, h_store, N, inplace=True, **kw), got[kind], ("h_out", "mu", "actions")):
            assert torch.equal(x, y), (kind, "in place against out of place", k)
    for x, y, k in zip(got["bg_actor_sample_gru"], got["bg_distill_act_gru"], ("h_out", "mu", "actions")):
        assert torch.equal(x, y), ("the student's half at beta = 0 against bg_actor_sample_gru", k)


# ------------------------------------------------------------------ 4. the rollout's cell and the update's recurrence walk the same states
@pytest.mark.parametrize("H", [128, 256])
def test_rollout_cell_and_update_recurrence_agree(H):
    """24 in-place bg_actor_sample_gru launches, each with its step's flags, against bg_mlp_layer_forward (gi on the 64-column padded rows, as
    GRUTrainer.forward computes it) + ONE bg_gru_sequence_forward: both state sequences within _bound of one float64 sequence."""
    from booster_gym_amd import _lib

    T, N, p, lib = 24, 33, _lib.ptr, _lib.load()
    model = _student(H, seed=11)
    cell = model.memory
    g = torch.Generator(device="cpu").manual_seed(77 + H)
    obs = torch.randn(T, N, 47, generator=g).to(DEV)
    h0 = (torch.randn(N, H, generator=g) * 0.5).to(DEV)
    reset = (torch.rand(T, N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    assert 0 < int(reset[0].sum()) < N and 0 < int(reset[1:].sum())
    # float64
    h, ref = h0.double(), []
    for t in range(T):
        h = _cell_f64(cell, obs[t], h * (1 - reset[t].double()).view(N, 1))[4].detach()
        ref.append(h)
    ref = torch.stack(ref)
    # the rollout: 24 launches on one state tensor, in place
    state, sd_ns, rolled = h0.clone(), _descs(model), []
    act = torch.empty(N, A, device=DEV)
    for t in range(T):
        _lib.check(lib.bg_actor_sample_gru(N, p(obs[t]), 47, model.gru_descriptor(), sd_ns[1], sd_ns[0], p(model.logstd), SEED, COUNTER + t, p(reset[t]), p(state),
                                           p(state), None, p(act), _lib.current_stream_ptr()), "bg_actor_sample_gru")
        rolled.append(state.clone())
    rolled = torch.stack(rolled)
    # the update: gi of all T N rows at once, then the recurrence as one launch
    x = torch.zeros(T * N, 64, device=DEV)
    x[:, :47] = obs.view(T * N, 47)
    w_pad = torch.zeros(3 * H, 64, device=DEV)
    w_pad[:, :47] = cell.weight_ih.detach()
    gi = torch.empty(T * N, 3 * H, device=DEV)
    _lib.check(lib.bg_mlp_layer_forward(T * N, 64, 3 * H, p(x), p(w_pad), p(cell.bias_ih), p(gi), 0, _lib.current_stream_ptr()), "bg_mlp_layer_forward")
    torch.cuda.synchronize()
    updated = _forward(T, N, H, gi.view(T, N, 3 * H), h0, reset, cell)[1]
    _bound(rolled, ref, f"H {H} the rollout's 24 states")
    _bound(updated, ref, f"H {H} the update's 24 states")
    print(f"H {H}: rollout against update, max difference {(rolled - updated).abs().max().item():.3e}; last step {(rolled[-1] - updated[-1]).abs().max().item():.3e}")
