"""The LSTM's launches at their edges, the counterpart of tests/test_gpu_gru_shapes.py: the recurrence's two launches (bg_lstm_sequence_forward /
_backward), the bias sums (bg_lstm_bias_partial) and the rollout's cell (bg_actor_sample_lstm, bg_distill_act_lstm, bg_distill_act_lstm_own) at the
shapes tests/test_gpu_lstm.py and tests/test_gpu_distill_lstm.py do not reach: one row, exact 16-row tiles, one row past a tile, an even T, the
workload's horizon of 24, saturated gates, h0 / c0 / reset NULL alone and together, dh0 / dc0 NULL in all four combinations (both NULL is the
trainer's own call), four reset patterns, both parities of the forward's LDS state tile, nine workgroups, the bias records at and around their 128-row
size, and the row counts of tests/test_gpu_actor_sample_packed.ROWS.

Reference: tests/parity_util.lstm_sequence_case, the float64 restatement of torch.nn.LSTMCell's recurrence with autograd's gradients of
sum(h * dh_ext), and an fp32 torch twin of the same loop whose error is printed beside the kernel's.  Bounds: the project's own, unchanged -- forward
quantities test_gpu_distill_memory._bound (2e-5 max(1, |ref|max)), gradients _grad_bound (1e-4 of the tensor's largest entry).
tests/test_lstm_shapes_ref.py holds the twin to a tenth of both at every case below, so no case has a bound of its own.

Every case also asserts: 16 guard rows in front of and behind every output untouched; a NaN in gi, h0, c0, dh_ext, gates and c_prev just past the
last valid row reaches no output; two calls give equal bits.  The bitwise properties (a forward launch split in time, the leading rows of a wider
launch, a backward launch cut where a reset zeroes both carries) use no bound at all.

The backward launch cannot be split in time in general: the API has dh_ext to hand carry_h over in, but no input for carry_c.  It is split where
both carries are zero: behind a step at which every env is reset ("f:step2", "f:last").

Measured on an MI355X, error / |ref|max in units of 1e-7, the fp32 twin's in brackets (dh0, dc0 "0 (0)": the case's one row enters step 0 behind a
reset).  The largest figure, 8.9 on gates at 4x129, H = 256, is 4.5 % of the bound (2e-5 max(1, |ref|max)); the largest on a gradient, 8.0, is 0.8 % of its bound:
  a:1x1              H 128  h 1.0 (1.0)  c 0.7 (0.7)  gates 0.7 (0.7)  dg 1.0 (1.7)  dh0 0 (0)  dc0 0 (0)
  a:1x1              H 256  h 0.9 (1.1)  c 0.7 (0.7)  gates 0.8 (0.8)  dg 0.5 (0.5)  dh0 0 (0)  dc0 0 (0)
  a:1x1_no_reset     H 128  h 1.9 (0.7)  c 1.0 (0.7)  gates 1.8 (0.8)  dg 1.3 (1.4)  dh0 3.5 (3.6)  dc0 1.4 (0.8)
  a:1x1_no_reset     H 256  h 2.2 (1.0)  c 1.5 (1.0)  gates 3.0 (1.1)  dg 1.6 (0.6)  dh0 4.7 (10.3)  dc0 2.4 (0.9)
  b:1x16             H 128  h 2.1 (1.9)  c 1.4 (1.2)  gates 3.4 (2.4)  dg 1.5 (1.0)  dh0 3.3 (3.4)  dc0 1.5 (1.1)
  b:1x16             H 256  h 3.0 (1.9)  c 1.8 (1.5)  gates 5.3 (3.7)  dg 3.6 (2.1)  dh0 8.0 (4.2)  dc0 2.7 (1.2)
  b:2x32             H 128  h 2.2 (1.6)  c 2.2 (1.1)  gates 4.0 (3.4)  dg 3.2 (1.8)  dh0 4.2 (3.2)  dc0 2.3 (1.1)
  b:2x32             H 256  h 3.8 (2.0)  c 2.7 (1.4)  gates 6.5 (3.2)  dg 2.8 (1.6)  dh0 8.0 (3.2)  dc0 1.5 (1.1)
  c:3x17             H 128  h 3.9 (1.6)  c 2.4 (1.3)  gates 4.4 (3.5)  dg 2.1 (1.3)  dh0 4.1 (4.4)  dc0 1.9 (1.1)
  c:3x17             H 256  h 4.4 (1.7)  c 2.7 (1.7)  gates 6.1 (3.4)  dg 2.9 (1.3)  dh0 5.5 (9.3)  dc0 2.0 (1.2)
  d:24x33            H 128  h 2.9 (2.0)  c 1.9 (1.6)  gates 4.3 (2.6)  dg 2.9 (2.0)  dh0 4.1 (3.6)  dc0 1.4 (1.2)
  d:24x33            H 256  h 4.3 (1.6)  c 2.9 (1.3)  gates 7.7 (2.6)  dg 3.9 (1.7)  dh0 5.8 (3.8)  dc0 2.1 (1.4)
  d:24x33_scale8     H 128  h 4.9 (3.3)  c 1.4 (1.3)  gates 4.9 (4.0)  dg 2.9 (2.0)  dh0 4.0 (4.8)  dc0 1.4 (1.2)
  d:24x33_scale8     H 256  h 5.1 (4.2)  c 1.6 (1.4)  gates 6.3 (4.3)  dg 3.0 (1.7)  dh0 6.0 (3.6)  dc0 1.5 (1.5)
  e:h0_null          H 128  h 2.5 (1.4)  c 2.1 (1.1)  gates 4.1 (1.6)  dg 2.9 (2.2)  dh0 3.6 (3.4)  dc0 1.9 (1.5)
  e:h0_null          H 256  h 3.5 (1.5)  c 2.4 (1.4)  gates 7.0 (1.6)  dg 5.5 (1.6)  dh0 6.7 (4.1)  dc0 1.4 (1.4)
  e:c0_null          H 128  h 2.7 (1.8)  c 2.3 (1.5)  gates 5.5 (3.0)  dg 3.4 (1.6)  dh0 4.7 (3.3)  dc0 2.5 (1.4)
  e:c0_null          H 256  h 3.7 (1.4)  c 2.7 (1.2)  gates 6.7 (2.6)  dg 3.1 (2.6)  dh0 5.3 (4.7)  dc0 3.0 (1.6)
  e:h0_c0_null       H 128  h 3.0 (1.4)  c 2.4 (1.2)  gates 3.7 (1.6)  dg 3.0 (1.4)  dh0 4.4 (3.5)  dc0 2.1 (1.6)
  e:h0_c0_null       H 256  h 3.2 (1.4)  c 2.8 (1.2)  gates 6.8 (1.6)  dg 2.9 (1.7)  dh0 6.3 (5.0)  dc0 1.6 (1.7)
  e:reset_null       H 128  h 3.3 (1.7)  c 2.1 (1.1)  gates 5.5 (3.0)  dg 3.4 (1.6)  dh0 4.4 (3.6)  dc0 1.8 (1.8)
  e:reset_null       H 256  h 3.8 (1.5)  c 2.8 (1.1)  gates 6.8 (2.6)  dg 3.3 (1.6)  dh0 6.4 (3.7)  dc0 2.8 (1.5)
  e:all_null         H 128  h 3.5 (1.4)  c 2.4 (1.4)  gates 3.8 (1.9)  dg 3.1 (2.1)  dh0 3.7 (3.3)  dc0 1.6 (1.3)
  e:all_null         H 256  h 3.2 (1.5)  c 2.8 (1.4)  gates 6.8 (1.8)  dg 2.8 (1.7)  dh0 6.3 (5.0)  dc0 1.4 (1.7)
  f:step2            H 128  h 3.3 (1.8)  c 2.1 (1.0)  gates 5.5 (3.0)  dg 3.4 (1.5)  dh0 4.4 (2.9)  dc0 1.9 (1.6)
  f:step2            H 256  h 3.8 (1.5)  c 2.8 (1.1)  gates 6.8 (2.6)  dg 2.9 (1.4)  dh0 7.7 (4.0)  dc0 1.9 (1.6)
  f:t0               H 128  h 3.2 (1.7)  c 2.1 (1.0)  gates 5.5 (3.0)  dg 3.4 (1.6)  dh0 5.2 (4.3)  dc0 1.8 (1.8)
  f:t0               H 256  h 3.8 (1.5)  c 2.8 (1.1)  gates 6.7 (2.6)  dg 3.0 (1.5)  dh0 6.4 (3.7)  dc0 2.8 (1.3)
  f:last             H 128  h 3.5 (1.8)  c 2.1 (1.1)  gates 5.5 (3.0)  dg 3.4 (1.8)  dh0 4.6 (3.0)  dc0 2.0 (1.7)
  f:last             H 256  h 3.8 (1.5)  c 2.8 (1.1)  gates 6.8 (2.6)  dg 3.9 (1.8)  dh0 5.7 (3.5)  dc0 2.1 (1.2)
  f:none             H 128  h 3.3 (1.7)  c 2.1 (1.1)  gates 5.5 (3.0)  dg 3.4 (1.6)  dh0 4.4 (3.6)  dc0 1.8 (1.8)
  f:none             H 256  h 3.8 (1.5)  c 2.8 (1.1)  gates 6.8 (2.6)  dg 3.3 (1.6)  dh0 6.4 (3.7)  dc0 2.8 (1.5)
  g:4x129            H 128  h 3.0 (2.1)  c 2.1 (1.2)  gates 5.6 (3.8)  dg 3.7 (1.3)  dh0 4.4 (3.5)  dc0 2.2 (1.5)
  g:4x129            H 256  h 4.1 (1.6)  c 3.2 (1.5)  gates 8.9 (3.1)  dg 3.6 (1.7)  dh0 8.0 (4.6)  dc0 2.3 (1.1)
At gi x 8, 78 % of the state entries have a g or f gate within 1e-3 of saturation, |c| stays below 4.8 and every output is finite.  The bias sums:
records and finished sums within 1.9e-7 of their largest entry at every B.  The cell launches at the six row counts: h' within 1.3e-7, c' within
2.3e-7 and mu within 8.2e-8 of float64 (|ref|max 0.56 / 1.8 / 0.16), the three launches equal bit for bit.  The rollout's 24 in-place cell launches
against the update's padded gi and one launch, 33 envs: the two sides differ by at most 1.5e-7 on h and 2.7e-7 on c (H = 128), 2.4e-7 and 4.0e-7
(H = 256), each within 3.6e-7 of float64.
No launch was found wrong."""
import copy
import functools
import itertools

import pytest
import torch

from parity_util import LSTM_CASES as CASES, lstm_sequence_case
from test_gpu_actor_sample_packed import ROWS
from test_gpu_distill import _descs
from test_gpu_distill_memory import A, _bound, _grad_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, CANARY = 16, 7.0
SEED, COUNTER = 987654321, 23
FORWARD, GRADS = ("h_prev", "c_prev", "h", "c", "gates"), ("dg", "dh0", "dc0")


@functools.lru_cache(maxsize=None)
def _case(T, N, H, scale=1.0, reset=0.2, h0=True, c0=True):
    return lstm_sequence_case(T, N, H, scale, reset, h0, c0, device=DEV)


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


def _forward(T, N, H, gi, h0, c0, reset, cell):
    """(h_prev, c_prev, h, c, gates) [T][N][*] of one bg_lstm_sequence_forward on contiguous gi [T][N][4H], h0 / c0 [N][H] or None, reset [T][N] or None."""
    from booster_gym_amd import _lib

    p = _lib.ptr
    gi_t, h0_t, c0_t = _nan_tailed(gi), _nan_tailed(h0), _nan_tailed(c0)
    bufs = [_guarded(T * N, w) for w in (H, H, H, H, 5 * H)]
    assert tuple(gi.shape) == (T, N, 4 * H) and (reset is None or (reset.is_contiguous() and tuple(reset.shape) == (T, N) and reset.dtype == torch.uint8))
    _lib.check(_lib.load().bg_lstm_sequence_forward(T, N, H, p(gi_t), p(h0_t), p(c0_t), p(reset), p(cell.weight_hh), p(cell.bias_hh), *[p(v) for _, v in bufs],
                                                    _lib.current_stream_ptr()), "bg_lstm_sequence_forward")
    torch.cuda.synchronize()
    for (full, _), name in zip(bufs, FORWARD):
        _guards_untouched(full, T * N, name)
    return [v.view(T, N, -1) for _, v in bufs]


def _backward(T, N, H, dh_ext, gates, c_prev, reset, cell, want_dh0=True, want_dc0=True):
    """(dg, dh0, dc0) of one bg_lstm_sequence_backward on contiguous [T][N][*] inputs; dh0 / dc0 are None where they are not requested, and their
    buffers must then keep every canary."""
    from booster_gym_amd import _lib

    p = _lib.ptr
    ins = [_nan_tailed(x) for x in (dh_ext, gates, c_prev)]
    assert tuple(dh_ext.shape) == (T, N, H) and tuple(gates.shape) == (T, N, 5 * H) and tuple(c_prev.shape) == (T, N, H)
    assert reset is None or (reset.is_contiguous() and tuple(reset.shape) == (T, N) and reset.dtype == torch.uint8)
    (dg_f, dg), (dh0_f, dh0), (dc0_f, dc0) = _guarded(T * N, 4 * H), _guarded(N, H), _guarded(N, H)
    _lib.check(_lib.load().bg_lstm_sequence_backward(T, N, H, *[p(x) for x in ins], p(reset), p(cell.weight_hh), p(dg), p(dh0) if want_dh0 else None,
                                                     p(dc0) if want_dc0 else None, _lib.current_stream_ptr()), "bg_lstm_sequence_backward")
    torch.cuda.synchronize()
    _guards_untouched(dg_f, T * N, "dg")
    for full, want, name in ((dh0_f, want_dh0, "dh0"), (dc0_f, want_dc0, "dc0")):
        if want:
            _guards_untouched(full, N, name)
        else:
            assert torch.all(full == CANARY), f"{name} was written though not requested"
    return dg.view(T, N, -1), dh0 if want_dh0 else None, dc0 if want_dc0 else None


def _rel(x, ref):
    return (x.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _check_forward(x, c, name, what):
    print(f"{what} {name}: the fp32 twin's error {_rel(c['twin'][name], c['ref'][name]):.3e} of |ref|max")
    _bound(x, c["ref"][name], f"{what} {name}")


def _check_gradient(x, c, name, what):
    ref = c["ref"][name]
    print(f"{what} {name}: the fp32 twin's error {_rel(c['twin'][name], ref):.3e} of |ref|max")
    if ref.abs().max().item() == 0.0:  # (one row that enters step 0 behind a reset: dh0 and dc0 are exactly zero)
        assert torch.all(x == 0.0), f"{what} {name}"
    else:
        _grad_bound(x, ref, f"{what} {name}")


def _cut(x, a, b):
    return None if x is None else x[a:b].contiguous()


# ------------------------------------------------------------------ 1. the cases a .. g
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("name", list(CASES))
def test_sequence_launches_match_float64(name, H):
    T, N, scale, reset, h0, c0 = CASES[name]
    c = _case(T, N, H, scale, reset, h0, c0)
    cell, what, flags, dh_ext = c["cell"], f"{name} H {H}", c["reset"], c["dh_ext"]
    fwd = lambda: _forward(T, N, H, c["gi"], c["h0"], c["c0"], flags, cell)
    h_prev, c_prev, h, cc, gates = out = fwd()
    for x, k in zip(out, FORWARD):
        assert torch.isfinite(x).all(), (what, k)
        _check_forward(x, c, k, what)
    for x, y, k in zip(out, fwd(), FORWARD):
        assert torch.equal(x, y), ("two forward calls differ", k)
    bwd = lambda **kw: _backward(T, N, H, dh_ext, gates, c_prev, flags, cell, **kw)
    dg, dh0, dc0 = grads = bwd()
    for x, k in zip(grads, GRADS):
        assert torch.isfinite(x).all(), (what, k)
        _check_gradient(x, c, k, what)
    for x, y, k in zip(grads, bwd(), GRADS):
        assert torch.equal(x, y), ("two backward calls differ", k)
    print("TABLE  %-18s H %d  " % (name, H) + "  ".join(f"{k} {1e7 * _rel(x, c['ref'][k]):.1f} ({1e7 * _rel(c['twin'][k], c['ref'][k]):.1f})"
                                                      for k, x in (("h", h), ("c", cc), ("gates", gates), ("dg", dg), ("dh0", dh0), ("dc0", dc0))))
    # the states entering a step: zero behind a reset, else h0 / c0 or the step before, bit for bit
    on = torch.zeros(T, N, dtype=torch.bool, device=DEV) if flags is None else flags.bool()
    for prev, new, start, k in ((h_prev, h, c["h0"], "h_prev"), (c_prev, cc, c["c0"], "c_prev")):
        first = torch.zeros(N, H, device=DEV) if start is None else start
        entering = torch.cat((first.view(1, N, H), new[:-1]))
        assert torch.all(prev[on] == 0.0) and torch.equal(prev[~on], entering[~on]), (what, k)
    # dh0 / dc0 NULL in all four combinations (both NULL: LSTMTrainer.backward's call): dg does not depend on them, what is requested neither
    for want_dh0, want_dc0 in itertools.product((True, False), repeat=2):
        got = bwd(want_dh0=want_dh0, want_dc0=want_dc0)
        assert torch.equal(got[0], dg), (what, "dg with dh0 / dc0 requested:", want_dh0, want_dc0)
        assert (got[1] is None) == (not want_dh0) and (got[2] is None) == (not want_dc0)
        assert (got[1] is None or torch.equal(got[1], dh0)) and (got[2] is None or torch.equal(got[2], dc0)), (what, want_dh0, want_dc0)
    if name == "a:1x1":
        assert int(flags.sum()) == 1 and torch.all(dh0 == 0.0) and torch.all(dc0 == 0.0)
    if name == "d:24x33_scale8":  # a large share of the gates is saturated: 1 - tc tc, f (1 - f) and 1 - g g vanish in fp32
        f, g = gates[..., H : 2 * H], gates[..., 2 * H : 3 * H]
        share = ((g.abs() > 0.999) | (f < 1e-3) | (f > 0.999)).float().mean().item()
        print(f"{what}: state entries whose g or f gate is within 1e-3 of saturation: {share:.3f}; |c|max {cc.abs().max().item():.2f}")
        assert share > 0.25  # (gi_g ~ N(0, 8^2): |tanh| > 0.999 beyond |x| = 3.8, a share of 0.63 of the draws on g alone)
    if name.startswith("e:"):
        # NULL is a zero tensor: bit for bit, forward and backward
        zero = lambda x, *shape, **kw: torch.zeros(*shape, device=DEV, **kw) if x is None else x
        z_h0, z_c0, z_reset = zero(c["h0"], N, H), zero(c["c0"], N, H), zero(flags, T, N, dtype=torch.uint8)
        assert c["h0"] is None or c["c0"] is None or flags is None
        for x, y, k in zip(out, _forward(T, N, H, c["gi"], z_h0, z_c0, z_reset, cell), FORWARD):
            assert torch.equal(x, y), (what, "NULL against a zero tensor", k)
        for x, y, k in zip(grads, _backward(T, N, H, dh_ext, gates, c_prev, z_reset, cell), GRADS):
            assert torch.equal(x, y), (what, "reset NULL against a zero tensor, backward", k)
        if c["h0"] is None and c["c0"] is not None:  # (a NULL h0 is not c0, a NULL c0 is not h0: the two states start apart)
            assert torch.all(h_prev[0] == 0.0) and c_prev[0].abs().max().item() > 0
        if c["c0"] is None and c["h0"] is not None:
            assert torch.all(c_prev[0] == 0.0) and h_prev[0].abs().max().item() > 0
    if name in ("f:step2", "f:last"):
        # every env is reset at step `cut`: both carries leaving it are zero, so the steps below it are those of a launch that ends there (dh0 and dc0
        # with them), and the steps from it on are those of a launch of their own, which leaves nothing behind
        cut = 2 if name == "f:step2" else T - 1
        assert torch.all(flags[cut] == 1) and int(flags.sum()) == N and torch.all(h_prev[cut] == 0.0) and torch.all(c_prev[cut] == 0.0)
        head = _backward(cut, N, H, *[_cut(x, 0, cut) for x in (dh_ext, gates, c_prev, flags)], cell)
        tail = _backward(T - cut, N, H, *[_cut(x, cut, T) for x in (dh_ext, gates, c_prev, flags)], cell)
        assert torch.equal(head[0], dg[:cut]) and torch.equal(head[1], dh0) and torch.equal(head[2], dc0), (what, "the steps below the reset")
        assert torch.equal(tail[0], dg[cut:]) and torch.all(tail[1] == 0.0) and torch.all(tail[2] == 0.0), (what, "the steps from the reset on")
        assert dh0.abs().max().item() > 0 and dc0.abs().max().item() > 0 and dg[cut:].abs().max().item() > 0
        # (the cut is not vacuous: with the flags taken away, the steps below it do receive something from above)
        free = _backward(T, N, H, dh_ext, gates, c_prev, None, cell)
        assert not torch.equal(free[0][:cut], dg[:cut])
    if name == "f:t0":
        on0 = flags[0].bool()
        assert 0 < int(on0.sum()) < N and int(flags[1:].sum()) == 0
        for x, k in ((dh0, "dh0"), (dc0, "dc0")):
            assert torch.all(x[on0] == 0.0) and torch.all((x[~on0] != 0.0).any(-1)), (what, k)


# ------------------------------------------------------------------ 2. bitwise: a forward launch split in time, the leading rows of a wider launch
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("T1", [1, 2, 4])
def test_a_forward_launch_split_in_time_reproduces_the_single_launch(T1, H):
    """An odd T1 starts the second launch on the LDS tile the single launch reads on even steps; c enters it from memory instead of the registers."""
    T, N = 5, 40
    c = _case(T, N, H)
    cell, gi, reset = c["cell"], c["gi"], c["reset"]
    assert 0 < int(reset[:T1].sum()) and 0 < int(reset[T1:].sum()) < (T - T1) * N
    whole = _forward(T, N, H, gi, c["h0"], c["c0"], reset, cell)
    first = _forward(T1, N, H, _cut(gi, 0, T1), c["h0"], c["c0"], _cut(reset, 0, T1), cell)
    second = _forward(T - T1, N, H, _cut(gi, T1, T), first[2][T1 - 1].contiguous(), first[3][T1 - 1].contiguous(), _cut(reset, T1, T), cell)
    for a, b, w, k in zip(first, second, whole, FORWARD):
        assert torch.equal(torch.cat((a, b)), w), ("forward", T1, k)


@pytest.mark.parametrize("H", [128, 256])
def test_the_leading_rows_of_a_wider_launch_are_the_narrow_launch(H):
    """17 of 48 rows: the second workgroup's one valid row and 15 tail rows against a full tile of the same workgroup."""
    T, N, M = 5, 48, 17
    c = _case(T, N, H)
    cell = c["cell"]
    cut = lambda x: x[:, :M].contiguous()
    wide = _forward(T, N, H, c["gi"], c["h0"], c["c0"], c["reset"], cell)
    narrow = _forward(T, M, H, cut(c["gi"]), c["h0"][:M].contiguous(), c["c0"][:M].contiguous(), cut(c["reset"]), cell)
    for a, b, k in zip(narrow, wide, FORWARD):
        assert torch.equal(a, cut(b)), ("forward", k)
    wide_g = _backward(T, N, H, c["dh_ext"], wide[4], wide[1], c["reset"], cell)
    narrow_g = _backward(T, M, H, cut(c["dh_ext"]), narrow[4], narrow[1], cut(c["reset"]), cell)
    assert torch.equal(narrow_g[0], cut(wide_g[0])) and torch.equal(narrow_g[1], wide_g[1][:M]) and torch.equal(narrow_g[2], wide_g[2][:M])
    assert narrow_g[1].abs().max().item() > 0 and narrow_g[2].abs().max().item() > 0


# ------------------------------------------------------------------ 3. the bias sums
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("B", [1, 3, 127, 128, 129, 257, 516])
def test_bias_partial_at_and_around_its_record_size(B, H):
    """A record holds 128 rows, four waves stride them by 4 (unrolled by 4): B = 3 and 129 leave waves without a row, 127 and 257 blocks whose row count
    is no multiple of 4, 128 the exact record, 516 = 4 x 129 case g's batch.  The row behind B is NaN: a record that reads on to the end of its block
    turns NaN."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import reduce_group

    lib, p, st, nb, C = _lib.load(), _lib.ptr, _lib.current_stream_ptr(), (B + 127) // 128, 4 * H
    g = torch.Generator(device="cpu").manual_seed(7000 + 10 * B + H)
    dg = _nan_tailed(torch.randn(B, C, generator=g).to(DEV))
    ref = dg[:B].double()
    blocks = torch.stack([ref[128 * k : min(128 * k + 128, B)].sum(0) for k in range(nb)])

    def run():
        (rec_f, rec), sums = _guarded(nb, C), [_guarded(1, C) for _ in range(2)]
        _lib.check(lib.bg_lstm_bias_partial(B, H, p(dg), p(rec), st), "bg_lstm_bias_partial")
        fins = []
        for _, s in sums:  # the two finishes on the same records: b_ih's and b_hh's gradients
            fin = _lib.ReduceProblem()
            fin.partial, fin.groups, fin.record, fin.n_out, fin.out[0], fin.n[0] = rec.data_ptr(), nb, C, C, s.data_ptr(), C
            fins.append(fin)
        reduce_group(fins)
        torch.cuda.synchronize()
        _guards_untouched(rec_f, nb, "records")
        for full, _ in sums:
            _guards_untouched(full, 1, "a finished sum")
        return rec, sums[0][1][0], sums[1][1][0]

    rec, s_ih, s_hh = run()
    assert torch.isfinite(rec).all() and torch.isfinite(s_ih).all() and torch.isfinite(s_hh).all()
    for k in range(nb):
        _grad_bound(rec[k], blocks[k], f"B {B} H {H} record {k}")
    for s, k in ((s_ih, "b_ih"), (s_hh, "b_hh")):
        _grad_bound(s, ref.sum(0), f"B {B} H {H} the finished sum of {k}")
    assert torch.equal(s_ih, s_hh), "the two finishes differ"
    for x, y in zip((rec, s_ih, s_hh), run()):
        assert torch.equal(x, y), "two calls differ"


# ------------------------------------------------------------------ 4. the rollout's cell launches
def _lstm_model(H, trunk=(256, 128, 128), P=0, seed=5):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(seed)
    m = ActorCritic(A, 47, 14 + P, trunk, memory_hidden=H, memory_cell="lstm").to(DEV)
    with torch.no_grad():
        m.logstd.copy_(torch.linspace(-2.5, 0.5, A, device=DEV).view(1, A))
    return m


def _teacher(P, hidden=(256, 128, 128)):
    from booster_gym_amd.utils.model import ActorCritic

    torch.manual_seed(9)
    return ActorCritic(A, 47 + P, 14 + P, hidden).to(DEV)


def _state_stores(h, c):
    """The states h, c [N][H] in the two layouts of the launches, canaries round them and one NaN row at N:
      two  [2][GUARD + N + 1 + GUARD][H]  bg_actor_sample_lstm's two pointers, each half with its own guards and NaN row;
      one  [GUARD + 2 N + 1 + GUARD][H]   the distillation launches' ONE tensor [2][N][H] from one pointer: guard rows in front of the h half, the NaN
                                          row and guard rows behind the c half (row N of h is row 0 of c)."""
    N, H = h.shape
    two = torch.full((2, 2 * GUARD + N + 1, H), CANARY, device=DEV)
    two[0, GUARD : GUARD + N], two[1, GUARD : GUARD + N] = h, c
    two[:, GUARD + N] = float("nan")
    one = torch.full((2 * GUARD + 2 * N + 1, H), CANARY, device=DEV)
    one[GUARD : GUARD + N], one[GUARD + N : GUARD + 2 * N] = h, c
    one[GUARD + 2 * N] = float("nan")
    return two, one


def _cell_launch(kind, model, reset, stores, N, inplace, obs=None, teacher=None, tobs=None, P=0):
    """One launch of `kind` on the first N rows.  obs: the rows of the cell's 47 inputs (bg_actor_sample_lstm, bg_distill_act_lstm_own); tobs: the
    teacher's rows.  Returns (h', c', mu, actions) [N][*]; every output's guard rows are checked on both sides; in place, the state stores' guard and
    NaN rows must be as they were."""
    from booster_gym_amd import _lib

    H, p, lib, st = model.memory_hidden, _lib.ptr, _lib.load(), _lib.current_stream_ptr()
    (mu_f, mu), (act_f, act), (tmu_f, tmu) = _guarded(N, A), _guarded(N, A), _guarded(N, A)
    sd, ns = _descs(model)
    cell = model.gru_descriptor()
    if kind == "bg_actor_sample_lstm":
        src = stores[0].clone()
        h_in, c_in = src[0, GUARD : GUARD + N], src[1, GUARD : GUARD + N]
        if inplace:
            h_out, c_out = h_in, c_in
        else:
            (ho_f, h_out), (co_f, c_out) = _guarded(N, H), _guarded(N, H)
        rc = lib.bg_actor_sample_lstm(N, p(obs), obs.shape[1], cell, ns, sd, p(model.logstd), SEED, COUNTER, p(reset), p(h_in), p(h_out), p(c_in), p(c_out), p(mu),
                                      p(act), st)
    else:
        src = stores[1].clone()
        s_in = src[GUARD : GUARD + 2 * N]
        if inplace:
            s_out = s_in
        else:
            so_f, s_out = _guarded(2 * N, H)
        td, nt = _descs(teacher)
        mid = (p(obs), obs.shape[1]) if kind == "bg_distill_act_lstm_own" else ()
        rc = getattr(lib, kind)(N, p(tobs), tobs.shape[1], *mid, nt, td, P, cell, ns, sd, p(model.logstd), SEED, COUNTER, 0.0, 1, p(reset), p(s_in), p(s_out), p(mu),
                                p(act), p(tmu), st)
        h_out, c_out = s_out[:N], s_out[N:]
    _lib.check(rc, kind)
    torch.cuda.synchronize()
    for full, name in ((mu_f, "mu"), (act_f, "actions")) + (((tmu_f, "teacher_mu"),) if teacher is not None else ()):
        _guards_untouched(full, N, f"{kind} {name}")
    if inplace:
        nan_row = GUARD + (N if kind == "bg_actor_sample_lstm" else 2 * N)
        assert torch.all(src[..., :GUARD, :] == CANARY) and torch.all(src[..., nan_row + 1 :, :] == CANARY) and torch.isnan(src[..., nan_row, :]).all(), \
            f"{kind}: rows round the state were written"
    elif kind == "bg_actor_sample_lstm":
        _guards_untouched(ho_f, N, f"{kind} h_out")
        _guards_untouched(co_f, N, f"{kind} c_out")
    else:
        _guards_untouched(so_f, 2 * N, f"{kind} state_out")
    assert torch.isfinite(h_out).all() and torch.isfinite(c_out).all(), f"{kind}: a value past the last valid row reached the state"
    return h_out.clone(), c_out.clone(), mu.clone(), act.clone()


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("H,trunk", [(128, (256, 128, 128)), (256, (512, 128))])
def test_cell_launches_at_every_row_count(H, trunk, N):
    """The three launches on one cell, one trunk and the same rows: bg_actor_sample_lstm on rows of stride 47, bg_distill_act_lstm (beta = 0) on the
    teacher's rows of stride 52, bg_distill_act_lstm_own on a student buffer of stride 50.  The observation row and the state row just past N hold NaN."""
    P = 5
    model, teacher = _lstm_model(H, trunk, P), _teacher(P)
    g = torch.Generator(device="cpu").manual_seed(1000 * H + N)
    tobs = torch.randn(N + 1, 47 + P, generator=g).to(DEV)
    tobs[N] = float("nan")
    narrow, own = tobs[:, :47].contiguous(), torch.randn(N + 1, 50, generator=g).to(DEV)
    own[:, :47] = narrow  # (row N: NaN with it)
    h, c = (torch.randn(N, H, generator=g) * 0.5).to(DEV), (torch.randn(N, H, generator=g) * 0.5).to(DEV)
    stores = _state_stores(h, c)
    reset = (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    keep = (1 - reset.double()).view(N, 1)
    with torch.no_grad():
        h_ref, c_ref = copy.deepcopy(model.memory).double()(narrow[:N].double(), (h.double() * keep, c.double() * keep))
        mu_ref = copy.deepcopy(model.actor).double()(h_ref)
    got = {}
    for kind, kw in (("bg_actor_sample_lstm", dict(obs=narrow)), ("bg_distill_act_lstm", dict(teacher=teacher, tobs=tobs, P=P)),
                     ("bg_distill_act_lstm_own", dict(obs=own, teacher=teacher, tobs=tobs, P=P))):
        h_out, c_out, mu, act = got[kind] = _cell_launch(kind, model, reset, stores, N, False, **kw)
        _bound(h_out, h_ref, f"{kind} H {H} N {N} h'")
        _bound(c_out, c_ref, f"{kind} H {H} N {N} c'")
        _bound(mu, mu_ref, f"{kind} H {H} N {N} mu")
        assert torch.isfinite(act).all() and not torch.equal(act, mu)
        for x, y, k in zip(_cell_launch(kind, model, reset, stores, N, True, **kw), got[kind], ("h'", "c'", "mu", "actions")):
            assert torch.equal(x, y), (kind, "in place against out of place", k)
    for kind in ("bg_distill_act_lstm", "bg_distill_act_lstm_own"):
        for x, y, k in zip(got["bg_actor_sample_lstm"], got[kind], ("h'", "c'", "mu", "actions")):
            assert torch.equal(x, y), (f"{kind} at beta = 0 against bg_actor_sample_lstm", k)


# ------------------------------------------------------------------ 5. the rollout's cell and the update's recurrence walk the same states
@pytest.mark.parametrize("H", [128, 256])
def test_rollout_cell_and_update_recurrence_agree(H):
    """24 in-place bg_actor_sample_lstm launches, each with its step's flags, against bg_mlp_layer_forward (gi on the 64-column padded rows and padded
    W_ih, as LSTMTrainer.forward computes it) + ONE bg_lstm_sequence_forward: both h and c sequences within _bound of one float64 walk."""
    from booster_gym_amd import _lib

    T, N, p, lib = 24, 33, _lib.ptr, _lib.load()
    model = _lstm_model(H, seed=11)
    cell = model.memory
    g = torch.Generator(device="cpu").manual_seed(77 + H)
    obs = torch.randn(T, N, 47, generator=g).to(DEV)
    state0 = (torch.randn(2, N, H, generator=g) * 0.5).to(DEV)
    reset = (torch.rand(T, N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    assert 0 < int(reset[0].sum()) < N and 0 < int(reset[1:].sum())
    # float64
    cell64, (h, c), ref_h, ref_c = copy.deepcopy(cell).double(), state0.double(), [], []
    with torch.no_grad():
        for t in range(T):
            keep = (1 - reset[t].double()).view(N, 1)
            h, c = cell64(obs[t].double(), (h * keep, c * keep))
            ref_h.append(h); ref_c.append(c)
    ref_h, ref_c = torch.stack(ref_h), torch.stack(ref_c)
    # the rollout: 24 launches on one state tensor, in place
    state, (sd, ns), rolled_h, rolled_c = state0.clone(), _descs(model), [], []
    act = torch.empty(N, A, device=DEV)
    for t in range(T):
        _lib.check(lib.bg_actor_sample_lstm(N, p(obs[t]), 47, model.gru_descriptor(), ns, sd, p(model.logstd), SEED, COUNTER + t, p(reset[t]), p(state[0]), p(state[0]),
                                            p(state[1]), p(state[1]), None, p(act), _lib.current_stream_ptr()), "bg_actor_sample_lstm")
        rolled_h.append(state[0].clone()); rolled_c.append(state[1].clone())
    rolled_h, rolled_c = torch.stack(rolled_h), torch.stack(rolled_c)
    # the update: gi of all T N rows at once, then the recurrence as one launch
    x = torch.zeros(T * N, 64, device=DEV)
    x[:, :47] = obs.view(T * N, 47)
    w_pad = torch.zeros(4 * H, 64, device=DEV)
    w_pad[:, :47] = cell.weight_ih.detach()
    gi = torch.empty(T * N, 4 * H, device=DEV)
    _lib.check(lib.bg_mlp_layer_forward(T * N, 64, 4 * H, p(x), p(w_pad), p(cell.bias_ih), p(gi), 0, _lib.current_stream_ptr()), "bg_mlp_layer_forward")
    torch.cuda.synchronize()
    _, _, upd_h, upd_c, _ = _forward(T, N, H, gi.view(T, N, 4 * H), state0[0], state0[1], reset, cell)
    _bound(rolled_h, ref_h, f"H {H} the rollout's 24 h")
    _bound(rolled_c, ref_c, f"H {H} the rollout's 24 c")
    _bound(upd_h, ref_h, f"H {H} the update's 24 h")
    _bound(upd_c, ref_c, f"H {H} the update's 24 c")
    print(f"H {H}: rollout against update, max difference h {(rolled_h - upd_h).abs().max().item():.3e}, c {(rolled_c - upd_c).abs().max().item():.3e}; "
          f"last step h {(rolled_h[-1] - upd_h[-1]).abs().max().item():.3e}, c {(rolled_c[-1] - upd_c[-1]).abs().max().item():.3e}")
