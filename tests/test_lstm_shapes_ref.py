"""tests/parity_util.lstm_sequence_case, the reference of tests/test_gpu_lstm_shapes.py, on its own (no GPU):
  (a) its float64 loop is torch.nn.LSTMCell: the cell itself, walked in float64 with autograd on gi as its input (W_ih the identity, b_ih = 0, as
      tests/test_gpu_lstm.py does), agrees with `ref` to 1e-12 of each tensor's largest entry, resets included;
  (b) its fp32 twin stays within ONE TENTH of the project's bounds (tests/test_gpu_distill_memory._bound on forward quantities, _grad_bound on
      gradients, both unchanged) at every case and both widths of the GPU file: ten times the twin's error still passes the bound itself.  That is
      the condition under which the GPU cases use those bounds with none of their own: a kernel is left at least 10 x what fp32 arithmetic costs.
Measured here: forward quantities use at most 3.3 % of the bound (gates, 24x33, H = 256), gradients at most 0.9 % (dh0, 4x129, H = 128); at gi x 8,
T = 24, N = 33, 77.7 % of the state entries have g or f within 1e-3 of saturation, |c| stays below 5 and every twin output is finite."""
import pytest
import torch

from parity_util import LSTM_CASES, lstm_sequence_case
from test_gpu_distill_memory import _bound, _grad_bound

FORWARD, GRADS = ("h_prev", "c_prev", "h", "c", "gates"), ("dg", "dh0", "dc0")


@pytest.mark.parametrize("name, H", [("d:24x33", 128), ("f:last", 256), ("e:all_null", 128)])
def test_the_float64_loop_is_the_lstm_cell(name, H):
    T, N, scale, reset, h0, c0 = LSTM_CASES[name]
    c = lstm_sequence_case(T, N, H, scale, reset, h0, c0)
    cell = torch.nn.LSTMCell(4 * H, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(4 * H)); cell.bias_ih.zero_()
        cell.weight_hh.copy_(c["cell"].weight_hh); cell.bias_hh.copy_(c["cell"].bias_hh)
    start = lambda x: (torch.zeros(N, H) if x is None else x).double().requires_grad_()
    gi, hs, cs = c["gi"].double().requires_grad_(), start(c["h0"]), start(c["c0"])
    (h, cc), rows = (hs, cs), {k: [] for k in ("h_prev", "c_prev", "h", "c")}
    for t in range(T):
        keep = 1.0 if c["reset"] is None else (1 - c["reset"][t].double()).view(N, 1)
        hp, cp = h * keep, cc * keep
        h, cc = cell(gi[t], (hp, cp))
        for k, v in zip(rows, (hp, cp, h, cc)):
            rows[k].append(v)
    (torch.stack(rows["h"]) * c["dh_ext"].double()).sum().backward()
    got = {k: torch.stack(v).detach() for k, v in rows.items()}
    got.update(dg=gi.grad, dh0=hs.grad, dc0=cs.grad)
    if c["reset"] is not None:
        assert 0 < int(c["reset"].sum())
    for k, x in got.items():
        ref = c["ref"][k]
        err, top = (x - ref).abs().max().item(), ref.abs().max().item()
        print(f"{name} H {H} {k}: {err:.3e} of |ref|max {top:.3e}")
        assert ref.dtype == torch.float64 and err <= 1e-12 * top, (name, H, k)
    # gates = i | f | g | o | tanh(c'), the kernel's layout: the last fifth against the cell's own c', the output gate through h' = o tanh(c')
    gates = c["ref"]["gates"]
    assert tuple(gates.shape) == (T, N, 5 * H)
    assert (gates[..., 4 * H :] - torch.tanh(got["c"])).abs().max().item() <= 1e-12
    assert (gates[..., 3 * H : 4 * H] * gates[..., 4 * H :] - got["h"]).abs().max().item() <= 1e-12
    assert (gates[..., H : 2 * H] * got["c_prev"] + gates[..., :H] * gates[..., 2 * H : 3 * H] - got["c"]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("name", list(LSTM_CASES))
def test_the_twin_stays_within_a_tenth_of_the_bounds(name, H):
    T, N, scale, reset, h0, c0 = LSTM_CASES[name]
    c = lstm_sequence_case(T, N, H, scale, reset, h0, c0)
    ref, twin = c["ref"], c["twin"]
    assert all(v.dtype == torch.float64 for v in ref.values()) and all(v.dtype == torch.float32 for v in twin.values())
    tenfold = lambda k: ref[k] + 10.0 * (twin[k].double() - ref[k])
    for k in FORWARD:
        assert torch.isfinite(twin[k]).all(), (name, H, k)
        _bound(tenfold(k), ref[k], f"{name} H {H} {k}, ten times the twin's error")
    for k in GRADS:
        assert torch.isfinite(twin[k]).all(), (name, H, k)
        if ref[k].abs().max().item() == 0.0:  # (every row enters step 0 behind a reset)
            assert torch.all(twin[k] == 0.0), (name, H, k)
        else:
            _grad_bound(tenfold(k), ref[k], f"{name} H {H} {k}, ten times the twin's error")
    assert (c["h0"] is None) == (not h0) and (c["c0"] is None) == (not c0) and (c["reset"] is None) == (reset is None)
    if name == "a:1x1":
        assert int(c["reset"].sum()) == 1
    if name == "f:t0":
        assert 0 < int(c["reset"][0].sum()) < N and int(c["reset"][1:].sum()) == 0
    if name == "f:last":
        assert torch.all(c["reset"][T - 1] == 1) and int(c["reset"][: T - 1].sum()) == 0
    if name == "f:step2":
        assert torch.all(c["reset"][2] == 1) and int(c["reset"].sum()) == N
    if name == "d:24x33_scale8":
        g = ref["gates"]
        f_, g_ = g[..., H : 2 * H], g[..., 2 * H : 3 * H]
        share = ((g_.abs() > 0.999) | (f_ < 1e-3) | (f_ > 0.999)).double().mean().item()
        print(f"{name} H {H}: saturated share {share:.3f}, |c|max {ref['c'].abs().max().item():.2f}")
        assert share > 0.25


def test_two_cases_of_one_shape_share_their_draws():
    a, b = lstm_sequence_case(5, 40, 128), lstm_sequence_case(5, 40, 128, 8.0, "last", False, False)
    assert torch.equal(a["gi"] * 8.0, b["gi"]) and torch.equal(a["dh_ext"], b["dh_ext"]) and b["h0"] is None and b["c0"] is None
    c = lstm_sequence_case(5, 40, 128, reset="t0")
    assert torch.equal(c["h0"], a["h0"]) and torch.equal(c["c0"], a["c0"]) and torch.equal(c["reset"][0], a["reset"][0])
