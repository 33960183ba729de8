"""Every update-path entry point held to the buffer extents include/booster_gym_amd.h documents for it ("Buffer extents").

Each case puts EVERY buffer of a call into a guarded window (tests/extent_util.py): one allocation whose bytes around the window hold a poison pattern,
the window itself placed 16 bytes past a 256-byte boundary where the header promises 16-byte alignment and 4 bytes (the element size, for float64) past it
where the header promises nothing.  Scratch buffers have exactly the number of elements the header states, written as the header's expression.  The
library is called through _lib.load(): no wrapper allocates on its own.  Each case asserts
  (a) the values against a float64 torch evaluation of the same operation on the same inputs, at the tolerance the family's own test file states:
      2e-5 x max(1, |ref|max) for layer outputs (test_gpu_mlp.py, test_gpu_mlp_chain_split.py, test_gpu_head.py), 1e-4 of the largest entry for sums over
      rows (test_gpu_head.py), bit for bit where the header says so;
  (b) that no band byte changed, and that outputs the header documents as written in full are written in full;
  (c) where the header says rows at or beyond M do not enter the results: the same bits with the inputs' pad rows at 0 and at 1e30;
  (d) that scratch documented as "left zero" is zero afterwards.
No call gives a kernel less memory than its header extent: every pointer points into an arena this process owns, with the header's full extent behind it
and a band of at least one more unit (a 128-row slab, a record, a slice) behind that.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import extent_util as X
from test_action_noise_ref import action_noise
from test_gpu_action_noise import _bound as noise_bound
from test_mini_batches import host_perm, perm_lib  # noqa: F401  (perm_lib: the fixture that compiles csrc/bg_perm.h for the host)
from test_smoothness import partner_draw

pytestmark = pytest.mark.gpu
DEV = X.DEV
F32, F64, I16, I32, U8 = torch.float32, torch.float64, torch.int16, torch.int32, torch.uint8

ROWS_ANY = [1, 31, 128, 129, 1025]   # any M >= 1: one row, below / at / above a 128-row slab, 9 slabs = one XCD group of 8 plus one
ROWS_EVEN = [64, 130, 1026]          # M even with slices * 8 <= M (bg_mlp_weight_grad and its grouped forms)
ROWS_32 = [32, 160, 1056]            # M a multiple of 32 (the split weight gradients)
ACTOR, CRITIC = (64, 256, 128, 128), (64, 256, 256, 128)   # (K0 padded, N1, N2, N3); the first layers' real inputs: 47 and 61
K_REAL = {ACTOR: 47, CRITIC: 61}


def _L():
    from booster_gym_amd import _lib

    return _lib


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    """the entry point on torch's current stream; a refusal is an error"""
    L = _L()
    L.check(getattr(L.load(), name)(*args, L.current_stream_ptr()), name)


def slabs(M):
    return (M + 127) // 128


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def elu(x):
    return torch.nn.functional.elu(x)


def elup(a):
    """elu'(z) through the layer's output a = elu(z)"""
    return torch.where(a > 0, torch.ones_like(a), a + 1.0)


def weight(g, n, k_real, k=None):
    """W [n][k] with the columns at or beyond k_real zero and two asymmetric entries (a transposed / permuted fragment map cannot pass)"""
    k = k or k_real
    w = torch.zeros(n, k)
    w[:, :k_real] = torch.randn(n, k_real, generator=g) / k_real**0.5
    w[3, 5] = 3.0
    w[n - 1, 0] = -2.0
    return w.to(DEV)


def close(got, ref, rel, what):
    """|got - ref|max <= rel x max(1, |ref|max) over EVERY element of the documented shape"""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    err, scale = (got.double() - ref.double()).abs().max().item(), max(1.0, ref.double().abs().max().item())
    print(f"{what}: {got.numel()} elements, max error {err:.3e}, bound {rel * scale:.3e}")
    assert err <= rel * scale, (what, err, rel * scale)


def unpack_planes(pl, n_out, k_out):
    """planes [n][k / 32][3][32] bf16 in the kernels' k order -> (hi, mid, lo) float64 [n][k]"""
    raw = pl.cpu().numpy().view(np.uint16).reshape(n_out, k_out // 32, 3, 32)
    f = (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    k = np.arange(32)
    s, h, q = k >> 3, (k >> 2) & 1, k & 3
    pos = (s >> 1) * 16 + h * 8 + (s & 1) * 4 + q
    return [f[:, :, i, :][:, :, pos].reshape(n_out, k_out) for i in range(3)]


def planes(ws, name, w, n_out, k_out, transpose=0, pm=False):
    """the planes of w (and of -w) in a window of exactly the header's size: n_out * k_out * 3 uint16 (x 2 for _pm), 16-byte aligned"""
    n = n_out * k_out * 3 * (2 if pm else 1)
    out = ws.out(name, (n,), I16, skew=16, band=max(X.MIN_BAND, k_out * 6))  # one more row of planes is k_out x 6 bytes
    src = ws.inp(name + ".src", w, skew=4)                                    # (W: no alignment promised, element loads)
    call("bg_mlp_split_weights_pm" if pm else "bg_mlp_split_weights", n_out, k_out, p(src), w.shape[1], w.shape[0], w.shape[1], transpose, p(out))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- layer forward
LAYERS_FWD = [(64, 256, 47), (64, 256, 61), (256, 128, 256), (256, 256, 256), (128, 128, 128), (512, 128, 512), (128, 512, 128)]


@pytest.mark.parametrize("K,N,k_real", LAYERS_FWD)
@pytest.mark.parametrize("M", ROWS_ANY)
def test_layer_forward_writes_exactly_M_rows(M, K, N, k_real):
    """bg_mlp_layer_forward and bg_mlp_layer_forward_split (terms 6, 9), with and without the ELU: "Y [M][N]", "Exactly the M rows of Y are written".  (The
    same sentence's "rows of X at or beyond M are never read" is true by the kernels' row clamp and is NOT pinned here: a row of X feeds only its own row
    of Y, so a read behind row M could only reach rows of Y that are not stored.  X holds exactly M rows with one more slab of owned memory behind.)"""
    g = gen(M + K + N + k_real)
    x = torch.zeros(M, K)
    x[:, :k_real] = torch.randn(M, k_real, generator=g)
    w, b = weight(g, N, k_real, K), randn(g, N, scale=0.3)
    lin = x.to(DEV).double() @ w.double().t() + b.double()
    slab = 128 * N * 4  # one more slab of Y
    forms = [("bg_mlp_layer_forward", None)] + ([("bg_mlp_layer_forward_split", 9), ("bg_mlp_layer_forward_split", 6)] if K <= 256 else [])
    for (name, terms), act in ((f, a) for f in forms for a in (1, 0)):
        ref = elu(lin) if act else lin
        ws = X.Windows()
        xw, bw = ws.inp("X", x.to(DEV)), ws.inp("bias", b)
        y = ws.out("Y", (M, N), band=slab)
        if terms is None:
            call(name, M, K, N, p(xw), p(ws.inp("W", w)), p(bw), p(y), act)
        else:
            call(name, M, K, N, p(xw), p(planes(ws, "planes", w[:, :k_real].contiguous(), N, K)), p(bw), p(y), act, terms)
        ws.check(f"{name} terms={terms} elu={act}")
        X.assert_fully_written(y, f"{name}: Y")
        close(y, ref, 2e-5, f"{name} terms={terms} elu={act} M={M} K={K} N={N}")


def test_layer_forward_refuses_a_bias_that_is_not_16_byte_aligned():
    """"X, W, bias and Y 16-byte aligned (-1 otherwise)": the epilogue loads the bias 16 bytes at a time.  Refused before any launch: Y stays poison."""
    L = _L()
    lib, st = L.load(), L.current_stream_ptr()
    g = gen(1)
    ws = X.Windows()
    x, w, y = ws.inp("X", randn(g, 4, 128)), weight(g, 128, 128), ws.out("Y", (4, 128))
    for skew in (4, 8):
        b = ws.inp(f"bias at {skew}", randn(g, 128), skew=skew)
        assert lib.bg_mlp_layer_forward(4, 128, 128, p(x), p(ws.inp("W", w)), p(b), p(y), 1, st) == -1 and b"aligned" in lib.bg_last_error()
        assert lib.bg_mlp_layer_forward_split(4, 128, 128, p(x), p(planes(ws, "planes", w, 128, 128)), p(b), p(y), 1, 9, st) == -1 and b"aligned" in lib.bg_last_error()
    ws.check("refused layer forward")
    assert bool(X.is_poison(y).all())


# ---------------------------------------------------------------------------------------------------------------------------- layer backward
LAYERS_BWD = [(128, 128), (128, 256), (256, 256), (256, 128), (512, 128), (128, 512)]  # (K = width above, N = width below)


@pytest.mark.parametrize("K,N", LAYERS_BWD)
@pytest.mark.parametrize("M", ROWS_ANY)
def test_layer_backward_scratch_and_outputs(M, K, N):
    """bg_mlp_layer_backward, _partial, _split: "Gout [M][N]", "scratch: ceil(M/128) * N floats", "bias_grad_below [N]"; the _partial form leaves
    bias_grad_below untouched until bg_reduce_group runs its descriptor."""
    L = _L()
    g = gen(M + 3 * K + N)
    G, W = randn(g, M, K), weight(g, K, N)  # W [K][N] in torch's layout (out = K, in = N); the kernel takes W^T [N][K]
    act = elu(randn(g, M, N))
    ref = (G.double() @ W.double()) * elup(act).double()
    cs = ref.sum(0)
    wt = W.t().contiguous()
    slab = 128 * N * 4
    for name, terms in [("bg_mlp_layer_backward", None), ("bg_mlp_layer_backward_partial", None)] + ([("bg_mlp_layer_backward_split", 9), ("bg_mlp_layer_backward_split", 6)] if K <= 256 else []):
        ws = X.Windows()
        Gw, aw = ws.inp("G", G), ws.inp("act_below", act)
        out = ws.out("Gout", (M, N), band=slab)
        bg = ws.out("bias_grad_below", (N,), skew=4)
        scratch = ws.out("scratch", (slabs(M) * N,), skew=4, band=N * 4)  # header: ceil(M/128) * N floats; one more record is N floats
        if terms is not None:
            call(name, M, K, N, p(Gw), p(planes(ws, "planes_t", W, N, K, transpose=1)), p(aw), p(out), p(bg), p(scratch), terms)
        elif name.endswith("_partial"):
            fin = L.ReduceProblem()
            call(name, M, K, N, p(Gw), p(ws.inp("Wt", wt)), p(aw), p(out), p(bg), p(scratch), C.byref(fin))
            torch.cuda.synchronize()
            assert bool(X.is_poison(bg).all()), "bg_mlp_layer_backward_partial wrote bias_grad_below before bg_reduce_group"
            assert (fin.groups, fin.record, fin.n_out) == (slabs(M), N, N)  # the records the descriptor names are the header's scratch, no more
            call("bg_reduce_group", (L.ReduceProblem * 1)(fin), 1)
        else:
            call(name, M, K, N, p(Gw), p(ws.inp("Wt", wt)), p(aw), p(out), p(bg), p(scratch))
        ws.check(f"{name} terms={terms}")
        X.assert_fully_written(out, f"{name}: Gout")
        X.assert_fully_written(bg, f"{name}: bias_grad_below")
        X.assert_fully_written(scratch, f"{name}: scratch")  # one record per slab: all of the header's extent is used, none behind it (bands)
        close(out, ref, 2e-5, f"{name} terms={terms} Gout M={M} K={K} N={N}")
        # sums over rows: 1e-4 of the largest entry (test_gpu_head.py)
        close(bg, cs, 1e-4, f"{name} terms={terms} bias_grad_below")


# ---------------------------------------------------------------------------------------------------------------------------- forward chains
def chain_inputs(M, dims, seed, x_rows=None):
    K0, N1, N2, N3 = dims
    g = gen(seed)
    x = torch.zeros(M, K0)
    x[:, : K_REAL[dims]] = torch.randn(M, K_REAL[dims], generator=g)
    Ws = [weight(g, N1, K_REAL[dims], K0), weight(g, N2, N1), weight(g, N3, N2)]
    bs = [randn(g, n, scale=0.3) for n in (N1, N2, N3)]
    vw, vb = randn(g, N3, scale=0.1), randn(g, 1)
    return x.to(DEV), Ws, bs, vw, vb


def chain_ref(x, Ws, bs, vw, vb):
    out, h = [], x.double()
    for W, b in zip(Ws, bs):
        h = elu(h @ W.double().t() + b.double())
        out.append(h)
    return out, h @ vw.double() + vb.double()


def chain_windows(ws, tag, M, dims, x, bs, vw, vb, value_head, y_rows=None):
    """X with exactly M rows; Y1..Y3 with the header's ceil(M / 128) * 128 rows (y_rows: the control declares fewer) and one more slab as the band"""
    K0, N1, N2, N3 = dims
    rows = slabs(M) * 128 if y_rows is None else y_rows
    d = dict(X=ws.inp(tag + "X", x), b=[ws.inp(f"{tag}b{i + 1}", b) for i, b in enumerate(bs)],
             Y=[ws.out(f"{tag}Y{i + 1}", (rows, n), band=256 * n * 4) for i, n in enumerate((N1, N2, N3))])
    if value_head:
        d.update(vw=ws.inp(tag + "v_w", vw), vb=ws.inp(tag + "v_b", vb, skew=4), vo=ws.out(tag + "v_out", (M,), skew=4))
    return d


def check_chain(tag, M, d, refs, vref, bits=None):
    for i, (y, r) in enumerate(zip(d["Y"], refs)):
        X.assert_fully_written(y[:M], f"{tag} Y{i + 1}")
        close(y[:M], r, 2e-5, f"{tag} Y{i + 1}")
        if bits is not None:
            assert torch.equal(y[:M], bits[i]), f"{tag} Y{i + 1}: not the bits of three bg_mlp_layer_forward launches"
    if "vo" in d:
        X.assert_fully_written(d["vo"], f"{tag} v_out")
        close(d["vo"], vref, 2e-5, f"{tag} v_out")


@pytest.mark.parametrize("dims", [ACTOR, CRITIC])
@pytest.mark.parametrize("M", ROWS_ANY)
def test_forward_chain_fp32_holds_whole_slabs_and_not_one_more(M, dims):
    """bg_mlp_chain_forward_group: "Y1 / Y2 / Y3 must hold ceil(M / 128) * 128 rows" and not one more, "v_out [M]" exactly, X rows >= M never read (X
    has M rows: a read behind them returns NaN into rows that are compared), "Bit-identical to three bg_mlp_layer_forward launches"; `workgroups` 0, 3
    and more than the slabs, with and without the value head."""
    L = _L()
    K0, N1, N2, N3 = dims
    x, Ws, bs, vw, vb = chain_inputs(M, dims, 11 * M + N2)
    refs, vref = chain_ref(x, Ws, bs, vw, vb)
    bits, h = [], x
    for W, b in zip(Ws, bs):  # three layer launches: the chain's bits
        z = torch.empty(M, W.shape[0], device=DEV)
        call("bg_mlp_layer_forward", M, h.shape[1], W.shape[0], p(h), p(W), p(b), p(z), 1)
        bits.append(z)
        h = z
    for wgs, head in ((0, True), (3, False), (slabs(M) + 2, True)):
        ws = X.Windows()
        d = chain_windows(ws, "", M, dims, x, bs, vw, vb, head)
        Ww = [ws.inp(f"W{i + 1}", W) for i, W in enumerate(Ws)]
        q = L.MlpChain(M, K0, N1, N2, N3, wgs, p(d["X"]), p(Ww[0]), p(d["b"][0]), p(Ww[1]), p(d["b"][1]), p(Ww[2]), p(d["b"][2]), p(d["Y"][0]), p(d["Y"][1]),
                       p(d["Y"][2]), p(d.get("vw")), p(d.get("vb")), p(d.get("vo")))
        call("bg_mlp_chain_forward_group", C.addressof(q), 1)
        ws.check(f"bg_mlp_chain_forward_group M={M} workgroups={wgs}")
        check_chain(f"bg_mlp_chain_forward_group M={M} wgs={wgs}", M, d, refs, vref, bits)


def split_chain_desc(ws, tag, M, dims, d, Ws, wgs, alternate, slab0=0):
    L = _L()
    K0, N1, N2, N3 = dims
    P = [planes(ws, f"{tag}P{i + 1}", W[:, : K_REAL[dims]].contiguous() if i == 0 else W, W.shape[0], K0 if i == 0 else W.shape[1], pm=True) for i, W in enumerate(Ws)]
    return L.MlpChainSplit(M, K0, N1, N2, N3, wgs, alternate, slab0, p(d["X"]), p(P[0]), p(P[1]), p(P[2]), p(d["b"][0]), p(d["b"][1]), p(d["b"][2]), p(d["Y"][0]),
                           p(d["Y"][1]), p(d["Y"][2]), p(d.get("vw")), p(d.get("vb")), p(d.get("vo")))


@pytest.mark.parametrize("dims", [ACTOR, CRITIC])
@pytest.mark.parametrize("M", ROWS_ANY)
def test_forward_chain_split_holds_whole_slabs_and_not_one_more(M, dims):
    """bg_mlp_chain_forward_split: the same sentences ("Same shapes, slab padding of Y1 / Y2 / Y3, `workgroups` and value head as bg_mlp_chain");
    `workgroups` 0, 3 and more than the slabs, `alternate` 0 / 1, with and without the value head; "which workgroup walks which slab changes no bit"."""
    x, Ws, bs, vw, vb = chain_inputs(M, dims, 13 * M + dims[2])
    refs, vref = chain_ref(x, Ws, bs, vw, vb)
    first = {}
    for wgs, alt, head in ((0, 1, True), (3, 1, False), (slabs(M) + 2, 1, True), (0, 0, True)):
        ws = X.Windows()
        d = chain_windows(ws, "", M, dims, x, bs, vw, vb, head)
        q = split_chain_desc(ws, "", M, dims, d, Ws, wgs, alt)
        call("bg_mlp_chain_forward_split", C.addressof(q), 1)
        ws.check(f"bg_mlp_chain_forward_split M={M} workgroups={wgs} alternate={alt}")
        check_chain(f"bg_mlp_chain_forward_split M={M} wgs={wgs} alt={alt}", M, d, refs, vref)
        got = [y[:M].clone() for y in d["Y"]]
        for a, b in zip(first.setdefault(alt, got), got):
            assert torch.equal(a, b), (wgs, alt)


def test_forward_chain_split_two_networks_and_a_piece_on_an_odd_slab():
    """Two networks in one launch, each inside its own windows; and a piece with slab0 = 1: rows [128, 385) of a 385-row batch through pointers at row 128
    leave the whole launch's bits in rows [128, 385) and touch nothing in front of row 128 (the pointers' front side is the batch's slab 0, compared)."""
    L = _L()
    Ma, Mc = 129, 385
    xa, Wa, ba, vwa, vba = chain_inputs(Ma, ACTOR, 3)
    xc, Wc, bc, vwc, vbc = chain_inputs(Mc, CRITIC, 4)
    ws = X.Windows()
    da, dc = chain_windows(ws, "actor.", Ma, ACTOR, xa, ba, vwa, vba, False), chain_windows(ws, "critic.", Mc, CRITIC, xc, bc, vwc, vbc, True)
    qa, qc = split_chain_desc(ws, "actor.", Ma, ACTOR, da, Wa, 2, 1), split_chain_desc(ws, "critic.", Mc, CRITIC, dc, Wc, 0, 1)
    arr = (L.MlpChainSplit * 2)(qc, qa)
    call("bg_mlp_chain_forward_split", C.addressof(arr), 2)
    ws.check("bg_mlp_chain_forward_split, two networks")
    check_chain("two networks: actor", Ma, da, *chain_ref(xa, Wa, ba, vwa, vba))
    check_chain("two networks: critic", Mc, dc, *chain_ref(xc, Wc, bc, vwc, vbc))
    keep = [y.clone() for y in dc["Y"]] + [dc["vo"].clone()]
    # the piece: slabs 1 .. 3 of the batch alone, on poisoned outputs whose slab 0 keeps the whole launch's values
    r0 = 128
    for y in dc["Y"]:
        y[r0:] = float("nan")
    dc["vo"][r0:] = float("nan")
    part = L.MlpChainSplit.from_buffer_copy(qc)
    part.M, part.slab0 = Mc - r0, 1
    part.X = qc.X + 4 * r0 * 64
    part.Y1, part.Y2, part.Y3, part.v_out = qc.Y1 + 4 * r0 * 256, qc.Y2 + 4 * r0 * 256, qc.Y3 + 4 * r0 * 128, qc.v_out + 4 * r0
    call("bg_mlp_chain_forward_split", C.addressof(part), 1)
    ws.check("bg_mlp_chain_forward_split, a piece with slab0 = 1")
    for k, (a, b) in enumerate(zip(keep, dc["Y"] + [dc["vo"]])):
        assert torch.equal(a[:Mc], b[:Mc]), k


def test_control_a_window_of_M_rows_sees_the_chains_pad_row_stores():
    """Control: the checker can fail.  bg_mlp_chain_forward_split at M = 129 gets its 256 rows of owned memory, but only a 129-row window is declared: the
    documented stores into the last slab's pad rows land in the band (127 rows, inside the arena's 256-row band), and assert_bands_untouched raises."""
    M, dims = 129, ACTOR
    x, Ws, bs, vw, vb = chain_inputs(M, dims, 5)
    ws = X.Windows()
    d = chain_windows(ws, "", M, dims, x, bs, vw, vb, False, y_rows=M)
    q = split_chain_desc(ws, "", M, dims, d, Ws, 0, 1)
    call("bg_mlp_chain_forward_split", C.addressof(q), 1)
    torch.cuda.synchronize()
    hit = 0
    for name, arena in ws.arenas:
        if name in ("Y1", "Y2", "Y3"):
            with pytest.raises(AssertionError, match="behind the window's end"):
                X.assert_bands_untouched(arena, name)
            hit += 1
        else:
            X.assert_bands_untouched(arena, name)
    assert hit == 3
    close(d["Y"][2], chain_ref(x, Ws, bs, vw, vb)[0][2], 2e-5, "control: Y3")


# ---------------------------------------------------------------------------------------------------------------------------- backward chain
def bwd_case(M, dims, seed, pad_fill, wgs=0, alternate=1, g3_rows=None, g3_fill=0.0):
    """every buffer of one bg_mlp_chain_backward_split network in windows; A2 / A1 hold the header's ceil(M / 128) * 128 rows, their pad rows = pad_fill"""
    L = _L()
    N1, N2, N3 = dims
    g = gen(seed)
    G3 = randn(g, M, N3)
    W3, W2 = weight(g, N3, N2), weight(g, N2, N1)
    A2, A1 = elu(randn(g, M, N2)), elu(randn(g, M, N1))
    pad, ws = slabs(M) * 128, X.Windows()
    t = dict(G3=G3, W3=W3, W2=W2, A2=A2, A1=A1, ws=ws)
    G3w = ws.inp("G3", G3) if g3_rows is None else ws.padded("G3", G3, g3_rows, g3_fill)
    t["G3w"] = G3w
    A2w, A1w = ws.padded("A2", A2, pad, pad_fill), ws.padded("A1", A1, pad, pad_fill)
    t["G2"], t["G1"] = ws.out("G2", (pad, N2), band=128 * N2 * 4), ws.out("G1", (pad, N1), band=128 * N1 * 4)
    t["part"] = ws.out("colsum_partial", (slabs(M) * 4, N2 + N1), skew=4, band=4 * (N2 + N1) * 4)  # header: [ceil(M / 128) * 4][N2 + N1]; one more slab: 4 records
    t["b2"], t["b1"] = ws.out("bias_grad2", (N2,), skew=4), ws.out("bias_grad1", (N1,), skew=4)
    PT3, PT2 = planes(ws, "PT3", W3, N2, N3, transpose=1, pm=True), planes(ws, "PT2", W2, N1, N2, transpose=1, pm=True)
    t["d"] = L.MlpChainSplitBwd(M, N1, N2, N3, wgs, alternate, p(G3w), p(PT3), p(PT2), p(A2w), p(A1w), p(t["G2"]), p(t["G1"]), p(t["part"]), p(t["b2"]), p(t["b1"]))
    return t


def bwd_run(t):
    L = _L()
    fin = L.ReduceProblem()
    call("bg_mlp_chain_backward_split", C.addressof(t["d"]), 1, C.byref(fin))
    torch.cuda.synchronize()
    assert bool(X.is_poison(t["b2"]).all()) and bool(X.is_poison(t["b1"]).all())  # the bias gradients wait for the descriptor
    call("bg_reduce_group", (L.ReduceProblem * 1)(fin), 1)
    t["ws"].check("bg_mlp_chain_backward_split")
    return [t[k].clone() for k in ("G2", "G1", "b2", "b1")]


@pytest.mark.parametrize("dims", [(256, 128, 128), (256, 256, 128)])
@pytest.mark.parametrize("M", ROWS_ANY)
def test_backward_chain_pad_rows_and_records(M, dims):
    """bg_mlp_chain_backward_split: "G2 / G1 must hold ceil(M / 128) * 128 rows (rows >= M are written with zeros)", "colsum_partial ([ceil(M / 128) * 4]
    [N2 + N1] floats)", A2 / A1 "holding ceil(M / 128) * 128 rows of finite values ... rows >= M do not enter the results": the same bits with their pad
    rows at 0 and at 1e30 (c)."""
    N1, N2, N3 = dims
    outs = []
    for fill, wgs in ((0.0, 0), (1e30, 0), (0.0, 3)):
        t = bwd_case(M, dims, 7 * M + N2, fill, wgs=wgs)
        outs.append(bwd_run(t))
        for k in ("G2", "G1", "part", "b2", "b1"):
            X.assert_fully_written(t[k], f"bg_mlp_chain_backward_split: {k}")
        assert bool((t["G2"][M:] == 0).all()) and bool((t["G1"][M:] == 0).all()), "pad rows of G2 / G1 must be zeros"
    r2 = (t["G3"].double() @ t["W3"].double()) * elup(t["A2"]).double()
    r1 = (r2 @ t["W2"].double()) * elup(t["A1"]).double()
    for k, (a, b, c) in enumerate(zip(*outs)):
        assert torch.equal(a, b), f"output {k} moved with the pad rows of A2 / A1"
        assert torch.equal(a, c), f"output {k} moved with the workgroup count"
    G2, G1, b2, b1 = outs[0]
    for name, got, ref in (("G2", G2[:M], r2), ("G1", G1[:M], r1)):
        close(got, ref, 2e-5, f"bg_mlp_chain_backward_split {name} M={M}")
    for name, got, ref in (("bias_grad2", b2, r2.sum(0)), ("bias_grad1", b1, r1.sum(0))):
        close(got, ref, 1e-4, f"bg_mlp_chain_backward_split {name} M={M}")


def test_control_backward_chain_rows_of_G3_beyond_M_are_never_used():
    """Control: G3 "[M][N3]" -- with 127 more rows of owned memory behind row M filled with 1e30 nothing moves; with 1e30 in row M - 1 the bias gradients
    do (the check can see a row that enters the sums)."""
    M, dims = 129, (256, 128, 128)
    base = bwd_run(bwd_case(M, dims, 21, 0.0))
    t = bwd_case(M, dims, 21, 0.0, g3_rows=256, g3_fill=1e30)
    far = bwd_run(t)
    for k, (a, b) in enumerate(zip(base, far)):
        assert torch.equal(a, b), f"output {k} moved with rows of G3 at or beyond M"
    t = bwd_case(M, dims, 21, 0.0, g3_rows=256, g3_fill=1e30)
    t["G3w"][M - 1] = 1e30
    near = bwd_run(t)
    assert not torch.equal(base[2], near[2]) and not torch.equal(base[3], near[3])


# ---------------------------------------------------------------------------------------------------------------------------- weight gradients
def wgrad_problem(ws, tag, M, co, ci, cr, slices, tw, seed, pad_fill):
    """one bg_wgrad_problem in windows: scratch exactly "slices * C_out * C_in floats" (band: one more slice), dW "[C_out][C_in_real]" with row stride
    C_in_real and nothing behind it (band: what a row stride of C_in would overrun); dW at a 4-byte skew when C_in_real < C_in -- in production it is a
    slice of the flat gradient buffer -- and 16-byte aligned otherwise (the entry points' own check); A's padded columns = pad_fill"""
    g = gen(seed)
    G, A = randn(g, M, co), randn(g, M, ci)
    G[:, 3] *= 3.0
    A[:, 1] += 0.5
    G[0, co - 1] = 4.0
    A[0, cr - 1] = -2.5
    ref = G.double().t() @ A.double()[:, :cr]
    A[:, cr:] = pad_fill
    t = dict(G=ws.inp(tag + "G", G), A=ws.inp(tag + "A", A), ref=ref,
             dW=ws.out(tag + "dW", (co, cr), skew=4 if cr < ci else 16, band=co * ci * 4),
             scratch=ws.out(tag + "scratch", (slices * co * ci,), band=co * ci * 4))
    q = _L().WgradProblem(p(t["G"]), p(t["A"]), p(t["dW"]), p(t["scratch"]), M, co, ci, cr, slices, tw)
    return t, q


WGRAD_LAYERS = [(256, 64, 47), (256, 64, 61), (128, 256, 256), (256, 256, 256), (128, 128, 128), (512, 128, 128), (128, 512, 512)]


@pytest.mark.parametrize("co,ci,cr", WGRAD_LAYERS)
@pytest.mark.parametrize("M", ROWS_EVEN)
def test_weight_grad_scratch_and_row_stride(M, co, ci, cr):
    """bg_mlp_weight_grad at the smallest legal `slices` (8): "scratch: slices * C_out * C_in floats", "only the first C_in_real columns are written, with
    row stride C_in_real"; the padded columns of A do not enter dW: the same bits with them at 0 and at 1e30."""
    got = []
    for fill in (0.0, 1e30):
        ws = X.Windows()
        t, q = wgrad_problem(ws, "", M, co, ci, cr, 8, 1, M + co + 7 * ci + cr, fill)
        call("bg_mlp_weight_grad", M, co, ci, cr, p(t["G"]), p(t["A"]), p(t["dW"]), p(t["scratch"]), 8)
        ws.check(f"bg_mlp_weight_grad M={M} {co}x{ci}({cr}) pad={fill}")
        X.assert_fully_written(t["dW"], "bg_mlp_weight_grad: dW")
        got.append(t["dW"].clone())
    assert torch.equal(got[0], got[1]), "dW moved with the padded columns of A"
    close(got[0], t["ref"], 1e-4, f"bg_mlp_weight_grad M={M} {co}x{ci}({cr})")  # a sum over rows: 1e-4 of the largest entry


def _wgrad_group(M, split, slices_of, pad_fill=0.0):
    """(problem array, per-layer dicts, windows) of the reference's six hidden layers (actor 47(64)-256-128-128, critic 61(64)-256-256-128) that are legal
    at M: the plain group takes all six; the split group needs slices * (4 / tiles) <= M / 32, which at M = 32 leaves the 256 x 256 layer alone"""
    L = _L()
    layers = [(256, 64, 47), (128, 256, 256), (128, 128, 128), (256, 64, 61), (256, 256, 256), (128, 256, 256)]
    ws, ts, qs = X.Windows(), [], []
    for k, (co, ci, cr) in enumerate(layers):
        tiles = (co // 128) * max(1, ci // 128)
        tw = tiles if split else 1
        s = slices_of(k)
        if split and s * (4 // tw) > M // 32:
            continue
        t, q = wgrad_problem(ws, f"layer{k}.", M, co, ci, cr, s, tw, 100 * M + k, pad_fill)
        ts.append(t)
        qs.append(q)
    assert qs
    return (L.WgradProblem * len(qs))(*qs), ts, ws


def _tail_norm(ws):
    return ws.out("norm_scratch", (_L().TAIL_MAX_BLOCKS,), F64, skew=8)  # header: float64 [BG_TAIL_MAX_BLOCKS]


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("M", ROWS_EVEN)
def test_weight_grad_group_and_its_partial_form(M, odd):
    """bg_mlp_weight_grad_group at the smallest legal `slices` (1) and at an odd count (3); bg_mlp_weight_grad_group_partial + bg_update_tail_sums leave the
    same bits in dW ("the same scratch layout, the same finish") within the same extents; norm_scratch is float64 [BG_TAIL_MAX_BLOCKS].  The padded columns
    of A (47 / 61 -> 64) do not enter dW: the full form with them at 1e30 and the partial form with them at 1e30 give the bits of the full form at 0."""
    L = _L()
    arr, ts, ws = _wgrad_group(M, False, lambda k: 3 if odd else 1)
    call("bg_mlp_weight_grad_group", arr, len(ts))
    ws.check(f"bg_mlp_weight_grad_group M={M}")
    for k, t in enumerate(ts):
        X.assert_fully_written(t["dW"], f"layer {k}: dW")
        X.assert_fully_written(t["scratch"], f"layer {k}: scratch")  # every slice leaves its tile: the header's extent is used up to its last float
        close(t["dW"], t["ref"], 1e-4, f"bg_mlp_weight_grad_group M={M} layer {k}")
    arr1, ts1, ws1 = _wgrad_group(M, False, lambda k: 3 if odd else 1, pad_fill=1e30)  # (c): the padded columns of A at 1e30 instead of 0
    call("bg_mlp_weight_grad_group", arr1, len(ts1))
    ws1.check(f"bg_mlp_weight_grad_group M={M}, padded columns at 1e30")
    for k, (a, b) in enumerate(zip(ts, ts1)):
        assert torch.equal(a["dW"], b["dW"]), f"layer {k}: dW moved with the padded columns of A"
    arr2, ts2, ws2 = _wgrad_group(M, False, lambda k: 3 if odd else 1, pad_fill=1e30)
    norm = _tail_norm(ws2)
    call("bg_mlp_weight_grad_group_partial", arr2, len(ts2))
    torch.cuda.synchronize()
    assert all(bool(X.is_poison(t["dW"]).all()) for t in ts2), "the partial form wrote dW"
    call("bg_update_tail_sums", arr2, len(ts2), None, 0, p(norm))
    ws2.check(f"bg_mlp_weight_grad_group_partial + bg_update_tail_sums M={M}")
    for k, (a, b) in enumerate(zip(ts, ts2)):
        assert torch.equal(a["dW"], b["dW"]), k


@pytest.mark.parametrize("terms", [9, 6])
@pytest.mark.parametrize("M", ROWS_32)
def test_weight_grad_group_split_and_its_partial_form(M, terms):
    """bg_mlp_weight_grad_group_split / _partial (M a multiple of 32, smallest legal `slices` = 1): the same extents; the partial form + bg_update_tail_sums
    gives the full form's bits; the padded columns of A at 1e30 change no bit of dW in either form (at M = 32 only the 256 x 256 layer is legal, which
    has none: the first layers run at 160 and 1056 rows)."""
    arr, ts, ws = _wgrad_group(M, True, lambda k: 1)
    call("bg_mlp_weight_grad_group_split", arr, len(ts), terms)
    ws.check(f"bg_mlp_weight_grad_group_split M={M} terms={terms}")
    for k, t in enumerate(ts):
        X.assert_fully_written(t["dW"], f"layer {k}: dW")
        X.assert_fully_written(t["scratch"], f"layer {k}: scratch")
        close(t["dW"], t["ref"], 1e-4, f"bg_mlp_weight_grad_group_split M={M} terms={terms} layer {k}")
    arr1, ts1, ws1 = _wgrad_group(M, True, lambda k: 1, pad_fill=1e30)  # (c): the padded columns of A at 1e30 instead of 0
    call("bg_mlp_weight_grad_group_split", arr1, len(ts1), terms)
    ws1.check(f"bg_mlp_weight_grad_group_split M={M}, padded columns at 1e30")
    for k, (a, b) in enumerate(zip(ts, ts1)):
        assert torch.equal(a["dW"], b["dW"]), f"layer {k}: dW moved with the padded columns of A"
    arr2, ts2, ws2 = _wgrad_group(M, True, lambda k: 1, pad_fill=1e30)
    norm = _tail_norm(ws2)
    call("bg_mlp_weight_grad_group_split_partial", arr2, len(ts2), terms)
    torch.cuda.synchronize()
    assert all(bool(X.is_poison(t["dW"]).all()) for t in ts2), "the partial form wrote dW"
    call("bg_update_tail_sums", arr2, len(ts2), None, 0, p(norm))
    ws2.check(f"bg_mlp_weight_grad_group_split_partial + bg_update_tail_sums M={M}")
    for k, (a, b) in enumerate(zip(ts, ts2)):
        assert torch.equal(a["dW"], b["dW"]), k


# ---------------------------------------------------------------------------------------------------------------------------- weight planes
@pytest.mark.parametrize("n,k,rows,cols,transpose", [(256, 64, 256, 47, 0), (256, 64, 256, 61, 0), (128, 256, 256, 128, 1), (128, 128, 128, 128, 0), (128, 512, 128, 512, 0)])
def test_split_weights_planes_extent(n, k, rows, cols, transpose):
    """bg_mlp_split_weights / _pm: "planes[n_out][k_out / 32][3][32] bf16" = n_out * k_out * 3 uint16 ("2 * n_out * k_out * 3" for _pm), "elements outside
    the source are zero"; hi + mid + lo == w exactly (the header's "EXACTLY the sum of three bf16 numbers"), the planes of -W are those of W with the
    sign bits flipped."""
    g = gen(n + k + cols)
    w = randn(g, rows, cols)
    want = np.zeros((n, k))
    src = (w.t() if transpose else w).double().cpu().numpy()
    want[: src.shape[0], : src.shape[1]] = src
    for pm in (False, True):
        ws = X.Windows()
        pl = planes(ws, "planes", w, n, k, transpose, pm)
        ws.check(f"bg_mlp_split_weights{'_pm' if pm else ''} {n}x{k}")
        X.assert_fully_written(pl, "planes")
        half = n * k * 3
        hi, mid, lo = unpack_planes(pl[:half], n, k)
        assert np.array_equal(hi + mid + lo, want)  # exact; n * k elements, the zero padding included
        if pm:
            assert torch.equal(pl[:half] ^ -32768, pl[half:])


# ---------------------------------------------------------------------------------------------------------------------------- ELU backward + column sums
@pytest.mark.parametrize("C_", [12, 128, 256, 384])
@pytest.mark.parametrize("with_act", [True, False])
@pytest.mark.parametrize("B", ROWS_ANY)
def test_elu_backward_colsum_scratch(B, with_act, C_):
    """bg_elu_backward_colsum: "scratch: ceil(B/128) * C floats", grad [B][C] in place, colsum [C]; the act == NULL form (identity).  No alignment is
    promised: at skew 4 every buffer sits 4 bytes past a 256-byte boundary (the generic form runs), at skew 16 grad / act / scratch are 16-byte aligned
    (C = 128 / 256 with act then take the wider form: the same terms of a column in another fixed order)."""
    g = gen(B + C_)
    grad, act = randn(g, B, C_), elu(randn(g, B, C_))
    ref = grad.double() * (elup(act).double() if with_act else 1.0)
    for skew in (4, 16):  # (16-byte aligned buffers of 128 / 256 columns take the kernel's 16-byte form, every other case the generic one)
        ws = X.Windows()
        gw = ws.inp("grad", grad, skew=skew)
        aw = ws.inp("act", act, skew=skew) if with_act else None
        col = ws.out("colsum", (C_,), skew=4)
        scratch = ws.out("scratch", (slabs(B) * C_,), skew=skew, band=C_ * 4)
        call("bg_elu_backward_colsum", B, C_, p(gw), p(aw), p(col), p(scratch))
        ws.check(f"bg_elu_backward_colsum B={B} C={C_} skew={skew}")
        X.assert_fully_written(col, "colsum")
        X.assert_fully_written(scratch, "scratch")
        close(gw, ref, 2e-5, f"bg_elu_backward_colsum grad B={B} C={C_}")
        close(col, ref.sum(0), 1e-4, f"bg_elu_backward_colsum colsum B={B} C={C_}")


# ---------------------------------------------------------------------------------------------------------------------------- output-layer heads
HALF_LOG_2PI = 0.9189385332046727
E_CLIP, BOUND_COEF, ENT_COEF, SYM_COEF = 0.2, 1.0, -0.01, 0.5
ACT_SRC = [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]          # left leg <-> right leg
ACT_SIGN = [1, -1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1]     # (sign[src[a]] == sign[a])


def rel(got, ref, what):
    """largest error relative to the largest entry, over every element of the documented shape (test_gpu_head.py's measure)"""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    r = ((got.double() - ref.double()).abs().max() / max(1e-30, ref.double().abs().max().item())).item()
    print(f"{what}: {got.numel()} elements, relative error {r:.3e}")
    return r


def head_inputs(B, rows, seed):
    """test_gpu_head.py's data recipe on `rows` rows of h (rows = 2B for the heads with a symmetry term), the PPO inputs on B rows"""
    g = gen(seed)
    A = 12
    t = dict(h=elu(randn(g, rows, 128)), W=randn(g, A, 128, scale=0.1), b=randn(g, A, scale=0.1))
    t["logstd"] = torch.full((A,), -2.0, device=DEV) + randn(g, A, scale=0.1)
    t["old_logstd"] = torch.full((A,), -2.0, device=DEV)
    mu = t["h"][:B] @ t["W"].t() + t["b"]
    t["old_mu"] = mu + randn(g, B, A, scale=0.02)
    t["actions"] = t["old_mu"] + randn(g, B, A, scale=0.135)
    t["old_logp"] = (-0.5 * ((t["actions"] - t["old_mu"]) / t["old_logstd"].exp()) ** 2 - t["old_logstd"] - HALF_LOG_2PI).sum(-1)
    t["adv"] = randn(g, B)
    # the advantage moments of a larger batch (bg_gae's sums): mean 0.1, variance about 1, count 4096 -- so that B = 1 has a variance
    t["adv_stats"] = torch.tensor([409.6, 4096.0 * 1.01, 4096.0], dtype=F64, device=DEV)
    t["values"], t["returns"] = randn(g, B), randn(g, B)
    return t


def ppo_terms(t, mu, ls):
    """float64, per row of mu [B][12] under log-std ls [12]: (surrogate [B], bound penalty [B][12], entropy of one row, kl [B]) -- runner.py:145-174"""
    ols, s = t["old_logstd"].double(), t["adv_stats"]
    mean = s[0] / s[2]
    An = (t["adv"].double() - mean) / (((s[1] - s[2] * mean * mean) / (s[2] - 1.0)).sqrt() + 1e-8)
    logp = (-0.5 * ((t["actions"].double() - mu) / ls.exp()) ** 2 - ls - HALF_LOG_2PI).sum(-1)
    ratio = (logp - t["old_logp"].double()).exp()
    surr = torch.max(-An * ratio, -An * ratio.clamp(1.0 - E_CLIP, 1.0 + E_CLIP))
    bound = torch.relu(mu - 1.0) ** 2 + torch.clamp(mu + 1.0, max=0.0) ** 2
    ent = (0.5 + HALF_LOG_2PI + ls).sum()
    kl = (ls - ols + 0.5 * (ols.exp() ** 2 + (mu - t["old_mu"].double()) ** 2) / ls.exp() ** 2 - 0.5).sum(-1)
    return surr, bound, ent, kl


def actor_loss_ref(t, B, sym):
    """float64 autograd of the actor's loss on the head's inputs: (mu [rows][12], g_hidden, grad_W, grad_b, grad_b_hidden, grad_logstd, stats [6])"""
    h, W, b, ls = (t[k].double().clone().requires_grad_() for k in ("h", "W", "b", "logstd"))
    mu_all = h @ W.t() + b
    mu = mu_all[:B]
    surr, bound, ent, kl = ppo_terms(t, mu, ls)
    loss = surr.mean() + BOUND_COEF * bound.mean() + ENT_COEF * ent
    sq = torch.zeros((), dtype=F64, device=DEV)
    if sym:
        d = mu_all[B:] - torch.tensor(ACT_SIGN, dtype=F64, device=DEV) * mu[:, ACT_SRC]
        sq = (d**2).sum()
        loss = loss + SYM_COEF / (B * 12) * sq
    loss.backward()
    g_hidden = h.grad * elup(h.detach())
    stats = torch.stack([torch.zeros_like(sq), surr.sum(), bound.sum(), ent * B, kl.sum(), sq]).detach()
    return mu_all.detach(), g_hidden, W.grad, b.grad, g_hidden.sum(0), ls.grad, stats


def head_windows(ws, t, B, rows, n_stats):
    """inputs at the skew the header promises (h: 16 bytes; nothing for the rest: 4, float64: 8), outputs of exactly the documented shapes, the scratch of
    exactly BG_HEAD_SCRATCH_FLOATS floats with one more record (12 * 128 + 128 + 16 floats) as its band"""
    L = _L()
    w = {k: ws.inp(k, t[k], skew=16 if k == "h" else (8 if t[k].dtype == F64 else 4)) for k in t}
    w["mu_out"], w["g_hidden"] = ws.out("mu_out", (rows, 12), skew=4), ws.out("g_hidden", (rows, 128), skew=4, band=64 * 128 * 4)  # (one more 64-row tile)
    w["grad_W"], w["grad_b"], w["grad_b_hidden"] = ws.out("grad_W", (12, 128), skew=4), ws.out("grad_b", (12,), skew=4), ws.out("grad_b_hidden", (128,), skew=4)
    w["grad_logstd"], w["stats"] = ws.zeros("grad_logstd", (12,), F64, skew=8), ws.zeros("stats", (n_stats,), F64, skew=8)
    w["scratch"] = ws.out("scratch", (L.HEAD_SCRATCH_FLOATS,), skew=16, band=8192)
    return w


def check_finish_fits(fin):
    """what bg_head.hip's static_assert states, from outside: the records and the float64 statistics the descriptor names lie inside BG_HEAD_SCRATCH_FLOATS
    for this launch and for the largest grid (768 workgroups)"""
    L = _L()
    assert fin.groups <= 768
    for groups in (fin.groups, 768):
        assert groups * fin.record <= fin.stat_base and fin.stat_base + 2 * fin.n_stat * groups <= L.HEAD_SCRATCH_FLOATS, (groups, fin.record, fin.n_stat)


@pytest.mark.parametrize("B", ROWS_ANY)
def test_actor_head_outputs_and_scratch(B):
    """bg_actor_head modes 0 / 1 and bg_actor_head_partial: "scratch: BG_HEAD_SCRATCH_FLOATS floats", mu_out / g_hidden [B] rows exactly, grad_W [12][128],
    grad_b [12], grad_b_hidden [128], grad_logstd [12], stats [5] with stats[0] "left to the critic head"; mode 0: "nothing else is touched"; the _partial
    form + bg_reduce_group: "Same sums, same fixed order as the immediate forms for the heads" -- bit for bit."""
    L = _L()
    t = head_inputs(B, B, 17 * B)
    mu_ref, gh_ref, dW_ref, db_ref, dbh_ref, gls_ref, st_ref = actor_loss_ref(t, B, False)
    ppo = lambda w: (p(w["h"]), p(w["W"]), p(w["b"]), p(w["logstd"]), p(w["actions"]), p(w["old_mu"]), p(w["old_logstd"]), p(w["old_logp"]), p(w["adv"]),
                     p(w["adv_stats"]), E_CLIP, BOUND_COEF, ENT_COEF, p(w["mu_out"]), p(w["g_hidden"]), p(w["grad_W"]), p(w["grad_b"]), p(w["grad_b_hidden"]),
                     p(w["grad_logstd"]), p(w["stats"]), p(w["scratch"]))
    # mode 0: the forward alone; every other buffer is handed over and must come back as it was
    ws = X.Windows()
    w = head_windows(ws, t, B, B, 5)
    call("bg_actor_head", B, 0, *ppo(w))
    ws.check(f"bg_actor_head mode 0 B={B}")
    X.assert_fully_written(w["mu_out"], "mode 0: mu_out")
    close(w["mu_out"], mu_ref, 2e-5, f"bg_actor_head mode 0 mu_out B={B}")
    for k in ("g_hidden", "grad_W", "grad_b", "grad_b_hidden", "scratch"):
        assert bool(X.is_poison(w[k]).all()), f"mode 0 touched {k}"
    assert bool((w["grad_logstd"] == 0).all()) and bool((w["stats"] == 0).all())
    mu0 = w["mu_out"].clone()
    # mode 1, immediate and deferred
    got = {}
    for form in ("bg_actor_head", "bg_actor_head_partial"):
        ws = X.Windows()
        w = head_windows(ws, t, B, B, 5)
        if form == "bg_actor_head":
            call(form, B, 1, *ppo(w))
        else:
            fin = L.ReduceProblem()
            call(form, B, *ppo(w), C.byref(fin))
            torch.cuda.synchronize()
            assert all(bool(X.is_poison(w[k]).all()) for k in ("grad_W", "grad_b", "grad_b_hidden")) and bool((w["stats"] == 0).all())
            check_finish_fits(fin)
            call("bg_reduce_group", (L.ReduceProblem * 1)(fin), 1)
        ws.check(f"{form} B={B}")
        for k in ("mu_out", "g_hidden", "grad_W", "grad_b", "grad_b_hidden"):
            X.assert_fully_written(w[k], f"{form}: {k}")
        got[form] = {k: w[k].clone() for k in ("mu_out", "g_hidden", "grad_W", "grad_b", "grad_b_hidden", "grad_logstd", "stats")}
    now, later = got["bg_actor_head"], got["bg_actor_head_partial"]
    for k in now:
        assert torch.equal(now[k], later[k]), f"deferred {k} differs from the immediate form"
    assert torch.equal(now["mu_out"], mu0)  # mode 0's bits
    close(now["mu_out"], mu_ref, 2e-5, f"bg_actor_head mode 1 mu_out B={B}")
    # test_gpu_head.py: 2e-3 of the largest entry for what passes through the ratio's exp() (an error of mu is amplified by |adv| / sigma^2 ~ 50)
    for k, ref in (("g_hidden", gh_ref), ("grad_W", dW_ref), ("grad_b", db_ref), ("grad_b_hidden", dbh_ref), ("grad_logstd", gls_ref)):
        assert rel(now[k], ref, f"bg_actor_head B={B} {k}") < 2e-3, k
    assert rel(now["stats"][1:], st_ref[1:5], f"bg_actor_head B={B} stats[1..4]") < 1e-4 and float(now["stats"][0]) == 0.0


@pytest.mark.parametrize("B", ROWS_ANY + [24577])
def test_actor_head_sym_outputs_and_scratch(B):
    """bg_actor_head_sym / _sym_partial: h / g_hidden / mu_out "[2B]" rows exactly, stats [6], the same scratch.  B = 24,577 makes 769 pair tiles: the grid
    is the largest there is (768 workgroups, one of them walking two tiles) and the records and statistics reach as far into the scratch as they ever
    do."""
    L = _L()
    t = head_inputs(B, 2 * B, 19 * B)
    mu_ref, gh_ref, dW_ref, db_ref, dbh_ref, gls_ref, st_ref = actor_loss_ref(t, B, True)
    src, sign = (C.c_int32 * 12)(*ACT_SRC), (C.c_float * 12)(*ACT_SIGN)
    args = lambda w: (p(w["h"]), p(w["W"]), p(w["b"]), p(w["logstd"]), p(w["actions"]), p(w["old_mu"]), p(w["old_logstd"]), p(w["old_logp"]), p(w["adv"]),
                      p(w["adv_stats"]), E_CLIP, BOUND_COEF, ENT_COEF, SYM_COEF, src, sign, p(w["mu_out"]), p(w["g_hidden"]), p(w["grad_W"]), p(w["grad_b"]),
                      p(w["grad_b_hidden"]), p(w["grad_logstd"]), p(w["stats"]), p(w["scratch"]))
    got = {}
    for form in ("bg_actor_head_sym", "bg_actor_head_sym_partial"):
        ws = X.Windows()
        w = head_windows(ws, t, B, 2 * B, 6)
        if form == "bg_actor_head_sym":
            call(form, B, *args(w))
        else:
            fin = L.ReduceProblem()
            call(form, B, *args(w), C.byref(fin))
            check_finish_fits(fin)
            assert fin.groups == min(768, (B + 31) // 32) and fin.n_stat == 18
            call("bg_reduce_group", (L.ReduceProblem * 1)(fin), 1)
        ws.check(f"{form} B={B}")
        for k in ("mu_out", "g_hidden", "grad_W", "grad_b", "grad_b_hidden"):
            X.assert_fully_written(w[k], f"{form}: {k}")
        got[form] = {k: w[k].clone() for k in ("mu_out", "g_hidden", "grad_W", "grad_b", "grad_b_hidden", "grad_logstd", "stats")}
    now, later = got["bg_actor_head_sym"], got["bg_actor_head_sym_partial"]
    for k in now:
        assert torch.equal(now[k], later[k]), f"deferred {k} differs from the immediate form"
    close(now["mu_out"], mu_ref, 2e-5, f"bg_actor_head_sym mu_out B={B}")
    for k, ref in (("g_hidden", gh_ref), ("grad_W", dW_ref), ("grad_b", db_ref), ("grad_b_hidden", dbh_ref), ("grad_logstd", gls_ref)):
        assert rel(now[k], ref, f"bg_actor_head_sym B={B} {k}") < 2e-3, k
    assert rel(now["stats"][1:], st_ref[1:], f"bg_actor_head_sym B={B} stats[1..5]") < 1e-4 and float(now["stats"][0]) == 0.0


@pytest.mark.parametrize("B", ROWS_ANY)
def test_critic_heads_outputs_and_scratch(B):
    """bg_critic_head_forward: values [rows] exactly; bg_critic_head_backward / _partial: g_hidden [B][128], grad_w [128], grad_b [1], grad_b_hidden [128],
    stats[0] alone, the scratch of BG_HEAD_SCRATCH_FLOATS floats; the deferred form bit for bit."""
    L = _L()
    t = head_inputs(B, B, 23 * B)
    h, w1, b1 = t["h"], t["W"][:1].contiguous(), t["b"][:1].contiguous()
    ws = X.Windows()
    hw, ww, bw = ws.inp("h", h), ws.inp("w", w1), ws.inp("b", b1, skew=4)  # header: h and w 16-byte aligned
    v = ws.out("values", (B,), skew=4)
    call("bg_critic_head_forward", B, p(hw), p(ww), p(bw), p(v))
    ws.check(f"bg_critic_head_forward B={B}")
    X.assert_fully_written(v, "values")
    close(v, (h.double() @ w1.double().t() + b1.double()).squeeze(-1), 2e-5, f"bg_critic_head_forward B={B}")
    gval = 2.0 * (t["values"].double() - t["returns"].double()) / B
    g_ref = gval[:, None] * w1.double() * elup(h).double()
    dw_ref, db_ref, dbh_ref = (gval[:, None] * h.double()).sum(0), gval.sum().reshape(1), g_ref.sum(0)
    sse = ((t["values"].double() - t["returns"].double()) ** 2).sum().item()
    got = {}
    for form in ("bg_critic_head_backward", "bg_critic_head_backward_partial"):
        ws = X.Windows()
        hw, ww = ws.inp("h", h), ws.inp("w", w1.reshape(128), skew=4)  # (the backward head reads w float by float: no alignment is asked of it)
        vw, rw = ws.inp("values", t["values"], skew=4), ws.inp("returns", t["returns"], skew=4)
        o = dict(g_hidden=ws.out("g_hidden", (B, 128), skew=4, band=64 * 128 * 4), grad_w=ws.out("grad_w", (128,), skew=4), grad_b=ws.out("grad_b", (1,), skew=4),
                 grad_b_hidden=ws.out("grad_b_hidden", (128,), skew=4), stats=ws.zeros("stats", (5,), F64, skew=8))
        scratch = ws.out("scratch", (L.HEAD_SCRATCH_FLOATS,), skew=16, band=8192)
        a = (B, p(hw), p(ww), p(vw), p(rw), p(o["g_hidden"]), p(o["grad_w"]), p(o["grad_b"]), p(o["grad_b_hidden"]), p(o["stats"]), p(scratch))
        if form.endswith("_partial"):
            fin = L.ReduceProblem()
            call(form, *a, C.byref(fin))
            check_finish_fits(fin)
            call("bg_reduce_group", (L.ReduceProblem * 1)(fin), 1)
        else:
            call(form, *a)
        ws.check(f"{form} B={B}")
        for k in ("g_hidden", "grad_w", "grad_b", "grad_b_hidden"):
            X.assert_fully_written(o[k], f"{form}: {k}")
        got[form] = {k: x.clone() for k, x in o.items()}
    now, later = got["bg_critic_head_backward"], got["bg_critic_head_backward_partial"]
    for k in now:
        assert torch.equal(now[k], later[k]), f"deferred {k} differs from the immediate form"
    # test_gpu_head.py's bounds
    assert rel(now["g_hidden"], g_ref, "critic g_hidden") < 1e-5 and rel(now["grad_w"], dw_ref, "critic grad_w") < 1e-4 and rel(now["grad_b_hidden"], dbh_ref, "critic grad_b_hidden") < 1e-4
    assert abs(now["grad_b"].item() - db_ref.item()) < 1e-4 * max(gval.abs().sum().item() / B, 1e-6) * B**0.5 + 1e-7
    assert abs(now["stats"][0].item() - sse) <= 1e-5 * sse and bool((now["stats"][1:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------- GAE
GAE_SHAPES = [(1, 1), (5, 17), (32, 16), (3, 33)]
GAMMA, LAM = float(np.float32(0.995)), float(np.float32(0.95))  # (what the library receives: fp32 arguments)


def gae_ref(rew, dones, touts, values, last):
    """float64: (rewards with the time-out bootstrap, advantages, returns) -- utils/utils.py:33-44 under runner.py:135"""
    r, v = rew.double().clone(), values.double()
    r[touts] = v[touts]
    nn = 1.0 - (dones | touts).double()
    adv, la, nv = torch.zeros_like(r), torch.zeros_like(r[0]), last.double()
    for t in reversed(range(r.shape[0])):
        la = r[t] + GAMMA * nn[t] * nv - v[t] + GAMMA * LAM * nn[t] * la
        adv[t], nv = la, v[t]
    return r, adv, v + adv


def gae_inputs(T, N, seed):
    g = gen(seed)
    t = dict(h=elu(randn(g, (T + 1) * N, 128)), w=randn(g, 128, scale=0.1), b=randn(g, 1), rew=randn(g, T, N))
    t["dones"] = (torch.rand(T, N, generator=g) < 0.2).to(DEV)
    t["touts"] = (torch.rand(T, N, generator=g) < 0.2).to(DEV)
    return t


def check_sums(sums, adv, ret=None):
    """float64 moments of what the launch wrote (another fixed order than torch's: 1e-12, test_gpu_head.py), the count exactly.  ret: the fp32 returns
    R = v + advantage, rounded once as the launch rounds them; their two sums to 1e-12 relative (test_gpu_value_norm.py)"""
    want = [adv.double().sum(), (adv.double() ** 2).sum(), torch.tensor(float(adv.numel()), dtype=F64, device=DEV)]
    if ret is not None:
        assert ret.dtype == F32
        want += [ret.double().sum(), (ret.double() ** 2).sum(), want[2]]
    want = torch.stack(want)
    assert tuple(sums.shape) == tuple(want.shape)
    assert torch.allclose(sums[:3], want[:3], rtol=1e-12, atol=1e-9), (sums, want)
    assert float(sums[2]) == adv.numel()
    if ret is not None:
        err = ((sums[3:5] - want[3:5]).abs() / want[3:5].abs()).max().item()
        print(f"sums of R against float64: {err:.3e}")
        assert err <= 1e-12 and float(sums[5]) == adv.numel(), (sums, want)


@pytest.mark.parametrize("T,N", GAE_SHAPES)
def test_gae_launches_outputs_and_ticket(T, N):
    """bg_gae: advantages / returns [T][N], "sums out [3]" accumulated; bg_critic_values_gae with and without h: "values_all [(T + 1) N]", "sums float64 [3]
    WRITTEN", "scratch: float64 [3 * ceil(N / 16) + 1], its last element zero-initialised once by the caller (the launch leaves it zero)"."""
    t = gae_inputs(T, N, 31 * T + N)
    vall = (t["h"].double() @ t["w"].double() + t["b"].double()).float()  # the values the scan starts from, as fp32 inputs of the reference
    # bg_gae on given values
    ws = X.Windows()
    rew, dn, to = ws.inp("rewards", t["rew"], skew=4), ws.inp("dones", t["dones"].to(U8), skew=4), ws.inp("time_outs", t["touts"].to(U8), skew=4)
    val, last = ws.inp("values", vall[: T * N].view(T, N), skew=4), ws.inp("last_values", vall[T * N :], skew=4)
    adv, ret = ws.out("advantages", (T, N), skew=4), ws.out("returns", (T, N), skew=4)
    sums = ws.zeros("sums", (3,), F64, skew=8)
    call("bg_gae", T, N, p(rew), p(dn), p(to), p(val), p(last), GAMMA, LAM, p(adv), p(ret), p(sums))
    ws.check(f"bg_gae T={T} N={N}")
    r_ref, a_ref, ret_ref = gae_ref(t["rew"], t["dones"], t["touts"], vall[: T * N].view(T, N), vall[T * N :])
    X.assert_fully_written(adv, "advantages")
    X.assert_fully_written(ret, "returns")
    assert torch.equal(rew, r_ref.float())  # the bootstrap is a copy of an fp32 value
    close(adv, a_ref, 2e-5, f"bg_gae advantages T={T} N={N}")  # test_gpu_ppo.py: 2e-5 on the fused form's advantages and returns
    close(ret, ret_ref, 2e-5, f"bg_gae returns T={T} N={N}")
    check_sums(sums, adv)
    adv0, ret0 = adv.clone(), ret.clone()
    # the fused launch: with h (values computed) and without (values given)
    for with_h in (True, False):
        ws = X.Windows()
        hw = ws.inp("h", t["h"]) if with_h else None
        ww, bw = ws.inp("w", t["w"]), ws.inp("b", t["b"], skew=4)
        rew, dn, to = ws.inp("rewards", t["rew"], skew=4), ws.inp("dones", t["dones"].to(U8), skew=4), ws.inp("time_outs", t["touts"].to(U8), skew=4)
        va = ws.out("values_all", ((T + 1) * N,), skew=4)
        if not with_h:
            va.copy_(vall)
        adv, ret = ws.out("advantages", (T, N), skew=4), ws.out("returns", (T, N), skew=4)
        sums = ws.out("sums", (3,), F64, skew=8)                       # WRITTEN: starts as poison
        scratch = ws.out("scratch", (3 * ((N + 15) // 16) + 1,), F64, skew=8)
        scratch[-1] = 0.0                                              # the caller's one-time zero; the records in front of it stay poison
        for rep in range(2):                                           # (the second call finds the ticket as the first one left it)
            rew.copy_(t["rew"])
            call("bg_critic_values_gae", T, N, p(hw), p(ww), p(bw), p(rew), p(dn), p(to), GAMMA, LAM, p(va), p(adv), p(ret), p(sums), p(scratch))
            ws.check(f"bg_critic_values_gae T={T} N={N} h={with_h} call {rep}")
            assert float(scratch[-1]) == 0.0, "the ticket element must be left zero"
        for k, x in (("values_all", va), ("advantages", adv), ("returns", ret), ("sums", sums)):
            X.assert_fully_written(x, k)
        close(va, vall.double(), 2e-5, f"bg_critic_values_gae values_all T={T} N={N}")
        r2, a2, ret2 = gae_ref(t["rew"], t["dones"], t["touts"], va[: T * N].view(T, N), va[T * N :])
        assert torch.equal(rew, r2.float())
        close(adv, a2, 2e-5, "bg_critic_values_gae advantages")
        close(ret, ret2, 2e-5, "bg_critic_values_gae returns")
        check_sums(sums, adv)
        if not with_h:  # "advantages [bit-identical] to bg_gae" on the same values
            assert torch.equal(adv, adv0) and torch.equal(ret, ret0)


@pytest.mark.parametrize("T,N", GAE_SHAPES)
def test_gae_norm_and_denormalize_outputs_and_ticket(T, N):
    """bg_critic_values_gae_norm: "sums float64 [6] WRITTEN", "scratch: float64 [6 * ceil(N / 16) + 1], its last element zero-initialised once"; values_all
    keeps u; bg_value_denormalize: values [rows] in place, "one rounding per value"."""
    t = gae_inputs(T, N, 37 * T + N)
    stats = torch.tensor([0.7, 2.5, 1.0 / 2.5], dtype=F32, device=DEV)  # (m, sigma, 1 / sigma)
    m, sigma, inv = (float(x) for x in stats)
    u_ref = t["h"].double() @ t["w"].double() + t["b"].double()
    for with_h in (True, False):
        ws = X.Windows()
        hw = ws.inp("h", t["h"]) if with_h else None
        ww, bw, sw = ws.inp("w", t["w"]), ws.inp("b", t["b"], skew=4), ws.inp("value_stats", stats, skew=4)
        rew, dn, to = ws.inp("rewards", t["rew"], skew=4), ws.inp("dones", t["dones"].to(U8), skew=4), ws.inp("time_outs", t["touts"].to(U8), skew=4)
        va = ws.out("values_all", ((T + 1) * N,), skew=4)
        if not with_h:
            va.copy_(u_ref.float())
        adv, ret = ws.out("advantages", (T, N), skew=4), ws.out("returns", (T, N), skew=4)
        sums = ws.out("sums", (6,), F64, skew=8)
        scratch = ws.out("scratch", (6 * ((N + 15) // 16) + 1,), F64, skew=8)
        scratch[-1] = 0.0
        for rep in range(2):
            rew.copy_(t["rew"])
            call("bg_critic_values_gae_norm", T, N, p(hw), p(ww), p(bw), p(rew), p(dn), p(to), GAMMA, LAM, p(va), p(adv), p(ret), p(sw), p(sums), p(scratch))
            ws.check(f"bg_critic_values_gae_norm T={T} N={N} h={with_h} call {rep}")
            assert float(scratch[-1]) == 0.0, "the ticket element must be left zero"
        for k, x in (("values_all", va), ("advantages", adv), ("returns", ret), ("sums", sums)):
            X.assert_fully_written(x, k)
        close(va, u_ref, 2e-5, "bg_critic_values_gae_norm values_all (u)")
        # bg_value_denormalize on a copy of u, in a window of exactly (T + 1) N values: v = fmaf(sigma, u, m), one rounding
        ws2 = X.Windows()
        v = ws2.inp("values", va.clone(), skew=4)
        call("bg_value_denormalize", (T + 1) * N, p(v), p(ws2.inp("value_stats", stats, skew=4)))
        ws2.check("bg_value_denormalize")
        assert torch.equal(v, (sigma * va.double() + m).float())
        r2, a2, R = gae_ref(t["rew"], t["dones"], t["touts"], v[: T * N].view(T, N), v[T * N :])
        assert torch.equal(rew, r2.float())
        close(adv, a2, 2e-5, "bg_critic_values_gae_norm advantages")
        close(ret, (R - m) * inv, 2e-5, "bg_critic_values_gae_norm returns")
        check_sums(sums, adv, v[: T * N].view(T, N) + adv)  # (torch's fp32 add: the one rounding of R)


# ---------------------------------------------------------------------------------------------------------------------------- reductions and the optimiser
B1, B2, EPS, MAX_NORM, LR = 0.9, 0.999, 1e-8, 1.0, 1e-3


def reduce_problem(ws, tag, groups, record, outs, n_stat=0, n_ls=0, gls=None, stats=None, seed=0):
    """a bg_reduce_problem on a window of exactly [groups][record] floats (+ [n_stat][groups] float64 behind them); outs: (pointer, n) x up to 3"""
    L = _L()
    g = gen(seed)
    n_out = sum(n for _, n in outs)
    part = ws.out(tag + "partial", (groups * record + 2 * n_stat * groups,), skew=16 if n_stat else 4, band=max(X.MIN_BAND, record * 4))
    part[: groups * record] = randn(g, groups * record)
    sd = None
    if n_stat:
        sd = part[groups * record :].view(F64).view(n_stat, groups)
        sd.copy_(torch.randn(n_stat, groups, generator=g, dtype=F64))
    q = L.ReduceProblem()
    q.partial, q.groups, q.record, q.n_out = part.data_ptr(), groups, record, n_out
    for k, (ptr, n) in enumerate(outs):
        q.out[k], q.n[k] = ptr, n
    q.stat_base, q.n_stat, q.n_ls, q.stat_skip, q.entropy_coef = groups * record, n_stat, n_ls, 0, ENT_COEF
    q.grad_logstd, q.stats = (gls.data_ptr() if gls is not None else None), (stats.data_ptr() if stats is not None else None)
    ref = part[: groups * record].view(groups, record)[:, :n_out].double().sum(0)
    return q, ref, sd


N_FLAT, LS_OFF = 339, 327  # [0, 45): three outputs of one reduction; [45, 327): a [6][47] first-layer matrix; [327, 339): the log-std.  339 % 4 == 3


def flat_windows(ws, seed, grads=None, grads_skew=4):
    """grads_skew: 16 for bg_optimizer_step alone ("grads 16-byte aligned": its norm pass reads float4); no other form is promised an alignment"""
    g = gen(seed)
    t = dict(params=ws.inp("params", randn(g, N_FLAT), skew=4), grads=ws.out("grads", (N_FLAT,), skew=grads_skew),
             m=ws.inp("exp_avg", randn(g, N_FLAT, scale=0.1), skew=4), v=ws.inp("exp_avg_sq", randn(g, N_FLAT).abs() * 0.01, skew=4),
             lr=ws.inp("lr_device", torch.tensor([LR], device=DEV), skew=4))
    t["grads"].zero_()
    if grads is not None:
        t["grads"].copy_(grads)
    return t


def adam_ref(params, grads, m, v, step, sqnorm=None):
    """float64: clip_grad_norm_(max 1) + Adam with the library's bias corrections"""
    g = grads.double()
    coef = min(MAX_NORM / (float((g**2).sum().sqrt()) + 1e-6), 1.0)
    g = g * coef
    m2, v2 = B1 * m.double() + (1 - B1) * g, B2 * v.double() + (1 - B2) * g * g
    bc1, bc2s = 1.0 - B1**step, (1.0 - B2**step) ** 0.5
    return params.double() - LR / bc1 * m2 / (v2.sqrt() / bc2s + EPS), m2, v2


def check_adam(t, before, grads, step, what):
    p_ref, m_ref, v_ref = adam_ref(before["params"], grads, before["m"], before["v"], step)
    for k, ref in (("params", p_ref), ("m", m_ref), ("v", v_ref)):  # test_gpu_ppo.py: rtol 1e-5, atol 1e-6 against torch's Adam
        assert tuple(t[k].shape) == (N_FLAT,)
        assert torch.allclose(t[k].double(), ref, rtol=1e-5, atol=1e-6), (what, k, (t[k].double() - ref).abs().max().item())


def test_reduce_group_and_tail_sums_on_odd_flat_buffers():
    """bg_reduce_group and bg_update_tail_sums: out[0..2] exactly n[0..2] floats inside a flat buffer of 45 floats (n % 4 != 0, the pieces at odd offsets),
    the float64 statistics added to grad_logstd [1] and stats [2] exactly; norm_scratch float64 [BG_TAIL_MAX_BLOCKS], one slot per block."""
    L = _L()
    got = []
    for form in ("bg_reduce_group", "bg_update_tail_sums"):
        ws = X.Windows()
        flat = ws.out("flat", (45,), skew=4)
        gls, stats = ws.zeros("grad_logstd", (1,), F64, skew=8), ws.zeros("stats", (2,), F64, skew=8)
        q, ref, sd = reduce_problem(ws, "", 7, 48, [(flat.data_ptr(), 37), (flat.data_ptr() + 4 * 37, 5), (flat.data_ptr() + 4 * 42, 3)], 3, 1, gls, stats, seed=3)
        arr = (L.ReduceProblem * 1)(q)
        if form == "bg_reduce_group":
            call(form, arr, 1)
        else:
            norm = _tail_norm(ws)
            call(form, None, 0, arr, 1, p(norm))
        ws.check(form)
        X.assert_fully_written(flat, "flat")
        close(flat, ref, 1e-4, f"{form}: sums over 7 records")
        assert abs(float(gls[0]) - (float(sd[0].sum()) + ENT_COEF)) < 1e-12 and torch.allclose(stats, sd[1:].sum(1), rtol=1e-12, atol=1e-12)
        if form == "bg_update_tail_sums":  # blocks: ceil(45 / 16) of outputs + 3 of statistics; slot sum = the squares written
            assert bool(X.is_poison(norm[6:]).all()) and abs(float(norm[:6].sum()) - float((flat.double() ** 2).sum())) <= 1e-12 * float((flat.double() ** 2).sum())
        got.append(flat.clone())
    assert torch.equal(got[0], got[1])


def mirrors_of(ws):
    """two copies of the [6][47] matrix at offset 45: row-major with ld = 64 (a first layer's zero-padded input columns: "the padding is not touched") and
    transposed with ld = 8"""
    L = _L()
    a, b = ws.out("mirror ld=64", (6, 64), skew=4), ws.out("mirror transposed", (47, 8), skew=4)
    arr = (L.ParamMirror * 2)(L.ParamMirror(45, 6, 47, 0, 64, 0, a.data_ptr()), L.ParamMirror(45, 6, 47, 1, 8, 0, b.data_ptr()))
    return arr, a, b


def check_mirrors(t, a, b, what):
    Wn = t["params"][45:327].view(6, 47)
    assert torch.equal(a[:, :47], Wn) and bool(X.is_poison(a[:, 47:]).all()), f"{what}: row-major mirror"
    assert torch.equal(b[:, :6], Wn.t()) and bool(X.is_poison(b[:, 6:]).all()), f"{what}: transposed mirror"


def stats_windows(ws):
    s = dict(gls=ws.inp("grad_logstd", torch.linspace(-0.3, 0.3, 12, dtype=F64, device=DEV), skew=8),
             stats=ws.inp("stats", torch.tensor([3.0, -1.0, 0.5, 20.0, 9.0], dtype=F64, device=DEV), skew=8),
             acc=ws.inp("stats_acc", torch.arange(5, dtype=F64, device=DEV), skew=8), last=ws.out("stats_last", (5,), F64, skew=8))
    return s


def check_stats(s, t, what):
    """kl = stats[4] / 100 = 0.09 > 2 x 0.01: the learning rate goes down by 1.5; stats_last = stats, stats_acc += stats, stats = 0, grad_logstd = 0"""
    assert torch.equal(s["last"], torch.tensor([3.0, -1.0, 0.5, 20.0, 9.0], dtype=F64, device=DEV)), what
    assert torch.equal(s["acc"], torch.tensor([3.0, 0.0, 2.5, 23.0, 13.0], dtype=F64, device=DEV)), what
    assert bool((s["stats"] == 0).all()) and bool((s["gls"] == 0).all()), what
    assert abs(float(t["lr"][0]) - LR / 1.5) <= 1e-6 * LR, what


def test_update_tail_flat_buffers_sync_and_mirrors():
    """bg_update_tail on flat buffers of n = 339 floats (n % 4 == 3): params / grads / exp_avg / exp_avg_sq [n] exactly, "norm_scratch: float64
    [BG_TAIL_MAX_BLOCKS]", "sync: uint32 [1] ... (the launch leaves it zero)", the mirrors inside rows x ld with the padding columns untouched."""
    L = _L()
    ws = X.Windows()
    t, s = flat_windows(ws, 5), stats_windows(ws)
    base = t["grads"].data_ptr()
    q1, r1, _ = reduce_problem(ws, "heads.", 7, 48, [(base, 37), (base + 4 * 37, 5), (base + 4 * 42, 3)], seed=6)
    q2, r2, _ = reduce_problem(ws, "matrix.", 3, 282, [(base + 4 * 45, 282)], seed=7)
    sync, norm = ws.zeros("sync", (1,), I32, skew=4), _tail_norm(ws)
    mir, ma, mb = mirrors_of(ws)
    before = {k: t[k].clone() for k in ("params", "m", "v")}
    gls0 = s["gls"].clone()
    for rep in range(2):  # the second call finds `sync` as the first one left it
        for k in before:
            t[k].copy_(before[k])
        s["gls"].copy_(gls0), s["stats"].copy_(torch.tensor([3.0, -1.0, 0.5, 20.0, 9.0], dtype=F64, device=DEV)), s["acc"].copy_(torch.arange(5, dtype=F64, device=DEV))
        t["lr"].fill_(LR)
        call("bg_update_tail", None, 0, (L.ReduceProblem * 2)(q1, q2), 2, N_FLAT, p(t["params"]), p(t["grads"]), p(t["m"]), p(t["v"]), p(t["lr"]), 3, B1, B2, EPS, MAX_NORM,
             p(s["gls"]), LS_OFF, 12, p(s["stats"]), p(s["acc"]), p(s["last"]), 5, 4, 100.0, 0.01, 1e-5, 1e-2, p(sync), p(norm), C.addressof(mir), 2)
        ws.check(f"bg_update_tail call {rep}")
        assert int(sync[0]) == 0, "sync must be left zero"
    grads_ref = torch.cat([r1, r2, gls0.float().double()])
    close(t["grads"], grads_ref, 1e-4, "bg_update_tail: the gradient it summed")
    check_adam(t, before, t["grads"], 3, "bg_update_tail")
    check_mirrors(t, ma, mb, "bg_update_tail")
    check_stats(s, t, "bg_update_tail")


def test_optimizer_step_and_adam_step_flat_buffers_and_ticket():
    """bg_optimizer_step: the same flat buffers, "ticket: one zero-initialised uint32" left zero, mirrors; bg_adam_step: "gnorm_scratch [1] device float64"."""
    g = gen(11)
    grads = randn(g, N_FLAT, scale=0.2)
    ws = X.Windows()
    t, s = flat_windows(ws, 5, grads, grads_skew=16), stats_windows(ws)
    ticket = ws.zeros("ticket", (1,), I32, skew=4)
    mir, ma, mb = mirrors_of(ws)
    before = {k: t[k].clone() for k in ("params", "m", "v")}
    gls0 = s["gls"].clone()
    call("bg_optimizer_step", N_FLAT, p(t["params"]), p(t["grads"]), p(t["m"]), p(t["v"]), p(t["lr"]), 3, B1, B2, EPS, MAX_NORM, p(s["gls"]), LS_OFF, 12, p(s["stats"]),
         p(s["acc"]), p(s["last"]), 5, 4, 100.0, 0.01, 1e-5, 1e-2, p(ticket), C.addressof(mir), 2)
    ws.check("bg_optimizer_step")
    assert int(ticket[0]) == 0, "ticket must be left zero"
    want = grads.clone()
    want[LS_OFF:] = gls0.float()
    assert torch.equal(t["grads"], want)  # the log-std slice written, nothing else
    check_adam(t, before, want, 3, "bg_optimizer_step")
    check_mirrors(t, ma, mb, "bg_optimizer_step")
    check_stats(s, t, "bg_optimizer_step")
    # bg_adam_step
    ws = X.Windows()
    t = flat_windows(ws, 5, grads)
    gnorm = ws.out("gnorm_scratch", (1,), F64, skew=8)
    before = {k: t[k].clone() for k in ("params", "m", "v")}
    call("bg_adam_step", N_FLAT, p(t["params"]), p(t["grads"]), p(t["m"]), p(t["v"]), p(t["lr"]), 3, B1, B2, EPS, MAX_NORM, p(gnorm))
    ws.check("bg_adam_step")
    assert torch.equal(t["grads"], grads) and abs(float(gnorm[0]) - float((grads.double() ** 2).sum())) <= 1e-12 * float((grads.double() ** 2).sum())
    check_adam(t, before, grads, 3, "bg_adam_step")


# ---------------------------------------------------------------------------------------------------------------------------- observation normalisation
@pytest.mark.parametrize("ca,sa,cb,sb", [(47, 47, 14, 14), (47, 50, 14, 17), (141, 141, 0, 0), (512, 512, 201, 201)])
@pytest.mark.parametrize("rows", [1, 31, 129, 1025])
def test_obs_moments_scratch(rows, ca, sa, cb, sb):
    """bg_obs_moments: scratch "float64, at least BG_OBS_MOMENTS_MAX_GROUPS * 2 * (cols_a + cols_b) values" -- exactly that many here; sum / sumsq float64
    [cols_a + cols_b] overwritten; the columns of a row between a block's columns and its stride are never read (they hold NaN)."""
    L = _L()
    g = gen(rows + ca + cb)
    Cn = ca + cb
    x = randn(g, rows, Cn) * (10.0 ** torch.linspace(-2, 2, Cn, device=DEV)) + 0.5
    ws = X.Windows()
    a = ws.out("a", (rows, sa), skew=4, band=max(X.MIN_BAND, 128 * sa * 4))
    a[:, :ca] = x[:, :ca]
    b = None
    if cb:
        b = ws.out("b", (rows, sb), skew=4, band=max(X.MIN_BAND, 128 * sb * 4))
        b[:, :cb] = x[:, ca:]
    s, ss = ws.out("sum", (Cn,), F64, skew=8), ws.out("sumsq", (Cn,), F64, skew=8)
    scratch = ws.out("scratch", (L.OBS_MOMENTS_MAX_GROUPS * 2 * Cn,), F64, skew=8, band=2 * Cn * 8)  # one more record: [2][cols] float64
    call("bg_obs_moments", rows, p(a), ca, sa, p(b), cb, sb, p(s), p(ss), p(scratch))
    ws.check(f"bg_obs_moments rows={rows} {ca}+{cb}")
    X.assert_fully_written(s, "sum")
    X.assert_fully_written(ss, "sumsq")
    x64 = x.double()
    # test_gpu_obs_norm.py's bound: M eps_f64 sum |x| and M eps_f64 sum x^2, whatever the fixed order
    es, ess = (s - x64.sum(0)).abs(), (ss - (x64 * x64).sum(0)).abs()
    assert tuple(es.shape) == (Cn,) and bool((es <= rows * 2.0**-52 * x64.abs().sum(0)).all()) and bool((ess <= rows * 2.0**-52 * (x64 * x64).sum(0)).all())


@pytest.mark.parametrize("cols,src_stride,dst_cols,dst_stride,col0", [(47, 47, 64, 64, 0), (14, 20, 14, 17, 47), (61, 61, 64, 70, 3), (1, 1, 1, 1, 0)])
@pytest.mark.parametrize("rows", [1, 31, 129, 1025])
def test_obs_normalize_columns(rows, cols, src_stride, dst_cols, dst_stride, col0):
    """bg_obs_normalize: "dst[r][c] = (src[r][c] - mean[col0 + c]) * inv_std[col0 + c] for c < cols and 0 for cols <= c < dst_cols", the subtract and the
    multiply each rounded: torch's fp32 sub and mul, bit for bit; columns [dst_cols, dst_stride) of dst are untouched; "src is not written"."""
    g = gen(rows + cols + col0)
    x = randn(g, rows, cols)
    mean, inv = randn(g, col0 + cols), randn(g, col0 + cols).abs() + 0.5
    ws = X.Windows()
    src = ws.out("src", (rows, src_stride), skew=4, band=max(X.MIN_BAND, 128 * src_stride * 4))
    src[:, :cols] = x
    src0 = src.clone()
    dst = ws.out("dst", (rows, dst_stride), skew=4, band=max(X.MIN_BAND, 128 * dst_stride * 4))
    call("bg_obs_normalize", rows, cols, p(src), src_stride, p(dst), dst_cols, dst_stride, p(ws.inp("mean", mean, skew=4)), p(ws.inp("inv_std", inv, skew=4)), col0)
    ws.check(f"bg_obs_normalize rows={rows} cols={cols}")
    assert torch.equal(dst[:, :cols], (x - mean[col0:]) * inv[col0:])
    assert bool((dst[:, cols:dst_cols] == 0).all()) and bool(X.is_poison(dst[:, dst_cols:]).all())
    assert torch.equal(src.view(torch.int32), src0.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------- row copies
@pytest.mark.parametrize("n", [1, 2, 31, 129, 1025])
def test_perm_fill_writes_n_values(perm_lib, n):  # noqa: F811
    """bg_perm_fill: "perm: int32 [n]" exactly, the permutation the key names (the host harness evaluates the same header, csrc/bg_perm.h)."""
    for seed, update, epoch in ((42, 0, 1), ((5 << 32) | 9, 123456, 19)):
        ws = X.Windows()
        perm = ws.out("perm", (n,), I32, skew=4)
        call("bg_perm_fill", n, seed, update, epoch, p(perm))
        ws.check(f"bg_perm_fill n={n}")
        X.assert_fully_written(perm, "perm")
        assert np.array_equal(perm.cpu().numpy(), host_perm(perm_lib, n, seed, update, epoch))
        assert torch.equal(torch.sort(perm).values, torch.arange(n, dtype=I32, device=DEV))


@pytest.mark.parametrize("skew", [4, 16])
@pytest.mark.parametrize("rows,src_rows", [(1, 1), (31, 40), (129, 129), (1025, 700)])
def test_gather_rows_widths_and_bad_indices(rows, src_rows, skew):
    """bg_gather_rows: "dst [rows][width]" for widths 1, 4 and 47 in ONE launch; "perm: int32 [rows] with values in [0, src_rows); a value outside leaves
    its destination row as it was (never read out of bounds)".  skew 16: the width-4 stream moves 16 bytes per thread; skew 4: element by element."""
    L = _L()
    g = gen(rows + src_rows)
    perm = torch.randint(0, src_rows, (rows,), generator=g, dtype=I32)
    bad = torch.zeros(rows, dtype=torch.bool)
    if rows > 2:
        perm[1], perm[rows - 1], bad[1], bad[rows - 1] = -1, src_rows, True, True
    ws = X.Windows()
    pw = ws.inp("perm", perm.to(DEV), skew=4)
    arr, keep = (L.GatherStream * 3)(), []
    for k, width in enumerate((1, 4, 47)):
        src = ws.inp(f"src{width}", randn(g, src_rows, width), skew=skew, band=max(X.MIN_BAND, 128 * width * 4))
        dst = ws.out(f"dst{width}", (rows, width), skew=skew, band=max(X.MIN_BAND, 128 * width * 4))
        arr[k].src, arr[k].dst, arr[k].width = src.data_ptr(), dst.data_ptr(), width
        keep.append((src, dst))
    call("bg_gather_rows", rows, src_rows, p(pw), arr, 3)
    ws.check(f"bg_gather_rows rows={rows}")
    ok = (~bad).to(DEV)
    for src, dst in keep:
        want = src[perm.clamp(0, src_rows - 1).long().to(DEV)]
        assert torch.equal(dst[ok], want[ok]) and bool(X.is_poison(dst[~ok]).all())


@pytest.mark.parametrize("cols", [1, 4, 47])
@pytest.mark.parametrize("rows", ROWS_ANY)
def test_mirror_rows_writes_rows_times_cols(rows, cols):
    """bg_mirror_rows: "y [rows][cols] = the rows of x [rows][cols] mirrored: y[r][c] = sign[c] x[r][src[c]] (src[c] = -1: 0)".  Exact."""
    g = gen(rows + cols)
    x = randn(g, rows, cols)
    src = list(reversed(range(cols)))
    sign = [1.0 if c % 3 else -1.0 for c in range(cols)]
    if cols > 2:
        src[2] = -1
    ws = X.Windows()
    xw, y = ws.inp("x", x, skew=4), ws.out("y", (rows, cols), skew=4, band=max(X.MIN_BAND, 128 * cols * 4))
    call("bg_mirror_rows", rows, cols, (C.c_int32 * cols)(*src), (C.c_float * cols)(*sign), p(xw), p(y))
    ws.check(f"bg_mirror_rows rows={rows} cols={cols}")
    X.assert_fully_written(y, "y")
    want = x[:, [max(s, 0) for s in src]] * torch.tensor(sign, device=DEV)
    if cols > 2:
        want[:, 2] = 0.0
    assert torch.equal(y, want)


@pytest.mark.parametrize("cols", [4, 48])
@pytest.mark.parametrize("T,N", GAE_SHAPES)
def test_partner_rows_writes_T_N_rows(T, N, cols):
    """bg_partner_rows: "every element of y's T N rows is written, nothing past them"; x, x_last and y 16-byte aligned; "cols a multiple of 4": 4 and 48
    stand for the row copies' widths 4 and 47.  NEXT: bit-exact copies of the next step's row (x_last behind the last step), of the row itself at a done /
    time-out.  INTERPOLATE: y[r][c] = fma(u_r, x+[r][c] - x[r][c], x[r][c]) with the host generator's u_r (test_smoothness.partner_draw: Philox on the
    header's key and counter): one rounding of the exact x + u fl(x+ - x), held to half an ulp of y against float64 as test_gpu_smoothness.py holds it."""
    L = _L()
    g = gen(T + N + cols)
    x, xl = randn(g, T, N, cols), randn(g, N, cols)
    dn, to = (torch.rand(T, N, generator=g) < 0.2).to(DEV), (torch.rand(T, N, generator=g) < 0.2).to(DEV)
    nxt = torch.cat((x[1:], xl[None]), 0)
    cut = (dn | to)[..., None]
    for mode in (L.PARTNER_NEXT, L.PARTNER_INTERPOLATE):
        ws = X.Windows()
        y = ws.out("y", (T, N, cols), band=max(X.MIN_BAND, 128 * cols * 4))
        call("bg_partner_rows", T, N, cols, p(ws.inp("x", x.view(T * N, cols))), p(ws.inp("x_last", xl)), p(ws.inp("dones", dn.to(U8), skew=4)),
             p(ws.inp("time_outs", to.to(U8), skew=4)), mode, 42, 3, 1, p(y))
        ws.check(f"bg_partner_rows T={T} N={N} cols={cols} mode={mode}")
        X.assert_fully_written(y, "y")
        if mode == L.PARTNER_NEXT:
            assert torch.equal(y, torch.where(cut, x, nxt))
        else:
            u = torch.from_numpy(partner_draw(42, T * N, 3, 1).reshape(T, N, 1)).to(DEV)
            assert u.dtype == F32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
            exact = x.double() + u.double() * (nxt - x).double()  # (the fp32 difference, then exact in float64: 24 x 24 bits and one add)
            assert torch.equal(y[cut.expand_as(y)], x[cut.expand_as(x)])  # a cut row is x itself, bit for bit
            live = (~cut).expand_as(y)
            ulp = torch.from_numpy(np.spacing(np.abs(y.cpu().numpy()))).to(DEV).double()
            err = ((y.double() - exact).abs() / ulp)[live]
            print(f"bg_partner_rows interpolate T={T} N={N} cols={cols}: {int(live.sum())} live elements, max |y - exact| {float(err.max()) if err.numel() else 0.0:.4f} ulp of y")
            assert err.numel() == 0 or float(err.max()) <= 0.5 + 1e-6  # test_gpu_smoothness.py's bound on the kernel's own contract


# ---------------------------------------------------------------------------------------------------------------------------- row outputs of the loss and the samplers
@pytest.mark.parametrize("B", ROWS_ANY)
def test_ppo_loss_and_logp_row_outputs(B):
    """bg_ppo_loss: grad_mu [B][12], grad_values [B], grad_logstd [12] and stats [5] float64 (atomic, caller zeroes); bg_gaussian_logp: logp [B]."""
    t = head_inputs(B, B, 29 * B)
    mu = (t["h"] @ t["W"].t() + t["b"]).contiguous()
    ws = X.Windows()
    w = {k: ws.inp(k, t[k], skew=8 if t[k].dtype == F64 else 4) for k in ("logstd", "actions", "old_mu", "old_logstd", "old_logp", "adv", "adv_stats", "values", "returns")}
    muw = ws.inp("mu", mu, skew=4)
    gmu, gv = ws.out("grad_mu", (B, 12), skew=4), ws.out("grad_values", (B,), skew=4)
    gls, st = ws.zeros("grad_logstd", (12,), F64, skew=8), ws.zeros("stats", (5,), F64, skew=8)
    call("bg_ppo_loss", B, 12, p(muw), p(w["logstd"]), p(w["actions"]), p(w["old_mu"]), p(w["old_logstd"]), p(w["old_logp"]), p(w["adv"]), p(w["adv_stats"]),
         p(w["values"]), p(w["returns"]), E_CLIP, BOUND_COEF, ENT_COEF, p(gmu), p(gv), p(gls), p(st))
    logp = ws.out("logp", (B,), skew=4)
    call("bg_gaussian_logp", B, 12, p(muw), p(w["logstd"]), p(w["actions"]), p(logp))
    ws.check(f"bg_ppo_loss / bg_gaussian_logp B={B}")
    for k, x in (("grad_mu", gmu), ("grad_values", gv), ("logp", logp)):
        X.assert_fully_written(x, k)
    m64, ls = mu.double().clone().requires_grad_(), t["logstd"].double().clone().requires_grad_()
    surr, bound, ent, kl = ppo_terms(t, m64, ls)
    (surr.mean() + BOUND_COEF * bound.mean() + ENT_COEF * ent).backward()
    verr = t["values"].double() - t["returns"].double()
    # test_gpu_head.py's bounds for what passes through the ratio's exp(): 2e-3 of the largest entry; statistics 1e-4
    assert rel(gmu, m64.grad, "grad_mu") < 2e-3 and rel(gls, ls.grad, "grad_logstd") < 2e-3
    assert rel(gv, 2.0 * verr / B, "grad_values") < 2e-5
    want = torch.stack([(verr**2).sum(), surr.sum(), bound.sum(), ent * B, kl.sum()]).detach()
    assert rel(st, want, "stats") < 1e-4
    ref_lp = (-0.5 * ((t["actions"].double() - mu.double()) / t["logstd"].double().exp()) ** 2 - t["logstd"].double() - HALF_LOG_2PI).sum(-1)
    assert torch.allclose(logp.double(), ref_lp, rtol=0, atol=2e-4)  # test_gpu_ppo.py: atol 2e-4 on the log-prob


@pytest.mark.parametrize("n", [1, 37])
def test_actor_samplers_write_n_rows(n):
    """bg_actor_pack: `packed` exactly BG_ACTOR_PACKED_FLOATS floats, 16-byte aligned; bg_actor_sample and bg_actor_sample_mlp: mu / actions [n][12] exactly
    (n = 1, 37: below and across the samplers' 16-row workgroups).  With logstd = 0, actions - mu is the header's draw, Philox(seed, row, counter, RS_ACTOR
    + group of 4 actions), up to one rounding: against the oracle's generator at test_gpu_action_noise.py's bound (4 x its measured 2.27e-6 + one ulp of
    the largest |action|)."""
    L = _L()
    g = gen(41 + n)
    dims = [(256, 47), (128, 256), (128, 128), (12, 128)]
    Ws, bs = [randn(g, o, i, scale=1.0 / i**0.5) for o, i in dims], [randn(g, o, scale=0.1) for o, _ in dims]
    logstd, obs = torch.zeros(12, device=DEV), randn(g, n, 47)
    ref = obs.double()
    for k, (W, b) in enumerate(zip(Ws, bs)):
        ref = ref @ W.double().t() + b.double()
        ref = elu(ref) if k < 3 else ref
    ws = X.Windows()
    Ww = [ws.inp(f"w{k}", W, skew=16 if k else 4) for k, W in enumerate(Ws)]  # header: "Weight matrices after the first 16-byte aligned"
    bw = [ws.inp(f"b{k}", b, skew=4) for k, b in enumerate(bs)]
    lw, ow = ws.inp("logstd", logstd, skew=4), ws.inp("obs", obs, skew=4)
    packed = ws.out("packed", (L.ACTOR_PACKED_FLOATS,), skew=16)
    call("bg_actor_pack", p(Ww[0]), p(bw[0]), p(Ww[1]), p(bw[1]), p(Ww[2]), p(bw[2]), p(Ww[3]), p(bw[3]), p(lw), p(packed))
    mu1, a1 = ws.out("mu", (n, 12), skew=4), ws.out("actions", (n, 12), skew=4)
    call("bg_actor_sample", n, p(ow), p(packed), 5, 3, p(mu1), p(a1))
    descs = (L.MlpLayerDesc * 4)(*[L.MlpLayerDesc(p(W), p(b), i, o) for W, b, (o, i) in zip(Ww, bw, dims)])
    mu2, a2 = ws.out("mu (mlp)", (n, 12), skew=4), ws.out("actions (mlp)", (n, 12), skew=4)
    call("bg_actor_sample_mlp", n, p(ow), 4, descs, p(lw), 5, 3, p(mu2), p(a2))
    ws.check(f"bg_actor_pack / bg_actor_sample / bg_actor_sample_mlp n={n}")
    for k, x in (("packed", packed), ("mu", mu1), ("actions", a1), ("mu (mlp)", mu2), ("actions (mlp)", a2)):
        X.assert_fully_written(x, k)
    close(mu1, ref, 2e-5, f"bg_actor_sample mu n={n}")
    close(mu2, ref, 2e-5, f"bg_actor_sample_mlp mu n={n}")
    draw = torch.from_numpy(action_noise(5, np.arange(n), 3)).to(DEV)
    for name, mu, act in (("bg_actor_sample", mu1, a1), ("bg_actor_sample_mlp", mu2, a2)):
        err, bound = float(((act - mu) - draw).abs().max()), noise_bound(float(act.abs().max()))
        print(f"{name} n={n}: {act.numel()} draws, max |(actions - mu) - oracle draw| {err:.3e}, bound {bound:.3e}")
        assert tuple(act.shape) == tuple(draw.shape) and err <= bound, (name, err, bound)
