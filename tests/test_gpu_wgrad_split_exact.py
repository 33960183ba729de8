"""The split weight-gradient launch on operands whose sums are exact in every order: G and A hold integers in [-8, 8], so every bf16 plane but the
first is zero, every product is an integer of at most 64 and every partial sum stays below 64 M < 2^24 -- fp32 holds all of them exactly and the launch
must EQUAL G^T A computed in float64, with no tolerance.  What this pins is the kernel's copies into LDS: which rows land where, in which buffer, how
many of them a wave waits for, and the zeros a sub-range multiplies past its end.  The operands are views into the middle of NaN-filled allocations
(a copy that reads a row too many or too few poisons the sum), the outputs and the partial-tile scratch start as NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64  # rows of NaN in front of and behind every operand

# (C_out, C_in, real C_in, tiles per workgroup): the four shapes of the kernel, the 64-wide one with both of its real widths
SHAPES = [(256, 256, 256, 4), (128, 256, 256, 2), (128, 128, 128, 1), (256, 64, 61, 2), (256, 64, 47, 2)]


def _problem(arr, k, keep, M, co, ci, cr, slices, tw, gen):
    def inside(cols, real):
        big = torch.full(((M + 2 * PAD) * cols,), float("nan"), device=DEV)
        v = big[PAD * cols : (PAD + M) * cols].view(M, cols)
        x = torch.randint(-8, 9, (M, cols), generator=gen).float()
        x[:, real:] = 0.0  # the zero padding of the 64-wide first layers
        v.copy_(x.to(DEV))
        return big, v

    gbig, G = inside(co, co)
    abig, A = inside(ci, cr)
    dW = torch.full((co, cr), float("nan"), device=DEV)
    sc = torch.full((slices * co * ci,), float("nan"), device=DEV)
    keep.append((G, A, dW, sc, gbig, abig, cr))
    arr[k].G, arr[k].A, arr[k].dW, arr[k].scratch = G.data_ptr(), A.data_ptr(), dW.data_ptr(), sc.data_ptr()
    arr[k].M, arr[k].C_out, arr[k].C_in, arr[k].C_in_real, arr[k].slices, arr[k].tiles_per_workgroup = M, co, ci, cr, slices, tw


def _check(keep):
    for G, A, dW, _, _, _, cr in keep:
        ref = G.double().t() @ A.double()[:, :cr]
        assert torch.equal(dW.double(), ref), (tuple(dW.shape), (dW.double() - ref).abs().max().item())


def _sub_range_blocks(M, slices, ks):
    """Blocks per sub-range, as the kernel partitions the batch (pairs of 16-row blocks dealt over slices x ks sub-ranges)."""
    nb2, w = M // 32, slices * ks
    return [2 * (nb2 * (i + 1) // w) - 2 * (nb2 * i // w) for i in range(w)]


@pytest.mark.parametrize("terms", [9, 6])
@pytest.mark.parametrize("case", ["two_blocks_each", "unequal_by_a_pair", "odd_lengths"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}r{s[2]}")
def test_split_weight_gradient_of_small_integers_is_exact(shape, case, terms):
    from booster_gym_amd import _lib

    lib, st = _lib.load(), _lib.current_stream_ptr()
    co, ci, cr, tw = shape
    ks = 4 // tw
    if case == "two_blocks_each":  # every sub-range is shorter than the prologue's depth of three (or two) blocks
        M, slices = 32 * ks * 3, 3
        assert set(_sub_range_blocks(M, slices, ks)) == {2}
    elif case == "unequal_by_a_pair":  # the last sub-range of the workgroup is a pair of blocks longer: the others multiply zeros meanwhile
        M, slices = 32 * (ks + 1), 1
        assert _sub_range_blocks(M, slices, ks) == [2] * (ks - 1) + [4]
    else:
        M, slices = 32 * 37, 5
        assert len(set(_sub_range_blocks(M, slices, ks))) > 1
    gen = torch.Generator().manual_seed(co * 7 + cr + M)
    arr, keep = (_lib.WgradProblem * 1)(), []
    _problem(arr, 0, keep, M, co, ci, cr, slices, tw, gen)
    _lib.check(lib.bg_mlp_weight_grad_group_split(arr, 1, terms, st), "bg_mlp_weight_grad_group_split")
    _check(keep)


def test_grouped_split_weight_gradients_of_small_integers_are_exact_and_repeat():
    """All five problems in ONE launch with the planner's slices at M = 4096 + 224, twice: exact, and the same bits both times."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import plan_wgrad_slices

    lib, st = _lib.load(), _lib.current_stream_ptr()
    M = 4096 + 224
    slices, tw = plan_wgrad_slices([(co, ci) for co, ci, _, _ in SHAPES], M, 256, share_rows=True)
    assert list(tw) == [s[3] for s in SHAPES]
    gen = torch.Generator().manual_seed(11)
    arr, keep = (_lib.WgradProblem * len(SHAPES))(), []
    for k, ((co, ci, cr, _), sl) in enumerate(zip(SHAPES, slices)):
        _problem(arr, k, keep, M, co, ci, cr, sl, tw[k], gen)
    _lib.check(lib.bg_mlp_weight_grad_group_split(arr, len(SHAPES), 9, st), "bg_mlp_weight_grad_group_split")
    _check(keep)
    first = [k[2].clone() for k in keep]
    for k in keep:
        k[2].fill_(float("nan"))
    _lib.check(lib.bg_mlp_weight_grad_group_split(arr, len(SHAPES), 9, st), "bg_mlp_weight_grad_group_split")
    assert all(torch.equal(a, k[2]) for a, k in zip(first, keep))
