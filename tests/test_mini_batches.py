"""runner.num_mini_batches without a GPU: the validation of the key, the permutation header compiled for the host (bijection, three uniformity
properties with bounds derived from the uniform law), and the update plan of a mini-batch's rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = os.environ.get("BG_SANITIZE", "0") == "1"
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
KEYS = [(0, 0, 0), (42, 0, 0), (42, 0, 1), (42, 1, 0), (7 + 1000003, 3, 4), (7 + 2 * 1000003, 3, 4), ((5 << 32) | 9, 123456, 19), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 24 - 1)]


@pytest.fixture(scope="module")
def perm_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("perm") / "libperm_harness.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared"] + (SAN_FLAGS if SANITIZE else ["-O2"]) + ["-o", so, os.path.join(HERE, "host_harness", "perm_harness.cpp")])
    lib = C.CDLL(so)
    lib.hh_perm_fill.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.hh_perm_fill.restype = None
    lib.hh_perm_half_bits.argtypes = [C.c_uint32]
    return lib


def host_perm(lib, n, seed, update, epoch):
    out = np.empty(n, dtype=np.int32)
    lib.hh_perm_fill(n, seed, update, epoch, out.ctypes.data)
    return out


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", over)


def test_validation_names_the_key_and_the_numbers():
    from booster_gym_amd.utils.runner import mini_batches

    cfg = _cfg()
    assert cfg["runner"]["num_mini_batches"] == 1 and mini_batches(cfg) == (False, 1)  # the shipped yaml: off
    del cfg["runner"]["num_mini_batches"]
    assert mini_batches(cfg) == (False, 1)  # absent: off
    cfg["runner"]["num_mini_batches"] = None
    assert mini_batches(cfg) == (False, 1)
    assert mini_batches(_cfg(**{"env.num_envs": 4096, "runner.num_mini_batches": 4})) == (True, 4)
    assert mini_batches(_cfg(**{"env.num_envs": 128, "runner.num_mini_batches": 2})) == (True, 2)
    for bad in (0, -2, 2.0, 1.5, "4", True, [2]):
        c = _cfg(**{"env.num_envs": 4096})
        c["runner"]["num_mini_batches"] = bad
        with pytest.raises(ValueError, match=r"runner\.num_mini_batches.*integer >= 1"):
            mini_batches(c)
    with pytest.raises(ValueError, match=r"runner\.num_mini_batches = 5 does not divide .*24 x 4096 = 98304"):
        mini_batches(_cfg(**{"env.num_envs": 4096, "runner.num_mini_batches": 5}))
    with pytest.raises(ValueError, match=r"runner\.num_mini_batches = 2 .*2400 / 2 = 1200 rows.*128"):  # (divides, but not into whole slabs)
        mini_batches(_cfg(**{"env.num_envs": 100, "runner.num_mini_batches": 2}))
    with pytest.raises(ValueError, match=r"runner\.num_mini_batches = 1024 .*98304 / 1024 = 96 rows.*128"):  # (below one slab)
        mini_batches(_cfg(**{"env.num_envs": 4096, "runner.num_mini_batches": 1024}))
    with pytest.raises(ValueError, match=r"runner\.num_mini_batches = 2 together with algorithm\.symmetry_loss"):
        mini_batches(_cfg(**{"env.num_envs": 128, "runner.num_mini_batches": 2, "algorithm.symmetry_loss": True}))
    assert mini_batches(_cfg(**{"env.num_envs": 128, "runner.num_mini_batches": 1, "algorithm.symmetry_loss": True})) == (False, 1)


def test_gather_stream_struct_matches_the_header(tmp_path):
    from booster_gym_amd import _lib

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "booster_gym_amd.h"\nint main(){printf("%zu %zu %zu %d\\n", sizeof(bg_gather_stream), '
                   "offsetof(bg_gather_stream, dst), offsetof(bg_gather_stream, width), BG_GATHER_MAX_STREAMS);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = _lib.GatherStream
    assert got == [C.sizeof(G), G.dst.offset, G.width.offset, _lib.GATHER_MAX_STREAMS]


@pytest.mark.parametrize("B", [128, 3072, 6144, 98304, 100 * 24, 786432])
def test_permutation_is_a_bijection(perm_lib, B):
    h = perm_lib.hh_perm_half_bits(B)
    assert 4 ** h >= B and (h == 1 or 4 ** (h - 1) < B)  # the smallest even bit width that holds B
    for seed, update, epoch in KEYS:
        p = host_perm(perm_lib, B, seed, update, epoch)
        assert p.min() == 0 and p.max() == B - 1 and np.array_equal(np.sort(p), np.arange(B, dtype=np.int32)), (B, seed, update, epoch)
    assert not np.array_equal(host_perm(perm_lib, B, 42, 0, 0), host_perm(perm_lib, B, 43, 0, 0))  # the seed, the update and the mini-epoch all key it
    assert not np.array_equal(host_perm(perm_lib, B, 42, 0, 0), host_perm(perm_lib, B, 42, 1, 0))
    assert not np.array_equal(host_perm(perm_lib, B, 42, 0, 0), host_perm(perm_lib, B, 42, 0, 1))
    assert np.array_equal(host_perm(perm_lib, B, 42, 3, 2), host_perm(perm_lib, B, 42, 3, 2))


# Bounds of the uniform law on the permutations of [0, B), B = 98,304, each at five standard deviations:
#   * positions and sources binned into 16 x 16 equal buckets: the table has fixed margins B / 16, (16 - 1)^2 = 225 degrees of freedom; the
#     chi-square statistic has mean 225 and variance 2 x 225: at most 225 + 5 sqrt(450) = 331.07;
#   * positions with pi(i + 1) = pi(i) + 1: each of the B - 1 positions has probability 1 / B (up to 1 / B^2), the count is Poisson(1) in the limit:
#     mean 1, standard deviation 1, at most 1 + 5 = 6 <= 8 (the Poisson tail beyond 8 is 1.1e-6);
#   * positions where two independent permutations agree: the fixed points of a uniform permutation, Poisson(1) likewise: at most 8.
CHI2_MAX, ADJACENT_MAX, AGREE_MAX = 225 + 5 * np.sqrt(2 * 225), 8, 8


def _chi2(p):
    B = p.size
    t = np.zeros((16, 16))
    np.add.at(t, (np.arange(B) * 16 // B, p.astype(np.int64) * 16 // B), 1)
    e = B / 256.0
    return float(((t - e) ** 2 / e).sum())


def _adjacent(p):
    return int((np.diff(p.astype(np.int64)) == 1).sum())


def test_uniformity_bounds_hold_for_numpys_own_shuffle():
    """The derivation above checked on a generator nobody doubts: if numpy's permutation left a bound, the bound would be wrong."""
    B = 98304
    ps = [np.random.default_rng(k).permutation(B) for k in range(9)]
    for k in range(8):
        c, a, g = _chi2(ps[k]), _adjacent(ps[k]), int((ps[k] == ps[k + 1]).sum())
        print(f"numpy seed {k}: chi-square {c:.1f} (<= {CHI2_MAX:.1f}), adjacent {a}, agreeing with seed {k + 1}: {g}")
        assert c <= CHI2_MAX and a <= ADJACENT_MAX and g <= AGREE_MAX, k


def test_permutation_is_uniform_within_five_sigma(perm_lib):
    B = 98304
    for seed, update, epoch in KEYS:
        p = host_perm(perm_lib, B, seed, update, epoch)
        q = host_perm(perm_lib, B, seed, update, (epoch + 1) % 2 ** 24)  # another mini-epoch of the same key
        c, a, g = _chi2(p), _adjacent(p), int((p == q).sum())
        print(f"key {(seed, update, epoch)}: chi-square {c:.1f} (<= {CHI2_MAX:.1f}), adjacent {a}, agreeing with the next mini-epoch: {g}")
        assert c <= CHI2_MAX, (seed, update, epoch, c)
        assert a <= ADJACENT_MAX, (seed, update, epoch, a)
        assert g <= AGREE_MAX, (seed, update, epoch, g)


def test_plan_of_a_mini_batch_has_the_whole_batchs_kernel_forms():
    from booster_gym_amd.utils.runner import plan_update

    inputs = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9,
                  one_stream=True, defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True,
                  rollout_forward=True, dp_active=False)
    nets = (((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64))
    B = 24 * 4096
    whole = plan_update(*nets, B, **inputs)
    for K in (2, 4, 8, 768):
        assert plan_update(*nets, B // K, **inputs) == whole, K
    # ... and with the per-layer kernels of a frame stack and a height scan (inputs of 256 columns)
    wide = (((342, 256, 256, 128, 1), 512), ((141, 256, 128, 128, 12), 256))
    assert plan_update(*wide, B // 4, **inputs) == plan_update(*wide, B, **inputs)
    assert plan_update(*wide, B, **inputs).critic.fwd == "layer"
