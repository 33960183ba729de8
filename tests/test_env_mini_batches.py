"""runner.num_env_mini_batches without a GPU: the validation of the key (runner.env_mini_batches), what stays refused, the shipped yaml, the new entry
point in header and bindings, and the index rule of bg_gather_sequences restated in numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "runner.num_env_mini_batches"
RNN = "algorithm.rnn_hidden_size"


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", over)


def gather_sequences_reference(T, N, K, sigma, src):
    """bg_gather_sequences' per-row rule: dst[(k T + t) n + j] = src[t N + sigma[k n + j]], n = N / K; src [T N][w] -> dst [K][T][n][w]."""
    assert N % K == 0
    n, w = N // K, src.shape[-1]
    src, dst = src.reshape(T * N, w), np.zeros((K * T * n, w), dtype=src.dtype)
    for k in range(K):
        for t in range(T):
            for j in range(n):
                dst[(k * T + t) * n + j] = src[t * N + sigma[k * n + j]]
    return dst.reshape(K, T, n, w)


def test_off_values():
    from booster_gym_amd.utils.runner import env_mini_batches

    cfg = _cfg()
    assert "num_env_mini_batches" not in cfg["runner"] and env_mini_batches(cfg) == (False, 1)  # absent: off
    for off in (None, 1):
        cfg["runner"]["num_env_mini_batches"] = off
        assert env_mini_batches(cfg) == (False, 1)
        assert env_mini_batches(_cfg(**{RNN: 128, KEY: off})) == (False, 1)
    assert env_mini_batches(_cfg(**{RNN: 128, KEY: 4, "env.num_envs": 4096})) == (True, 4)
    assert env_mini_batches(_cfg(**{RNN: 256, KEY: 2, "env.num_envs": 80, "runner.horizon_length": 16})) == (True, 2)


def test_every_refusal_names_its_keys():
    from booster_gym_amd.utils.runner import env_mini_batches

    for bad in (0, -2, 2.0, 1.5, "4", True, [2]):
        c = _cfg(**{RNN: 128, "env.num_envs": 4096})
        c["runner"]["num_env_mini_batches"] = bad
        with pytest.raises(ValueError, match=r"runner\.num_env_mini_batches.*integer >= 1"):
            env_mini_batches(c)
    with pytest.raises(ValueError, match=r"runner\.num_env_mini_batches = 3 does not divide env\.num_envs = 4096"):
        env_mini_batches(_cfg(**{RNN: 128, KEY: 3, "env.num_envs": 4096}))
    with pytest.raises(ValueError, match=r"runner\.num_env_mini_batches = 2 .*24 x 50 = 1200 rows.*128"):  # (divides the envs, but not into whole slabs)
        env_mini_batches(_cfg(**{RNN: 128, KEY: 2, "env.num_envs": 100}))
    with pytest.raises(ValueError, match=r"runner\.num_env_mini_batches = 1024 .*24 x 4 = 96 rows.*128"):  # (below one slab)
        env_mini_batches(_cfg(**{RNN: 128, KEY: 1024, "env.num_envs": 4096}))
    for cfg in (_cfg(**{KEY: 4, "env.num_envs": 4096}), _cfg(**{KEY: 4, RNN: 0, "env.num_envs": 4096})):  # a feed-forward actor
        with pytest.raises(ValueError, match=r"runner\.num_env_mini_batches = 4 .*algorithm\.rnn_hidden_size.*runner\.num_mini_batches"):
            env_mini_batches(cfg)
    with pytest.raises(ValueError, match=r"runner\.num_env_mini_batches = 4 together with runner\.num_mini_batches = 2"):
        env_mini_batches(_cfg(**{RNN: 128, KEY: 4, "runner.num_mini_batches": 2, "env.num_envs": 4096}))


def test_what_a_recurrent_actor_refused_stays_refused():
    from booster_gym_amd.utils.runner import rnn_hidden_size_of

    for over in ({"runner.num_mini_batches": 4}, {"runner.num_mini_batches": 4, KEY: 4}):
        with pytest.raises(ValueError, match=r"algorithm\.rnn_hidden_size.*runner\.num_mini_batches"):
            rnn_hidden_size_of(_cfg(**{RNN: 128, "env.num_envs": 4096, **over}))
    assert rnn_hidden_size_of(_cfg(**{RNN: 128, KEY: 4, "env.num_envs": 4096})) == 128  # the new key is none of that function's business


def test_shipped_config_describes_the_key_in_a_comment_only():
    assert "num_env_mini_batches" not in _cfg()["runner"]
    text = open(os.path.join(ROOT, "booster_gym_amd", "envs", "T1.yaml")).read()
    block = text[: text.index("\nrunner:")]
    assert "num_env_mini_batches" in block[block.rindex("\n\n"):]  # the comment block above `runner:`
    assert all(line.lstrip().startswith("#") for line in text.splitlines() if "num_env_mini_batches" in line)


def test_entry_point_is_declared_and_bound_with_matching_arguments(tmp_path):
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    m = re.search(r"\bint bg_gather_sequences\(([^;]*)\);", header)
    assert m and "bg_gather_sequences" in _lib.SYMBOLS
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ["int32_t", "int32_t", "int32_t", "const int32_t*", "const bg_sequence_stream*", "int32_t", "void*"]
    fn = _lib.load().bg_gather_sequences
    i32, vp = C.c_int32, C.c_void_p
    assert list(fn.argtypes) == [i32, i32, i32, vp, C.POINTER(_lib.SequenceStream), i32, vp] and fn.restype is i32
    # the descriptor's layout and the stream limit, from the header itself
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "booster_gym_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %d %d\\n", '
                   "sizeof(bg_sequence_stream), offsetof(bg_sequence_stream, dst), offsetof(bg_sequence_stream, width), offsetof(bg_sequence_stream, elem_size), "
                   "offsetof(bg_sequence_stream, per_env), BG_SEQUENCE_MAX_STREAMS, BG_GATHER_MAX_STREAMS);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.SequenceStream
    assert got == [C.sizeof(S), S.dst.offset, S.width.offset, S.elem_size.offset, S.per_env.offset, _lib.SEQUENCE_MAX_STREAMS, _lib.GATHER_MAX_STREAMS]
    assert _lib.SEQUENCE_MAX_STREAMS >= 9  # the recurrent update's nine streams


@pytest.mark.parametrize("T,N,K,w", [(5, 48, 3, 4), (3, 40, 2, 1), (24, 64, 4, 3), (2, 6, 6, 2)])
def test_index_rule_in_numpy(T, N, K, w):
    n = N // K
    src = np.arange(T * N * w, dtype=np.float32).reshape(T, N, w)
    ident = gather_sequences_reference(T, N, K, np.arange(N), src)
    assert ident.shape == (K, T, n, w) and np.array_equal(ident, src.reshape(T, K, n, w).transpose(1, 0, 2, 3))
    sigma = np.random.default_rng(T * N + K).permutation(N)
    out = gather_sequences_reference(T, N, K, sigma, src)
    # every source row exactly once (the rows are distinct: their first column names them)
    assert np.array_equal(np.sort(out[..., 0].reshape(-1)), src[..., 0].reshape(-1))
    # mini-batch k holds, at every step, the envs sigma[k n : (k + 1) n] in that order
    for k in range(K):
        assert np.array_equal(out[k], src[:, sigma[k * n : (k + 1) * n]])
