"""The action-smoothness loss without a GPU (algorithm.smoothness_loss): the validation of its three keys, the refused combinations, the plan of its
update, and the numpy restatement of the partner rule and of its draw that tests/test_gpu_smoothness.py holds bg_partner_rows to."""
import os

import numpy as np
import pytest

from oracle.task_ref import philox4x32_10, rand4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_PARTNER = 30  # bg_rng.h: the stream id of the draw


# ------------------------------------------------------------------ the restatement
def partner_draw(seed, rows, update, epoch):
    """u of rows 0 .. rows - 1 as float32 in [0, 1): the upper 24 bits of word 0 of Philox4x32-10 on the key (seed) and the counter (row, update,
    RS_PARTNER, mini-epoch), times 2^-24."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o = philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(rows, dtype=np.uint32), np.uint32(int(update) & 0xFFFFFFFF), np.uint32(RS_PARTNER),
                      np.uint32(int(epoch) & 0xFFFFFFFF))
    return (o[0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def partner_rows_ref(x, x_last, dones, time_outs, mode="next", seed=0, update=0, epoch=0):
    """(y, u) of the partner rule on float32 x [T, N, cols], x_last [N, cols] and flags [T, N]: y = x + u (x+ - x) in float32 with two roundings (the
    kernel's fma has one), x+ the same env's row one step later (x_last behind the last step); a cut row (dones or time_outs) is x itself; mode "next":
    u = 1 and y is x+ itself."""
    T, N, cols = x.shape
    nxt = np.concatenate([x[1:], x_last[None]], axis=0)
    cut = (np.asarray(dones).astype(bool) | np.asarray(time_outs).astype(bool))[..., None]
    if mode == "next":
        u = np.ones((T, N), dtype=np.float32)
        y = nxt.copy()
    else:
        u = partner_draw(seed, T * N, update, epoch).reshape(T, N)
        y = (x + u[..., None] * (nxt - x)).astype(np.float32)
    return np.where(cut, x, y).astype(np.float32), u


def test_draw_is_the_oracles_philox_on_a_stream_of_its_own():
    """The draw's bits are rand4's first word on counter word 3 = 0 (the one counter rand4 exposes); it stays in [0, 1); it differs between
    mini-epochs and updates and repeats on a repeat; no id of oracle/task_ref.py's streams moves."""
    u = partner_draw(42, 4096, 0, 0)
    ur, _ = rand4(42, np.arange(4096, dtype=np.uint32), 0, RS_PARTNER)
    # rand4's uniform is ((o >> 8) + 0.5) 2^-24 in float32: the same 24 bits (the + 0.5 is absorbed above 2^23: compare where it is exact)
    small = u < 0.5
    assert small.any() and np.array_equal((u[small] * np.float32(16777216.0) + np.float32(0.5)) * np.float32(1.0 / 16777216.0), ur[small, 0])
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55
    assert not np.array_equal(u, partner_draw(42, 4096, 0, 1)) and not np.array_equal(u, partner_draw(42, 4096, 1, 0))
    assert not np.array_equal(u, partner_draw(43, 4096, 0, 0)) and np.array_equal(u, partner_draw(42, 4096, 0, 0))
    rng_h = open(os.path.join(ROOT, "booster_gym_amd", "csrc", "bg_rng.h")).read()
    assert f"RS_PARTNER = {RS_PARTNER}," in rng_h and "RS_PERM = 28," in rng_h and "RS_DAGGER = 29," in rng_h and "RS_ACTOR = 32," in rng_h


def test_partner_rule_restated():
    rng = np.random.default_rng(0)
    T, N, cols = 3, 5, 8
    x, x_last = rng.standard_normal((T, N, cols)).astype(np.float32), rng.standard_normal((N, cols)).astype(np.float32)
    dones, time_outs = np.zeros((T, N), bool), np.zeros((T, N), bool)
    dones[1, 2] = time_outs[2, 4] = time_outs[0, 0] = True
    y, u = partner_rows_ref(x, x_last, dones, time_outs)
    assert np.array_equal(y[2, 1], x_last[1]) and np.array_equal(y[0, 3], x[1, 3]) and (u == 1).all()
    for t, e in ((1, 2), (2, 4), (0, 0)):
        assert np.array_equal(y[t, e], x[t, e])
    yi, ui = partner_rows_ref(x, x_last, dones, time_outs, "interpolate", 7, 3, 2)
    assert np.array_equal(ui.reshape(-1), partner_draw(7, T * N, 3, 2))
    for t, e in ((1, 2), (2, 4), (0, 0)):
        assert np.array_equal(yi[t, e], x[t, e])
    lo, hi = np.minimum(x[0, 3], x[1, 3]), np.maximum(x[0, 3], x[1, 3])
    assert ((yi[0, 3] >= lo - 1e-6) & (yi[0, 3] <= hi + 1e-6)).all()


# ------------------------------------------------------------------ the keys
def _cfg(**alg):
    return {"algorithm": dict(alg), "runner": {"horizon_length": 24}, "env": {"num_envs": 128}}


def test_defaults_and_values():
    from booster_gym_amd.utils.runner import smoothness_loss

    for off in ({}, {"smoothness_loss": None}, {"smoothness_loss": False}, {"smoothness_loss": False, "smoothness_coef": "x", "smoothness_pairs": 3}):
        assert smoothness_loss(_cfg(**off)) == (False, 0.0, "next")
    assert smoothness_loss({}) == (False, 0.0, "next") and smoothness_loss({"algorithm": None}) == (False, 0.0, "next")
    assert smoothness_loss(_cfg(smoothness_loss=True, smoothness_coef=2)) == (True, 2.0, "next")
    assert smoothness_loss(_cfg(smoothness_loss=True, smoothness_coef=0)) == (True, 0.0, "next")
    assert smoothness_loss(_cfg(smoothness_loss=True, smoothness_coef=0.5, smoothness_pairs="interpolate")) == (True, 0.5, "interpolate")
    assert smoothness_loss(_cfg(smoothness_loss=True, smoothness_coef=0.5, smoothness_pairs="next")) == (True, 0.5, "next")


def test_every_bad_value_names_its_key():
    from booster_gym_amd.utils.runner import smoothness_loss

    for bad in (1, 0, "true", "yes", 1.0, [True]):
        with pytest.raises(ValueError, match=r"algorithm\.smoothness_loss"):
            smoothness_loss(_cfg(smoothness_loss=bad, smoothness_coef=1.0))
    with pytest.raises(ValueError, match=r"algorithm\.smoothness_coef"):
        smoothness_loss(_cfg(smoothness_loss=True))  # no default
    for bad in (None, -1, -1e-9, float("nan"), float("inf"), "1", True, [1.0]):
        with pytest.raises(ValueError, match=r"algorithm\.smoothness_coef"):
            smoothness_loss(_cfg(smoothness_loss=True, smoothness_coef=bad))
    for bad in ("", "Next", "both", "lerp", 1, None, True, ["next"]):
        with pytest.raises(ValueError, match=r"algorithm\.smoothness_pairs"):
            smoothness_loss(_cfg(smoothness_loss=True, smoothness_coef=1.0, smoothness_pairs=bad))


def test_each_refused_combination_names_both_keys():
    from booster_gym_amd.utils.runner import smoothness_loss

    on = {"smoothness_loss": True, "smoothness_coef": 1.0}
    cases = [(_cfg(symmetry_loss=True, **on), r"algorithm\.symmetry_loss"),
             ({**_cfg(**on), "runner": {"horizon_length": 24, "num_mini_batches": 4}}, r"runner\.num_mini_batches"),
             ({**_cfg(**on), "estimator": {"enabled": True}}, r"estimator\.enabled"),
             (_cfg(rnn_hidden_size=128, **on), r"algorithm\.rnn_hidden_size")]
    for cfg, other in cases:
        with pytest.raises(ValueError) as ex:
            smoothness_loss(cfg)
        msg = str(ex.value)
        import re

        assert re.search(r"algorithm\.smoothness_loss", msg) and re.search(other, msg), msg
    # ... and none of them with the key off, or with the other option off
    for cfg, _ in cases:
        cfg["algorithm"]["smoothness_loss"] = False
        assert smoothness_loss(cfg)[0] is False
    assert smoothness_loss({**_cfg(symmetry_loss=False, rnn_hidden_size=0, **on), "runner": {"num_mini_batches": 1}, "estimator": {"enabled": False}})[0]


def test_shipped_yaml_lists_none_of_the_keys_and_documents_them():
    import yaml

    path = os.path.join(ROOT, "booster_gym_amd", "envs", "T1.yaml")
    alg = yaml.safe_load(open(path))["algorithm"]
    text = open(path).read()
    for k in ("smoothness_loss", "smoothness_coef", "smoothness_pairs"):
        assert k not in alg
        assert any(k in line and line.lstrip().startswith("#") for line in text.splitlines()), k
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import smoothness_loss

    assert smoothness_loss(load_cfg("T1")) == (False, 0.0, "next")
    assert smoothness_loss(load_cfg("T1", {"algorithm.smoothness_loss": True, "algorithm.smoothness_coef": 3.0,
                                           "algorithm.smoothness_pairs": "interpolate"})) == (True, 3.0, "interpolate")


def test_distill_does_not_read_the_keys():
    text = open(os.path.join(ROOT, "booster_gym_amd", "utils", "distill.py")).read()
    assert "smoothness" not in text


# ------------------------------------------------------------------ the plan
SW = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
          defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
NETS = (((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64))


def test_plan_with_the_key_on_is_the_symmetric_plan():
    from booster_gym_amd.utils.runner import plan_update

    B = 24 * 4096
    today = plan_update(*NETS, B, **SW)
    assert plan_update(*NETS, B, smoothness=False, **SW) == today and today.ahead and not today.smoothness and not today.symmetry
    sym, smooth = plan_update(*NETS, B, symmetry=True, **SW), plan_update(*NETS, B, smoothness=True, **SW)
    assert smooth.smoothness and not sym.smoothness
    assert smooth._replace(smoothness=False) == sym  # field by field the plan of symmetry = True
    assert not smooth.ahead and smooth.fused_head
    # the actor's passes are planned for 2 x rows: at a batch where B and 2B fall on different sides of a kernel's range the actor's plan is 2B's
    double = plan_update(NETS[0], NETS[1], 2 * B, **SW)
    assert smooth.actor == double.actor and smooth.critic == today.critic
    small = 40  # B = 40 rows: the actor's 80
    assert plan_update(*NETS, small, smoothness=True, **SW).actor == plan_update(*NETS, 2 * small, **SW).actor


def test_plan_without_the_fused_heads_is_refused():
    from booster_gym_amd.utils.runner import plan_update

    with pytest.raises(ValueError, match=r"algorithm\.smoothness_loss.*fused output layers"):
        plan_update(*NETS, 24 * 4096, smoothness=True, **{**SW, "fused_head": False})
    with pytest.raises(ValueError, match=r"algorithm\.symmetry_loss.*fused output layers"):  # (the symmetry loss's own message has not moved)
        plan_update(*NETS, 24 * 4096, symmetry=True, **{**SW, "fused_head": False})


def test_entry_point_is_declared_bound_and_wrapped():
    from booster_gym_amd import _lib
    from booster_gym_amd.utils import utils

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    assert "int bg_partner_rows(" in header and "bg_partner_rows" in _lib.SYMBOLS and callable(utils.partner_rows)
    assert "#define BG_PARTNER_NEXT 0" in header and "#define BG_PARTNER_INTERPOLATE 1" in header
    assert (_lib.PARTNER_NEXT, _lib.PARTNER_INTERPOLATE) == (0, 1)
