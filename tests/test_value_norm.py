"""Value normalisation without a device (algorithm.normalize_value, utils/value_norm.py): the key's rules, the shipped yaml, the checkpoint rules on
plain dicts, the plan's new field and its refusals, the library's declarations, and the merge rule bg_value_norm_update restates."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "algorithm.normalize_value"
SW = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
          defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
CRITIC, ACTOR = ((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64)


def test_key_rules():
    from booster_gym_amd.utils.value_norm import KEY as K, normalize_value_of

    assert K == KEY
    for cfg in ({}, {"algorithm": None}, {"algorithm": {}}, {"algorithm": {"normalize_value": None}}, {"algorithm": {"normalize_value": False}}):
        assert normalize_value_of(cfg) == (False, 1.0e-2), cfg
    assert normalize_value_of({"algorithm": {"normalize_value": True}}) == (True, 1.0e-2)
    # normalization_eps is read with empirical_normalization off (and absent)
    assert normalize_value_of({"algorithm": {"normalize_value": True, "normalization_eps": 0.05, "empirical_normalization": False}}) == (True, 0.05)
    assert normalize_value_of({"algorithm": {"normalize_value": True, "normalization_eps": None}}) == (True, 1.0e-2)
    for bad in (1, 0, "true", "yes", 1.0, [True]):
        with pytest.raises(ValueError, match=r"algorithm\.normalize_value"):
            normalize_value_of({"algorithm": {"normalize_value": bad}})
    for bad in (0, 0.0, -1.0e-2, float("nan"), float("inf"), "0.01", True):
        with pytest.raises(ValueError, match=r"algorithm\.normalization_eps"):
            normalize_value_of({"algorithm": {"normalize_value": True, "normalization_eps": bad}})


def test_shipped_yaml_names_the_key_in_a_comment_only():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.value_norm import normalize_value_of

    cfg = load_cfg("T1")
    assert "normalize_value" not in cfg["algorithm"] and normalize_value_of(cfg) == (False, 1.0e-2)
    text = open(os.path.join(ROOT, "booster_gym_amd", "envs", "T1.yaml")).read()
    comment = "\n".join(l for l in text.splitlines() if l.lstrip().startswith("#"))
    assert "# normalize_value (an addition of this build" in comment and "not listed below" in comment.split("# normalize_value (", 1)[1].split("\n", 1)[0]
    assert "normalize_value" not in "\n".join(l.split("#", 1)[0] for l in text.splitlines())
    assert load_cfg("T1", {KEY: True})["algorithm"]["normalize_value"] is True


def test_checkpoint_rules_on_plain_dicts():
    from booster_gym_amd.utils.value_norm import ValueNormalizer, check_checkpoint, check_entry, triple_of

    entry = {"mean": 0.1, "var": 0.3, "count": 640.0, "eps": 1.0e-2}  # (not fp32 numbers: the state is float64)
    check_entry(None, False, 1.0e-2)
    check_entry(entry, True, 1.0e-2)
    with pytest.raises(ValueError, match=r"has no value normaliser but the config sets algorithm\.normalize_value: true"):
        check_entry(None, True, 1.0e-2, "x.pth")
    with pytest.raises(ValueError, match=r"carries a value normaliser but the config has algorithm\.normalize_value: false"):
        check_entry(entry, False, 1.0e-2, "x.pth")
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value.*algorithm\.normalization_eps = 0\.01, the config has 0\.05"):
        check_entry(entry, True, 0.05, "x.pth")
    # a host-side normaliser (CPU tensors: no library call) takes the entry and gives it back; the triple is the float64 state's, rounded
    norm = ValueNormalizer(1.0e-2, device="cpu")
    assert norm.state.tolist() == [0.0, 1.0, 0.0] and norm.stats.tolist() == [0.0, float(np.float32(1.01)), float(np.float32(1.0 / 1.01))]
    assert norm.state_dict() == {"mean": 0.0, "var": 1.0, "count": 0.0, "eps": 1.0e-2}
    check_checkpoint("x.pth", entry, norm)
    assert norm.state_dict() == entry
    sigma = np.sqrt(0.3) + 1.0e-2
    assert np.array_equal(norm.stats.numpy(), np.array([0.1, sigma, 1.0 / sigma]).astype(np.float32)) and np.array_equal(norm.stats.numpy(), triple_of(0.1, 0.3, 1.0e-2))
    assert norm.scalars() == {"value_norm/mean": 0.1, "value_norm/std": float(np.sqrt(0.3)), "value_norm/count": 640.0}
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value"):
        check_checkpoint("x.pth", None, norm)
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value"):
        check_checkpoint("x.pth", entry, None)
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value"):
        check_checkpoint("x.pth", entry, ValueNormalizer(0.05, device="cpu"))
    check_checkpoint("x.pth", None, None)


def test_runner_checkpoint_dict_and_load_on_a_stub(tmp_path):
    """Runner.checkpoint_dict / Runner._load on tests/test_obs_norm.py's stub: key off, exactly the keys as before; key on, one more; a runner that
    only plays (test = True) loads either checkpoint."""
    import torch

    from booster_gym_amd.utils.runner import Runner
    from booster_gym_amd.utils.value_norm import ValueNormalizer
    from test_obs_norm import _runner_stub

    def stub(norm, ck, test=False):
        s = _runner_stub(None, ck)
        s.value_norm, s.test = norm, test
        return s

    assert sorted(Runner.checkpoint_dict(stub(None, None))) == ["curriculum", "model", "optimizer"]
    norm = ValueNormalizer(1.0e-2, device="cpu")
    norm.load_state_dict({"mean": -1.7, "var": 4.3, "count": 1280.0, "eps": 1.0e-2})
    d = Runner.checkpoint_dict(stub(norm, None))
    assert sorted(d) == ["curriculum", "model", "optimizer", "value_normalizer"] and d["value_normalizer"] == {"mean": -1.7, "var": 4.3, "count": 1280.0, "eps": 1.0e-2}
    model_keys = sorted(d["model"])
    assert model_keys == sorted(Runner.checkpoint_dict(stub(None, None))["model"])  # "model" is untouched
    on, off = str(tmp_path / "on.pth"), str(tmp_path / "off.pth")
    torch.save(d, on)
    torch.save(Runner.checkpoint_dict(stub(None, None)), off)
    fresh = stub(ValueNormalizer(1.0e-2, device="cpu"), on)
    Runner._load(fresh)
    assert torch.equal(fresh.value_norm.state, norm.state) and torch.equal(fresh.value_norm.stats, norm.stats)
    Runner._load(stub(None, off))
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value: true"):
        Runner._load(stub(ValueNormalizer(1.0e-2, device="cpu"), off))
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value: false"):
        Runner._load(stub(None, on))
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value.*normalization_eps"):
        Runner._load(stub(ValueNormalizer(0.05, device="cpu"), on))
    Runner._load(stub(None, on, test=True))  # play, evaluation and export never evaluate the critic


def test_plan_field_defaults_to_off_and_refuses_plans_without_the_fused_launch():
    from booster_gym_amd.utils.runner import UpdatePlan, plan_update

    today = plan_update(CRITIC, ACTOR, 24 * 4096, **SW)
    off = plan_update(CRITIC, ACTOR, 24 * 4096, value_norm=False, **SW)
    assert today._fields == off._fields and "value_norm" in UpdatePlan._fields
    for f in today._fields:
        assert getattr(today, f) == getattr(off, f), f
    assert today.value_norm is False
    on = plan_update(CRITIC, ACTOR, 24 * 4096, value_norm=True, **SW)
    assert on.value_norm is True and on._replace(value_norm=False) == today and on.ahead  # every other field, the forward-ahead included, as without the key
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value needs the fused output layers"):
        plan_update(CRITIC, ACTOR, 24 * 4096, value_norm=True, **{**SW, "fused_head": False})
    with pytest.raises(ValueError, match=r"algorithm\.normalize_value needs the fused GAE launch.*horizon_length"):
        plan_update(CRITIC, ACTOR, 24 * 4096, value_norm=True, **{**SW, "fused_gae": False})
    plan_update(CRITIC, ACTOR, 24 * 4096, **{**SW, "fused_gae": False})  # (off: no refusal)


def test_library_declares_binds_and_exports_the_entry_points():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    declared = set(re.findall(r"\b(bg_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in ("bg_critic_values_gae_norm", "bg_value_denormalize", "bg_value_norm_update"):
        assert s in declared and s in _lib.SYMBOLS and getattr(lib, s).argtypes is not None, s
    # argument checks on the host, before any launch
    assert lib.bg_critic_values_gae_norm(0, 4, None, None, None, None, None, None, 0.9, 0.9, None, None, None, None, None, None, None) == -1
    assert b"bg_critic_values_gae_norm" in lib.bg_last_error()
    assert lib.bg_value_denormalize(4, None, None, None) == -1 and b"bg_value_denormalize" in lib.bg_last_error()
    assert lib.bg_value_norm_update(None, None, None, 1.0e-2, None) == -1 and b"bg_value_norm_update" in lib.bg_last_error()


def merge_f64(state, sums):
    """What bg_value_norm_update computes, in numpy float64: state (mean, var, count), sums (sum, sum of squares, count) -> the new state."""
    mean, var, count = (np.float64(x) for x in state)
    s, ss, n = (np.float64(x) for x in sums)
    if not n > 0:
        return (mean, var, count)
    m_b = s / n
    v_b = max(ss / n - m_b * m_b, np.float64(0.0))
    total = count + n
    r = n / total
    d = m_b - mean
    new_mean = mean + r * d
    new_var = max(var + r * (v_b - var + d * (m_b - new_mean)), np.float64(0.0))
    return (new_mean, new_var, total)


def test_three_merges_equal_merge_moments_and_the_statistics_of_all_rows():
    from booster_gym_amd.utils.obs_norm import merge_moments, moments_from_sums

    rng = np.random.default_rng(5)
    batches = [rng.normal(0.05, 0.02, 640), rng.normal(1.5, 0.7, 3072), rng.normal(9.0, 2.5, 1000)]  # returns growing as over a run
    # the state's start (0, 1, 0) has no rows: after the first merge nothing of it is left
    st, ref = (0.0, 1.0, 0.0), (np.zeros(1), np.ones(1), 0.0)
    for k, x in enumerate(batches):
        sums = (x.sum(), (x * x).sum(), float(x.size))
        st = merge_f64(st, sums)
        ref = merge_moments(*ref, *moments_from_sums([sums[0]], [sums[1]], sums[2]), sums[2])
        assert st[0] == ref[0][0] and st[1] == ref[1][0] and st[2] == ref[2], k  # the same operations in the same order: the same bits
        seen = np.concatenate(batches[: k + 1])
        assert abs(st[0] - seen.mean()) <= 1e-12 * abs(seen.mean()) and abs(st[1] - seen.var()) <= 1e-12 * seen.var() and st[2] == seen.size, k
    assert merge_f64(st, (123.0, 456.0, 0.0)) == st
