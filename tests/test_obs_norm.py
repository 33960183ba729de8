"""Empirical observation normalisation (algorithm.empirical_normalization) without a GPU: the merge rule against numpy, the fold into the actor's
first layer (and the real export_model.py path), the checkpoint rules of Runner._load / checkpoint_dict, the C ABI's argument checks and the
exchange of the statistics between two gloo ranks."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)


def _cfg(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", dict(over))


# ------------------------------------------------------------------ config keys
def test_keys_default_off_and_eps_is_checked():
    from booster_gym_amd.utils.obs_norm import normalization_cfg

    cfg = _cfg()
    assert cfg["algorithm"]["empirical_normalization"] is False and cfg["algorithm"]["normalization_eps"] == 1.0e-2  # (the shipped yaml names both)
    assert normalization_cfg(cfg) == (False, 1.0e-2)
    absent = _cfg()
    del absent["algorithm"]["empirical_normalization"], absent["algorithm"]["normalization_eps"]
    assert normalization_cfg(absent) == (False, 1.0e-2)
    assert normalization_cfg(_cfg(**{"algorithm.empirical_normalization": True, "algorithm.normalization_eps": 0.5})) == (True, 0.5)
    for bad in (0, 0.0, -1.0e-2, float("nan"), "1e-2", True):
        with pytest.raises(ValueError, match=r"algorithm\.normalization_eps"):
            normalization_cfg(_cfg(**{"algorithm.normalization_eps": bad}))
    with pytest.raises(ValueError, match=r"algorithm\.empirical_normalization"):
        normalization_cfg(_cfg(**{"algorithm.empirical_normalization": 1}))


# ------------------------------------------------------------------ merge rule
def test_merge_rule_equals_the_moments_of_the_concatenation():
    """K batches fed one by one (among them a single row and batches of very different sizes; one column constant, one with mean^2 / var = 1e8) give
    the mean and biased variance numpy computes in float64 on their concatenation.

    Bound.  One merge step is a handful of float64 operations on d = m_b - mean, d (m_b - mean'), v_b - var: each rounds at eps_f64 relative to its
    own magnitude, at most max(var, d^2), and the rounding of the mean itself (eps_f64 |mean|) enters d, hence d^2 with 2 |d| eps_f64 |mean| <=
    eps_f64 (d^2 + mean^2).  The batches here are drawn within 4 standard deviations of the column mean, so d^2 <= 16 var: per step at most
    ~4 roundings x 16 x eps_f64 x max(var, mean^2), and K steps add up linearly at worst:
        |var error| <= 64 eps_f64 K max(var, mean^2) = 64 eps_f64 K var max(1, mean^2 / var),       |mean error| <= 64 eps_f64 K max(|mean|, std)
    (the absolute form of the same bound, so that it holds for the constant column whose variance is 0).  numpy's own pairwise sums stay below
    that (eps_f64 log2(rows) relative to the same magnitudes)."""
    from booster_gym_amd.utils.obs_norm import ObsNormalizer, merge_moments

    rng = np.random.default_rng(11)
    cols = 7
    offset = np.array([0.0, 1.0, -3.0, 1.0e4, 2.5, 0.02, -40.0])
    scale = np.array([1.0, 1.0e-3, 1.0e3, 1.0, 0.0, 5.0, 0.3])  # column 3: mean^2 / var = 1e8; column 4: constant
    sizes = [1, 5, 1, 4096, 3, 257, 1, 64, 1000, 2, 31, 1]
    batches = [offset + scale * np.clip(rng.standard_normal((n, cols)), -4.0, 4.0) for n in sizes]
    K = len(batches)
    norm = ObsNormalizer(cols)
    assert norm.count == 0 and np.array_equal(norm.mean, np.zeros(cols)) and np.array_equal(norm.var, np.ones(cols))
    for b in batches:
        norm.merge(b.mean(axis=0), b.var(axis=0), b.shape[0])
    allrows = np.concatenate(batches)
    mean, var = allrows.mean(axis=0), allrows.var(axis=0)
    assert norm.count == allrows.shape[0]
    bound_var = 64 * EPS64 * K * np.maximum(var, mean * mean)
    bound_mean = 64 * EPS64 * K * np.maximum(np.abs(mean), np.sqrt(var))
    err_var, err_mean = np.abs(norm.var - var), np.abs(norm.mean - mean)
    print("merge: var error / bound", err_var / bound_var, "mean error / bound", err_mean / bound_mean)
    assert (err_var <= bound_var).all(), (err_var, bound_var)
    assert (err_mean <= bound_mean).all(), (err_mean, bound_mean)
    assert norm.var[4] >= 0.0
    # the pure function: the first batch replaces the initial state entirely (count 0), an empty batch changes nothing
    m1, v1, c1 = merge_moments(np.zeros(cols), np.ones(cols), 0, batches[3].mean(0), batches[3].var(0), sizes[3])
    assert c1 == sizes[3] and np.allclose(m1, batches[3].mean(0), rtol=0, atol=0) and np.abs(v1 - batches[3].var(0)).max() <= 4 * EPS64 * np.abs(v1).max()
    m2, v2, c2 = merge_moments(m1, v1, c1, np.zeros(cols), np.zeros(cols), 0)
    assert c2 == c1 and np.array_equal(m2, m1) and np.array_equal(v2, v1)
    # the sums form (what bg_obs_moments writes and the ranks exchange) gives the same statistics
    n2 = ObsNormalizer(cols)
    for b in batches:
        n2.merge_sums(np.concatenate([b.sum(0), (b * b).sum(0), [b.shape[0]]]))
    # (sumsq / n - mean^2 cancels: eps_f64 mean^2 per batch)
    assert (np.abs(n2.var - var) <= 64 * EPS64 * K * np.maximum(var, mean * mean)).all()
    # first iteration: the identity-like initial state, y = x / 1.01
    x = rng.standard_normal((3, cols))
    assert np.allclose(ObsNormalizer(cols).normalize_host(x), x / 1.01, rtol=1e-6)


# ------------------------------------------------------------------ fold into the first layer / export
def _trained_normalizer(cols, seed=5):
    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    rng = np.random.default_rng(seed)
    norm = ObsNormalizer(cols)
    mean, std = rng.uniform(-2.0, 2.0, cols), 10.0 ** rng.uniform(-1.5, 0.7, cols)
    rows = mean + std * rng.standard_normal((4096, cols))
    norm.merge(rows.mean(0), rows.var(0), rows.shape[0])
    return norm, mean, std


def test_fold_into_first_layer_equals_the_actor_on_normalised_rows():
    from booster_gym_amd.utils.model import ActorCritic

    norm, mean, std = _trained_normalizer(61)
    torch.manual_seed(3)
    actor = ActorCritic(12, 47, 14).actor.double()
    x = torch.from_numpy(mean[:47] + std[:47] * np.random.default_rng(6).standard_normal((256, 47)))
    with torch.no_grad():
        want = actor(torch.from_numpy(norm.normalize_host(x.numpy())))
        w, b = norm.fold_into_first_layer(actor[0].weight, actor[0].bias, dtype=torch.float64)
        assert w.dtype == torch.float64 and w.shape == actor[0].weight.shape
        actor[0].weight.copy_(w); actor[0].bias.copy_(b)
        got = actor(x)
    # float64 round-off of a 47-term dot product whose terms reach |W'| |x| ~ |W| (|x| + |mean|) inv_std, through three more layers of gain ~1:
    # 1e-12 is four orders above eps_f64 x 47 x those magnitudes and seven below what a wrong fold (mean or inv_std misplaced) gives
    assert (got - want).abs().max() < 1e-12, float((got - want).abs().max())
    w32, b32 = norm.fold_into_first_layer(actor[0].weight, actor[0].bias)
    assert w32.dtype == b32.dtype == torch.float32


def test_export_model_folds_the_normaliser_of_a_checkpoint(tmp_path):
    """The real export_model.py on a temporary checkpoint with a non-trivial normaliser: the TorchScript module takes RAW observations and
    reproduces actor(normalise(x)) in fp32 to 1e-5, the tolerance of exported actions."""
    from booster_gym_amd.utils.model import ActorCritic

    norm, mean, std = _trained_normalizer(61, seed=9)
    torch.manual_seed(4)
    model = ActorCritic(12, 47, 14)
    ck = tmp_path / "model_1.pth"
    torch.save({"model": model.state_dict(), "obs_normalizer": norm.state_dict()}, ck)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={ck}"], cwd=tmp_path, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert re.search(r"Folded the observation normaliser \(61 columns", out.stdout), out.stdout
    scripted = torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"))
    x = torch.from_numpy((mean[:47] + std[:47] * np.random.default_rng(8).standard_normal((512, 47))).astype(np.float32))
    with torch.no_grad():
        want = model.actor(torch.from_numpy(norm.normalize_host(x.numpy())))
        got = scripted(x)
    assert got.dtype == torch.float32 and (got - want).abs().max() < 1e-5, float((got - want).abs().max())
    # a checkpoint without the entry exports as before, with no word about a normaliser
    torch.save({"model": model.state_dict()}, ck)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "export_model.py"), "--task=T1", f"--checkpoint={ck}"], cwd=tmp_path, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "normaliser" not in out.stdout
    with torch.no_grad():
        assert torch.equal(torch.jit.load(str(tmp_path / "deploy" / "models" / "T1.pt"))(x), model.actor(x))


def test_play_oracle_folds_the_normaliser(tmp_path):
    from booster_gym_amd.utils.model import ActorCritic

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import play_oracle
    finally:
        sys.path.pop(0)
    norm, mean, std = _trained_normalizer(61, seed=2)
    model = ActorCritic(12, 47, 14)
    ck = str(tmp_path / "m.pth")
    torch.save({"model": model.state_dict(), "obs_normalizer": norm.state_dict()}, ck)
    layers = play_oracle.load_actor(ck)
    x = mean[:47] + std[:47] * np.random.default_rng(1).standard_normal(47)
    h = norm.normalize_host(x)
    l0 = model.actor[0]
    want = l0.weight.detach().double().numpy() @ h + l0.bias.detach().double().numpy()
    got = layers[0][0].astype(np.float64) @ x + layers[0][1].astype(np.float64)
    assert np.abs(got - want).max() < 1e-5


# ------------------------------------------------------------------ checkpoint rules
def _runner_stub(norm, ck):
    """What Runner._load / Runner.checkpoint_dict read of a runner, without an env on a device."""
    from booster_gym_amd.utils.model import ACTOR_HIDDEN, CRITIC_HIDDEN, ActorCritic

    model = ActorCritic(12, 47, 14)
    env = types.SimpleNamespace(num_single_obs=47, num_envs=4, curriculum_prob=torch.zeros(3, 3), terrain=types.SimpleNamespace(curriculum=False))
    opt = types.SimpleNamespace(state_dict=lambda: {"state": {}}, load_state_dict=lambda sd: None)
    return types.SimpleNamespace(cfg={"basic": {"checkpoint": ck}}, device="cpu", model=model, env=env, optimizer=opt, obs_norm=norm, invalidate=lambda: None,
                                 actor_hidden=ACTOR_HIDDEN, critic_hidden=CRITIC_HIDDEN)


def test_checkpoint_rules(tmp_path):
    from booster_gym_amd.utils.obs_norm import ObsNormalizer
    from booster_gym_amd.utils.runner import Runner

    norm, _, _ = _trained_normalizer(61)
    # key false: exactly the parent's keys; key true: one more
    off = _runner_stub(None, None)
    assert sorted(Runner.checkpoint_dict(off)) == ["curriculum", "model", "optimizer"]
    on = _runner_stub(norm, None)
    d = Runner.checkpoint_dict(on)
    assert sorted(d) == ["curriculum", "model", "obs_normalizer", "optimizer"]
    assert sorted(d["obs_normalizer"]) == ["count", "eps", "mean", "var"]
    assert d["obs_normalizer"]["mean"].dtype == torch.float64 and d["obs_normalizer"]["count"] == 4096.0 and d["obs_normalizer"]["eps"] == 1.0e-2
    with_norm, without = str(tmp_path / "with.pth"), str(tmp_path / "without.pth")
    torch.save(d, with_norm)
    torch.save(Runner.checkpoint_dict(off), without)
    # round trip: a fresh normaliser takes the saved state, bit for bit
    fresh = _runner_stub(ObsNormalizer(61), with_norm)
    Runner._load(fresh)
    assert np.array_equal(fresh.obs_norm.mean, norm.mean) and np.array_equal(fresh.obs_norm.var, norm.var) and fresh.obs_norm.count == norm.count
    assert np.array_equal(fresh.obs_norm.inv_std32, norm.inv_std32)
    Runner._load(_runner_stub(None, without))
    # the three refusals
    with pytest.raises(ValueError, match=r"has no observation normaliser but the config sets algorithm\.empirical_normalization: true"):
        Runner._load(_runner_stub(ObsNormalizer(61), without))
    with pytest.raises(ValueError, match=r"carries an observation normaliser but the config has algorithm\.empirical_normalization: false"):
        Runner._load(_runner_stub(None, with_norm))
    with pytest.raises(ValueError, match=r"algorithm\.empirical_normalization: the checkpoint's normaliser has 61 columns, the config's networks read 248"):
        Runner._load(_runner_stub(ObsNormalizer(248), with_norm))
    # the config's eps is not replaced by the checkpoint's without a word
    with pytest.raises(ValueError, match=r"algorithm\.empirical_normalization.*algorithm\.normalization_eps = 0\.01, the config has 0\.05"):
        Runner._load(_runner_stub(ObsNormalizer(61, 0.05), with_norm))


def test_normalize_into_refuses_views_of_unequal_leading_shape():
    """The wrapper checks the views before the launch (no device is touched: the check comes first)."""
    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    norm = ObsNormalizer(61)
    src = torch.zeros(5, 8, 47)
    with pytest.raises(ValueError, match="equal leading shapes"):
        norm.normalize_into(src, torch.zeros(4, 8, 64), dst_cols=64)
    with pytest.raises(ValueError, match="equal leading shapes"):
        norm.normalize_into(src, torch.zeros(5, 8, 47), dst_cols=64)


# ------------------------------------------------------------------ C ABI
def test_library_declares_and_exports_the_two_entry_points():
    from booster_gym_amd import _lib

    header = open(os.path.join(ROOT, "include", "booster_gym_amd.h")).read()
    declared = set(re.findall(r"\b(bg_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for s in ("bg_obs_moments", "bg_obs_normalize"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert int(re.search(r"#define BG_OBS_MOMENTS_MAX_GROUPS (\d+)", header).group(1)) == _lib.OBS_MOMENTS_MAX_GROUPS


def test_abi_argument_errors_without_gpu():
    """Both entry points check their arguments on the host before any launch: null pointers, zero rows and more columns than supported are the
    project's argument error (-1) with the entry point's name in bg_last_error()."""
    from booster_gym_amd import _lib

    lib = _lib.load()
    f = (C.c_float * 1024)()
    d = (C.c_double * 4096)()
    mom = lambda rows=4, a=f, ca=47, sa=47, b=f, cb=14, sb=14, s=d, ss=d, sc=d: lib.bg_obs_moments(rows, a, ca, sa, b, cb, sb, s, ss, sc, None)
    for kw in (dict(rows=0), dict(a=None), dict(s=None), dict(ss=None), dict(sc=None), dict(b=None), dict(ca=513), dict(ca=0), dict(cb=202), dict(cb=-1),
               dict(sa=46), dict(sb=13)):
        assert mom(**kw) == -1 and b"bg_obs_moments" in lib.bg_last_error(), kw
    nrm = lambda rows=4, cols=47, src=f, ss=47, dst=d, dc=64, ds=64, mean=f, inv=f, col0=0: lib.bg_obs_normalize(rows, cols, src, ss, dst, dc, ds, mean, inv, col0, None)
    for kw in (dict(rows=0), dict(src=None), dict(dst=None), dict(mean=None), dict(inv=None), dict(cols=0), dict(cols=600, ss=600, dc=600, ds=600),
               dict(col0=700), dict(col0=-1), dict(ss=46), dict(dc=46), dict(ds=63), dict(dc=513, ds=513), dict(dst=f)):
        assert nrm(**kw) == -1 and b"bg_obs_normalize" in lib.bg_last_error(), kw


# ------------------------------------------------------------------ two gloo ranks
def _rows_of_rank(rank):
    rng = np.random.default_rng(100 + rank)
    n = 300 + 77 * rank  # the ranks need not hold equal row counts for the statistics to be right
    return np.array([0.5, -20.0, 3.0, 0.0, 1.0e3]) + np.array([1.0, 0.1, 30.0, 1.0e-3, 2.0]) * rng.standard_normal((n, 5))


def _norm_worker(rank, world, port, q):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), BG_DIST_BACKEND="gloo",
                      BG_DP_LOG_ORDER="1")
    sys.path.insert(0, ROOT)
    from booster_gym_amd.utils.obs_norm import ObsNormalizer
    from booster_gym_amd.utils.parallel import DataParallel

    torch.set_num_threads(1)
    dp = DataParallel()
    norm = ObsNormalizer(5)
    for it in range(2):  # two iterations: the second merges into statistics that are no longer the initial ones
        x = _rows_of_rank(rank) + it
        sums = torch.from_numpy(np.concatenate([x.sum(0), (x * x).sum(0), [x.shape[0]]]))
        norm.merge_exchanged(sums, dp)  # ONE float64 vector through DataParallel.sum_
    q.put((rank, norm.mean.tolist(), norm.var.tolist(), norm.count, dp.order_log))
    dp.shutdown()


def test_two_gloo_ranks_end_with_the_statistics_of_all_rows():
    import socket

    import torch.multiprocessing as mp

    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_norm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=180) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    single = ObsNormalizer(5)  # one process that holds all rows
    for it in range(2):
        x = np.concatenate([_rows_of_rank(0), _rows_of_rank(1)]) + it
        single.merge_sums(np.concatenate([x.sum(0), (x * x).sum(0), [x.shape[0]]]))
    (r0, m0, v0, c0, log0), (r1, m1, v1, c1, log1) = res
    assert (m0, v0, c0) == (m1, v1, c1)  # identical on both ranks, bit for bit
    assert c0 == single.count == 2 * (300 + 377)
    # against the single process: the only difference is the order of two float64 additions per sum (rank 0 + rank 1 against one pass over all rows):
    # a few eps_f64 relative to sumsq / n ~ var + mean^2
    tol = 16 * EPS64 * (single.var + single.mean**2)
    assert (np.abs(np.array(v0) - single.var) <= tol).all() and (np.abs(np.array(m0) - single.mean) <= 16 * EPS64 * np.abs(single.mean) + 1e-300).all()
    assert log0 == log1 == [("obs_norm", "main")] * 2  # one exchange per iteration, the same on both ranks
