"""The addressing of the exploration noise, on the oracle: actions = mu + exp(logstd) n with n = rand4(seed, row, counter, RS_ACTOR + g).n[k] for action
a = 4 g + k (include/booster_gym_amd.h).  tests/test_gpu_action_noise.py pins every sampling launch to these draws; this file checks that the draws so
addressed are what a policy's exploration needs them to be: standard normal per action column, uncorrelated between the 12 actions of a row, between
neighbouring rows and between one counter and the next.  No GPU.

4,096 rows x 12 draws at three (seed, counter) pairs.  Every statistic is bounded by 5 / sqrt(4096) = 0.078, five standard errors of a mean or of a
correlation of 4,096 independent pairs.  Measured on the oracle: |mean| at most 0.041, |std - 1| 0.022, the largest correlation of two action
columns 0.050, of a column with itself one row on 0.050, of counter against counter + 1 0.032; the largest |n| stays below 6 (the 24-bit uniform
bounds it at sqrt(-2 log(2^-25)) = 5.89)."""
import numpy as np
import pytest

from oracle.task_ref import RS_ACTOR, rand4

ROWS, A = 4096, 12
BOUND = 5.0 / np.sqrt(ROWS)
PAIRS = [(5, 3), (987654321, 23), (42 | 1 << 32, 0)]


def action_noise(seed, rows, counter):
    """[rows][12] float32: the draw of every action of every row, as the header addresses it."""
    return np.concatenate([rand4(seed, rows, counter, RS_ACTOR + g)[1] for g in range(A // 4)], axis=1)


def _corr(x, y):
    x, y = x - x.mean(0), y - y.mean(0)
    return (x * y).sum(0) / np.sqrt((x * x).sum(0) * (y * y).sum(0))


@pytest.mark.parametrize("seed,counter", PAIRS)
def test_the_documented_draws_are_independent_standard_normals(seed, counter):
    n = action_noise(seed, np.arange(ROWS), counter).astype(np.float64)
    assert n.shape == (ROWS, A) and np.isfinite(n).all()
    mean, std = np.abs(n.mean(0)).max(), np.abs(n.std(0, ddof=1) - 1.0).max()
    c = np.corrcoef(n, rowvar=False)
    cross = np.abs(c - np.eye(A)).max()
    lag = np.abs(_corr(n[:-1], n[1:])).max()
    nxt = action_noise(seed, np.arange(ROWS), counter + 1).astype(np.float64)
    step = np.abs(_corr(n, nxt)).max()
    print(f"seed {seed} counter {counter}: |mean| {mean:.3f}, |std - 1| {std:.3f}, columns {cross:.3f}, lag-1 over rows {lag:.3f}, counter + 1 {step:.3f}, "
          f"largest |n| {np.abs(n).max():.3f}; bound {BOUND:.3f}")
    assert mean <= BOUND and std <= BOUND and cross <= BOUND and lag <= BOUND and step <= BOUND
    assert np.abs(n).max() < 6.0
    assert not np.array_equal(n, nxt)


def test_every_word_of_the_address_moves_the_draw():
    """Seed (either word), row, counter and group each select another draw: no two of the 12 x 4096 draws of a call coincide beyond chance."""
    rows = np.arange(ROWS)
    base = action_noise(5, rows, 3)
    assert len(np.unique(base)) > 0.999 * base.size
    for other in (action_noise(5 | 1 << 32, rows, 3), action_noise(6, rows, 3), action_noise(5, rows, 4), action_noise(5, rows + 1, 3)):
        assert (other != base).mean() > 0.999
    assert np.array_equal(action_noise(5, rows + 1, 3)[:-1], base[1:])
