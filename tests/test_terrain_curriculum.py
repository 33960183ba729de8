"""Terrain curriculum (terrain.curriculum, an addition of this build): config validation, the levelled height field and the initial levels /
columns / origins.  CPU only; the level update in the env step is tests/test_gpu_terrain_curriculum.py."""
import hashlib

import numpy as np
import pytest

from booster_gym_amd.utils.config import load_cfg
from booster_gym_amd.utils.terrain import Terrain

# SHA-256 of the shipped config's height field at seed 42 (curriculum off): the field this build has always generated
DEFAULT_FIELD_SHA256 = "7e9145d086d114e05603ac77e6f796cbb5a6e6b0847507178701f3362606121f"


def _tcfg(**over):
    t = dict(load_cfg("T1")["terrain"])
    t.update(over)
    return t


@pytest.mark.parametrize("over, key", [
    ({"type": "plane", "curriculum": True}, "terrain.curriculum"),
    ({"curriculum": True, "num_levels": 0, "max_init_level": 0}, "terrain.num_levels"),
    ({"curriculum": True, "num_levels": 5, "max_init_level": 5}, "terrain.max_init_level"),
    ({"curriculum": True, "num_levels": 5, "max_init_level": -1}, "terrain.max_init_level"),
])
def test_config_validation_names_the_key(over, key):
    from booster_gym_amd.envs import T1

    cfg = load_cfg("T1", {"env.num_envs": 4, **{"terrain." + k: v for k, v in over.items()}})
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        T1(cfg)


def test_curriculum_off_and_absent_keys_are_today():
    hf = Terrain("cpu", _tcfg(), seed=42).height_field_raw
    assert hf.shape == (900, 200)
    assert hashlib.sha256(np.ascontiguousarray(hf).tobytes()).hexdigest() == DEFAULT_FIELD_SHA256
    absent = {k: v for k, v in _tcfg().items() if k not in ("curriculum", "num_levels", "max_init_level")}
    assert np.array_equal(Terrain("cpu", absent, seed=42).height_field_raw, hf)
    # the level keys are not read while the curriculum is off
    assert np.array_equal(Terrain("cpu", _tcfg(num_levels=3, max_init_level=2), seed=42).height_field_raw, hf)


def test_one_level_equals_curriculum_off():
    for seed in (0, 42, 7):
        off = Terrain("cpu", _tcfg(), seed=seed)
        on = Terrain("cpu", _tcfg(curriculum=True, num_levels=1, max_init_level=0), seed=seed)
        assert on.height_field_raw.dtype == off.height_field_raw.dtype
        assert np.array_equal(on.height_field_raw, off.height_field_raw)
        assert (on.env_width, on.env_length) == (off.env_width, off.env_length)


def test_field_shape_and_per_tile_amplitude():
    L, T = 4, 6
    c = _tcfg(curriculum=True, num_levels=L, max_init_level=1, num_terrains=T, terrain_proportions=[0.0, 2.0, 2.0, 2.0],
              slope=0.2, random_height=0.2, discrete_height=0.1)
    t = Terrain("cpu", c, seed=3)
    hf, b = t.height_field_raw, t.border_pixels
    wpx, lpx = int(c["terrain_width"] / c["horizontal_scale"]), int(c["terrain_length"] / c["horizontal_scale"])
    assert hf.shape == (T * wpx + 2 * b, L * lpx + 2 * b)
    assert t.env_length == L * c["terrain_length"] and t.env_width == T * c["terrain_width"]
    vs = c["vertical_scale"]
    tile = lambda lv, col: hf[b + col * wpx : b + (col + 1) * wpx, b + lv * lpx : b + (lv + 1) * lpx]
    kinds = {"slope": (0, 1), "random": (2, 3), "discrete": (4, 5)}
    # the top level is the field without the curriculum (same amplitudes), lower levels are scaled by (l + 1) / L to within one height unit
    for kind, cols in kinds.items():
        for col in cols:
            top = np.abs(tile(L - 1, col)).max()
            assert top > 0
            for lv in range(L):
                k = (lv + 1) / L
                m = np.abs(tile(lv, col)).max()
                if kind == "discrete":
                    assert m <= int(c["discrete_height"] * k / vs) and m >= k * top - 1, (kind, lv, m)
                else:
                    assert abs(m - k * top) <= 1.0, (kind, lv, m, top)
            if kind == "random":
                assert np.abs(tile(L - 1, col)).max() <= 0.5 * c["random_height"] / vs
    # platforms (slope and discrete tiles): flat around the tile centre on every level
    for col in kinds["slope"] + kinds["discrete"]:
        for lv in range(L):
            centre = tile(lv, col)[wpx // 2 - 5 : wpx // 2 + 5, lpx // 2 - 5 : lpx // 2 + 5]
            assert (centre == centre[0, 0]).all(), (col, lv)
    # the border stays flat
    assert (hf[:b] == 0).all() and (hf[:, :b] == 0).all() and (hf[-b:] == 0).all() and (hf[:, -b:] == 0).all()


def _origins(n, seed=42, rank=0, **terrain):
    """T1's initial origin assignment without the native env (the part of T1.__init__ that runs before the library is touched)."""
    from booster_gym_amd.envs import T1

    cfg = load_cfg("T1", {"env.num_envs": n, "basic.seed": seed, **{"terrain." + k: v for k, v in terrain.items()}})
    cfg["basic"]["rank"] = rank
    env = T1.__new__(T1)
    env.cfg, env.num_envs, env.device, env._env = cfg, n, "cpu", None
    env.terrain = Terrain("cpu", cfg["terrain"], seed=seed)
    env._get_env_origins()
    return env, cfg


def test_initial_levels_columns_and_origins():
    from booster_gym_amd.envs.t1 import TERRAIN_LEVEL_STREAM

    n = 1000
    env, cfg = _origins(n, curriculum=True, num_levels=10, max_init_level=4)
    levels, cols = env._terrain_init
    T = cfg["terrain"]["num_terrains"]
    # columns: floor(i / (N / num_terrains)), legged_gym's rule
    assert np.array_equal(cols, np.floor(np.arange(n) / (n / T)).astype(np.int32))
    assert cols.min() == 0 and cols.max() == T - 1
    # levels: uniform in [0, max_init_level] from a generator of their own, seeded from basic.seed (and the rank)
    want = np.random.default_rng([42, 0, TERRAIN_LEVEL_STREAM]).integers(0, 5, size=n)
    assert np.array_equal(levels, want)
    assert set(np.unique(levels).tolist()) == {0, 1, 2, 3, 4}
    assert abs(levels.mean() - 2.0) < 0.2
    # origins: tile centres at the height of the field there
    t = env.terrain
    o = env._origins
    assert np.allclose(o[:, 0], (cols + 0.5) * cfg["terrain"]["terrain_width"])
    assert np.allclose(o[:, 1], (levels + 0.5) * cfg["terrain"]["terrain_length"])
    hf, b = t.height_field_raw, t.border_pixels
    ix = np.rint(b + o[:, 0] / t.horizontal_scale).astype(int)
    iy = np.rint(b + o[:, 1] / t.horizontal_scale).astype(int)
    assert np.allclose(o[:, 2], hf[ix, iy] * t.vertical_scale, atol=1e-9)
    assert np.allclose(env.env_origins.numpy(), o, atol=1e-6)
    # another rank draws other levels, the same columns
    env1, _ = _origins(n, rank=1, curriculum=True, num_levels=10, max_init_level=4)
    assert np.array_equal(env1._terrain_init[1], cols) and not np.array_equal(env1._terrain_init[0], levels)


def test_initial_origins_without_curriculum_unchanged():
    env_off, _ = _origins(300)
    env_abs, _ = _origins(300, num_levels=3)  # level keys unread while the curriculum is off
    assert not hasattr(env_off, "_terrain_init")
    assert np.array_equal(env_off._origins, env_abs._origins)
    t = env_off.terrain
    num_cols = max(1.0, np.floor(np.sqrt(300 * t.env_length / t.env_width)))
    num_rows = np.ceil(300 / num_cols)
    assert np.isclose(env_off._origins[0, 0], t.env_width / (num_rows + 1)) and np.isclose(env_off._origins[0, 1], t.env_length / (num_cols + 1))
