"""sensors.enabled without a GPU: the section's rules (every refusal names its key), the section off in its three spellings, the host restatement of
the row rule (sensor_rows_ref, float64; tests/test_gpu_sensors.py holds bg_obs_sensor against it) on hand-built cases, the host restatement of the
episode's draws (host_draws, on oracle/task_ref.py's Philox), and the seed of the GPU test: its first episode has both floor(lam) = 0 and 1."""
import ctypes as C

import numpy as np
import pytest

from oracle.task_ref import rand4

SEED, N_GPU = 42, 37  # basic.seed and env.num_envs of tests/test_gpu_sensors.py
RS_SENSOR, RS_SENSOR_RESET, LAT_STREAM = 640, 656, 8
SENSOR_COLUMNS = tuple(range(0, 6)) + tuple(range(11, 35))
GROUP_OF = [0] * 3 + [1] * 3 + [2] * 12 + [3] * 12  # sensor column s -> gravity, ang_vel, dof_pos, dof_vel
GAUSS = lambda a, b: {"range": [a, b], "operation": "additive", "distribution": "gaussian"}
UNIF = lambda a, b: {"range": [a, b], "operation": "additive", "distribution": "uniform"}
FULL_BIAS = {"gravity": GAUSS(0.0, 0.05), "ang_vel": UNIF(-0.2, 0.2), "dof_pos": GAUSS(0.01, 0.03), "dof_vel": UNIF(-0.5, 0.3)}
LATENCY = [0.25, 1.75]


def env_seed(seed, rank=0):
    """bg_env_cfg.seed as envs/t1.py builds it from basic.seed and basic.rank."""
    return (int(seed) & 0xFFFFFFFF) | ((int(rank) + 1) << 32)


def host_draws(seed, n, step, reset_all, bias, latency, norms):
    """(beta [n][30], lam [n]) float64 that a reset at step counter `step` draws: beta[s] = apply_rand(0, bias of s's group) on entry s & 3 of stream
    base + (s >> 2), times the group's normalisation factor; lam = lo + (hi - lo) u on entry 0 of stream base + 8.  bias: {group: entry or None}."""
    base = RS_SENSOR_RESET if reset_all else RS_SENSOR
    envs = np.arange(n)
    beta = np.zeros((n, 30))
    names = ("gravity", "ang_vel", "dof_pos", "dof_vel")
    for s in range(30):
        entry = bias.get(names[GROUP_OF[s]])
        if entry is None:
            continue
        u, nr = rand4(seed, envs, step, base + (s >> 2))
        a, b = entry["range"]
        draw = a + b * nr[:, s & 3].astype(np.float64) if entry["distribution"] == "gaussian" else a + (b - a) * u[:, s & 3].astype(np.float64)
        beta[:, s] = draw * norms[GROUP_OF[s]]
    u, _ = rand4(seed, envs, step, base + LAT_STREAM)
    lam = latency[0] + (latency[1] - latency[0]) * u[:, 0].astype(np.float64)
    return beta, lam


def sensor_rows_ref(obs, dones, bias, lat, H):
    """The row rule in float64.  obs[t]: [N][47] single observation the env stored at call t (t = 0: reset-all); dones[t]: [N] bool, the envs call t
    reset (all of them at t = 0); bias[t]: [N][30] and lat[t]: [N] as they stand after call t; H: frames.  Returns (rows [T][N][47 H], mag [T][N][47 H]):
    mag = |a| + |b| + |beta| on the sensor columns of live frames, 0 where the element is exact (zero frames, non-sensor columns)."""
    T, N = len(obs), obs[0].shape[0]
    obs = [np.asarray(o, dtype=np.float64) for o in obs]
    sens = list(SENSOR_COLUMNS)
    age = np.zeros(N, dtype=np.int64)
    rows, mags = [], []
    rng = np.arange(N)
    for t in range(T):
        age = np.where(np.asarray(dones[t], dtype=bool), 0, age + 1)
        assert (age <= t).all()

        def o(j):  # o~_e(j) = o_e(min(j, age_e))
            jj = np.minimum(j, age)
            return np.stack([obs[t - jj[e]][e] for e in rng])

        lam = np.asarray(lat[t], dtype=np.float64)
        i = np.floor(lam).astype(np.int64)
        f = (lam - i)[:, None]
        beta = np.asarray(bias[t], dtype=np.float64)
        row, mag = np.zeros((N, H, 47)), np.zeros((N, H, 47))
        for k in range(H):
            d = H - 1 - k
            live = (d <= age)[:, None]
            v = o(np.full(N, d))
            a, b = o(d + i)[:, sens], o(d + i + 1)[:, sens]
            v[:, sens] = a + f * (b - a) + beta
            m = np.zeros((N, 47))
            m[:, sens] = np.abs(a) + np.abs(b) + np.abs(beta)
            row[:, k], mag[:, k] = np.where(live, v, 0.0), np.where(live, m, 0.0)
        rows.append(row.reshape(N, H * 47))
        mags.append(mag.reshape(N, H * 47))
    return rows, mags


def _on(**over):
    from booster_gym_amd.utils.config import load_cfg

    return load_cfg("T1", {"sensors.enabled": True, **over})


def test_defaults_and_the_section_off():
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.sensors import DEFAULTS, GROUPS, NUM_SENSOR_COLUMNS, SENSOR_COLUMNS as COLS, SensorsCfg, sensors_cfg, sensors_enabled

    assert GROUPS == ("gravity", "ang_vel", "dof_pos", "dof_vel") and COLS == SENSOR_COLUMNS and NUM_SENSOR_COLUMNS == 30
    assert [s for s, c in enumerate(COLS) if s != (c if c < 6 else c - 5)] == []
    assert DEFAULTS == {"enabled": False, "bias": {g: None for g in GROUPS}, "latency_steps": [0.0, 0.0]}
    absent = load_cfg("T1")
    absent.pop("sensors", None)
    assert sensors_cfg(absent) is None and not sensors_enabled(absent)
    null = load_cfg("T1")
    null["sensors"] = None
    assert sensors_cfg(null) is None
    assert sensors_cfg(load_cfg("T1", {"sensors.enabled": False})) is None
    assert sensors_cfg(load_cfg("T1", {"sensors.enabled": None})) is None
    sparse = load_cfg("T1")
    sparse["sensors"] = {}
    assert sensors_cfg(sparse) is None  # `enabled` absent
    # off: nothing else of the section is read
    assert sensors_cfg(load_cfg("T1", {"sensors.enabled": False, "sensors.latency_steps": "nonsense", "sensors.momentum": 1, "sensors.bias": 7})) is None
    on = sensors_cfg(_on())
    assert on == SensorsCfg((None, None, None, None), (0.0, 0.0)) and on.extra_planes == 0
    assert sensors_cfg(_on(**{"sensors.bias": None, "sensors.latency_steps": None})) == on
    assert sensors_cfg(_on(**{"sensors.bias": dict(DEFAULTS["bias"]), "sensors.latency_steps": [0.0, 0.0]})) == on
    got = sensors_cfg(_on(**{"sensors.bias": FULL_BIAS, "sensors.latency_steps": LATENCY}))
    assert got.bias == tuple(FULL_BIAS[g] for g in GROUPS) and got.latency_steps == (0.25, 1.75) and got.extra_planes == 2
    assert sensors_cfg(_on(**{"sensors.latency_steps": [1, 1]})).extra_planes == 1
    assert sensors_cfg(_on(**{"sensors.latency_steps": [0, 0.5]})).extra_planes == 1
    assert sensors_cfg(_on(**{"sensors.latency_steps": [2, 2]})).extra_planes == 2
    assert sensors_cfg(_on(**{"sensors.bias.dof_pos": UNIF(0.3, -0.3)})).bias[2]["range"] == [0.3, -0.3]  # (apply_rand's low + (high - low) u takes any order)


@pytest.mark.parametrize("over,match", [
    ({"sensors.enabled": 1}, r"sensors\.enabled must be true or false"),
    ({"sensors.enabled": "yes"}, r"sensors\.enabled must be true or false"),
    ({"sensors.momentum": 1}, r"sensors\.momentum is not a key"),
    ({"sensors.bias": [1]}, r"sensors\.bias must be null or a mapping"),
    ({"sensors.bias.lin_vel": GAUSS(0, 1)}, r"sensors\.bias\.lin_vel is not a group"),
    ({"sensors.bias.gravity": 0.1}, r"sensors\.bias\.gravity must be null or an entry"),
    ({"sensors.bias.gravity": dict(GAUSS(0, 1), scale=2)}, r"sensors\.bias\.gravity\.scale is not a key"),
    ({"sensors.bias.ang_vel": dict(GAUSS(0, 1), operation="scaling")}, r"sensors\.bias\.ang_vel\.operation"),
    ({"sensors.bias.ang_vel": {"range": [0, 1], "distribution": "gaussian"}}, r"sensors\.bias\.ang_vel\.operation"),
    ({"sensors.bias.dof_pos": dict(GAUSS(0, 1), distribution="laplace")}, r"sensors\.bias\.dof_pos\.distribution"),
    ({"sensors.bias.dof_pos": {"range": [0, 1], "operation": "additive"}}, r"sensors\.bias\.dof_pos\.distribution"),
    ({"sensors.bias.dof_vel": GAUSS(0, float("inf"))}, r"sensors\.bias\.dof_vel\.range"),
    ({"sensors.bias.dof_vel": GAUSS(float("nan"), 1)}, r"sensors\.bias\.dof_vel\.range"),
    ({"sensors.bias.dof_vel": {"range": [0, 1, 2], "operation": "additive", "distribution": "uniform"}}, r"sensors\.bias\.dof_vel\.range"),
    ({"sensors.bias.dof_vel": {"range": 0.1, "operation": "additive", "distribution": "uniform"}}, r"sensors\.bias\.dof_vel\.range"),
    ({"sensors.bias.dof_vel": {"range": [0, True], "operation": "additive", "distribution": "uniform"}}, r"sensors\.bias\.dof_vel\.range"),
    ({"sensors.bias.gravity": GAUSS(0.0, -0.1)}, r"sensors\.bias\.gravity\.range.*std"),
    ({"sensors.latency_steps": [0.5, 0.25]}, r"sensors\.latency_steps"),
    ({"sensors.latency_steps": [-0.1, 1]}, r"sensors\.latency_steps"),
    ({"sensors.latency_steps": [0, 2.5]}, r"sensors\.latency_steps"),
    ({"sensors.latency_steps": [0, float("nan")]}, r"sensors\.latency_steps"),
    ({"sensors.latency_steps": 1}, r"sensors\.latency_steps"),
    ({"sensors.latency_steps": [0, 1, 2]}, r"sensors\.latency_steps"),
    ({"terrain.measure_heights": True, "terrain.actor_heights": True}, r"sensors\.enabled.*terrain\.actor_heights"),
])
def test_every_refusal_names_its_key(over, match):
    from booster_gym_amd.utils.sensors import sensors_cfg

    with pytest.raises(ValueError, match=match):
        sensors_cfg(_on(**over))


def test_the_section_must_be_a_mapping_and_other_validators_keep_their_behaviour():
    from booster_gym_amd.envs.t1 import check_env_sizes, frame_stack_of
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.estimator import estimator_cfg
    from booster_gym_amd.utils.rnd import rnd_cfg
    from booster_gym_amd.utils.sensors import sensors_cfg

    with pytest.raises(ValueError, match=r"sensors must be a mapping"):
        sensors_cfg({"sensors": [1]})
    on = _on(**{"sensors.bias": FULL_BIAS, "sensors.latency_steps": LATENCY})
    assert frame_stack_of(on) == 1 and check_env_sizes(on, 0) is None and estimator_cfg(on) is None and rnd_cfg(on) is None
    stacked = _on(**{"env.frame_stack": 3, "env.num_observations": 141})
    assert frame_stack_of(stacked) == 3 and check_env_sizes(stacked, 0) is None  # the row's width is env.frame_stack's alone
    both = load_cfg("T1", {"sensors.enabled": True, "estimator.enabled": True, "rnd.enabled": True, "rnd.weight": 0.5})
    plain = load_cfg("T1", {"estimator.enabled": True, "rnd.enabled": True, "rnd.weight": 0.5})
    assert estimator_cfg(both) == estimator_cfg(plain) and rnd_cfg(both) == rnd_cfg(plain)


def test_struct_fields_stand_behind_the_existing_ones_and_zero_is_off():
    from booster_gym_amd import _lib

    E = _lib.EnvCfg
    assert E.sensor_model.offset == E.priv_clearance_scale.offset + 4
    assert [E.sensor_bias_gravity.offset, E.sensor_bias_ang_vel.offset, E.sensor_bias_dof_pos.offset, E.sensor_bias_dof_vel.offset] == \
        [E.sensor_model.offset + 4 + 12 * g for g in range(4)]
    assert E.sensor_latency_lo.offset == E.sensor_bias_dof_vel.offset + C.sizeof(_lib.Rand) and E.sensor_latency_hi.offset == E.sensor_latency_lo.offset + 4
    assert E.sensor_latency_hi.offset + 4 <= C.sizeof(E)
    z = E()
    assert z.sensor_model == 0 and z.sensor_bias_dof_vel.mode == 0 and z.sensor_latency_hi == 0.0
    assert "bg_env_sensor_launches" in _lib.SYMBOLS


def test_env_create_rejects_an_inconsistent_sensor_model_without_gpu(flat_model):
    """bg_env_create checks the sensor fields before it touches the device; a consistent struct gets as far as the device check."""
    import torch

    from booster_gym_amd import _lib

    lib = _lib.load()
    m = flat_model
    d = _lib.ModelDesc(); d.num_bodies, d.num_dofs = 13, 12
    for b in range(13):
        d.parent[b], d.joint_axis[b], d.mass[b] = int(m.parent[b]), int(m.joint_axis[b]), float(m.mass[b])
    model = C.c_void_p()
    assert lib.bg_model_create(C.byref(d), C.byref(model)) == 0

    def create(**fields):
        cfg = _lib.EnvCfg(); cfg.num_envs, cfg.decimation, cfg.sim_dt, cfg.sensor_model = 4, 10, 0.002, 1
        for k, v in fields.items():
            if isinstance(v, tuple):
                r = getattr(cfg, k); r.mode, r.a, r.b = v
            else:
                setattr(cfg, k, v)
        env = C.c_void_p()
        return lib.bg_env_create(C.byref(cfg), model, C.byref(env)), lib.bg_last_error()

    try:
        bad = [({"sensor_model": 2}, b"sensor_model"), ({"actor_heights": 1, "height_scan_points": 0}, b"actor_heights"),
               ({"sensor_bias_gravity": (2, 0.0, 1.0)}, b"sensor_bias"), ({"sensor_bias_ang_vel": (4, 0.0, 1.0)}, b"sensor_bias"),
               ({"sensor_bias_dof_pos": (1, 0.0, -1.0)}, b"sensor_bias"), ({"sensor_bias_dof_vel": (3, float("inf"), 1.0)}, b"sensor_bias"),
               ({"sensor_bias_dof_vel": (1, 0.0, float("nan"))}, b"sensor_bias"),
               ({"sensor_latency_lo": 1.0, "sensor_latency_hi": 0.5}, b"sensor_latency"), ({"sensor_latency_lo": -0.5, "sensor_latency_hi": 0.5}, b"sensor_latency"),
               ({"sensor_latency_hi": 2.5}, b"sensor_latency"), ({"sensor_latency_hi": float("nan")}, b"sensor_latency")]
        for fields, word in bad:
            rc, msg = create(**fields)
            assert rc == -1 and word in msg, (fields, msg)
        if not torch.cuda.is_available():
            for fields in ({}, {"sensor_bias_gravity": (1, 0.0, 0.05), "sensor_bias_dof_vel": (3, -0.5, 0.3), "sensor_latency_lo": 0.25, "sensor_latency_hi": 2.0},
                           {"frame_stack": 10, "sensor_latency_lo": 2.0, "sensor_latency_hi": 2.0}):
                rc, msg = create(**fields)
                assert rc == -3 and b"no HIP device" in msg, (fields, msg)
    finally:
        lib.bg_model_destroy(model)


def _toy(T, N, seed=0):
    r = np.random.default_rng(seed)
    return [r.normal(size=(N, 47)).astype(np.float32) for _ in range(T)]


def test_row_rule_by_hand():
    T, N, H = 7, 3, 3
    obs = _toy(T, N)
    dones = [np.ones(N, bool)] + [np.zeros(N, bool) for _ in range(T - 1)]
    dones[4] = np.array([False, True, False])  # env 1 resets at call 4
    beta = np.zeros((N, 30)); beta[:, 0] = 0.5; beta[2, 29] = -1.25
    lam = np.array([0.0, 1.0, 1.5])  # env 0: no delay; env 1: one whole step (f = 0); env 2: between one and two steps
    rows, mags = sensor_rows_ref(obs, dones, [beta] * T, [lam] * T, H)
    sens, rest = list(SENSOR_COLUMNS), [c for c in range(47) if c not in SENSOR_COLUMNS]
    assert len(rest) == 17 and rest == list(range(6, 11)) + list(range(35, 47))
    fr = lambda t, e, k: rows[t][e].reshape(H, 47)[k]
    # zero frames: after reset-all the two older frames, one call later the oldest; for env 1 again after its reset at call 4
    assert not fr(0, 0, 0).any() and not fr(0, 0, 1).any() and fr(0, 0, 2).any()
    assert not fr(1, 2, 0).any() and fr(1, 2, 1).any()
    assert not fr(4, 1, 0).any() and not fr(4, 1, 1).any() and not fr(5, 1, 0).any() and fr(5, 1, 1).any() and fr(6, 1, 0).any()
    assert not mags[4][1].reshape(H, 47)[:2].any() and not mags[0][0].reshape(H, 47)[:, rest].any()
    # untouched non-sensor columns: frame k is the observation of H - 1 - k calls ago, bit for bit
    for t, e, k in ((6, 0, 0), (6, 1, 1), (6, 2, 2), (3, 2, 0), (5, 1, 2)):
        assert np.array_equal(fr(t, e, k)[rest], obs[t - (H - 1 - k)][e][rest].astype(np.float64))
    # env 0, no delay: the sensor columns are the same observation plus the bias
    want = obs[6][0].astype(np.float64)[sens] + beta[0]
    assert np.array_equal(fr(6, 0, 2)[sens], want) and fr(6, 0, 2)[0] == obs[6][0][0] + 0.5
    # env 1, lam = 1 (f = 0): exactly the observation one call earlier; age clamp: at its reset (call 4) and the first reading of the episode after it
    assert np.array_equal(fr(3, 1, 2)[sens], obs[2][1].astype(np.float64)[sens] + beta[1])
    assert np.array_equal(fr(4, 1, 2)[sens], obs[4][1].astype(np.float64)[sens] + beta[1])  # age 0: o~(1) = o(0)
    assert np.array_equal(fr(5, 1, 2)[sens], obs[4][1].astype(np.float64)[sens] + beta[1])  # age 1: o(1)
    assert np.array_equal(fr(5, 1, 1)[sens], obs[4][1].astype(np.float64)[sens] + beta[1])  # d = 1, i = 1: o~(2) = o(1), never call 3 of the episode before
    # env 2, lam = 1.5: half way between one and two calls ago; clamped to the episode's first reading while the episode is young
    a, b = obs[5][2].astype(np.float64)[sens], obs[4][2].astype(np.float64)[sens]
    assert np.allclose(fr(6, 2, 2)[sens], a + 0.5 * (b - a) + beta[2], rtol=0, atol=1e-15)
    assert np.array_equal(mags[6][2].reshape(H, 47)[2][sens], np.abs(a) + np.abs(b) + np.abs(beta[2]))
    assert np.array_equal(fr(1, 2, 2)[sens], obs[0][2].astype(np.float64)[sens] + beta[2])  # age 1: a = b = o(1) = the reset's observation
    a, b = obs[1][2].astype(np.float64)[sens], obs[0][2].astype(np.float64)[sens]
    assert np.allclose(fr(2, 2, 2)[sens], a + 0.5 * (b - a) + beta[2], rtol=0, atol=1e-15)  # age 2: o(1) and o~(2) = o(2)
    assert np.allclose(fr(2, 2, 1)[sens], b + beta[2], rtol=0, atol=1e-15)  # d = 1: o~(2) and o~(3), both the reset's
    # H = 1: the one frame, never zero
    r1, _ = sensor_rows_ref(obs, dones, [beta] * T, [lam] * T, 1)
    assert all(np.array_equal(r1[t][e], fr(t, e, 2)) for t in range(T) for e in range(N))


def test_draw_addressing_and_the_gpu_tests_seed():
    seed = env_seed(SEED)
    norms = (1.0, 1.0, 1.0, 0.1)
    beta, lam = host_draws(seed, N_GPU, 0, True, FULL_BIAS, LATENCY, norms)
    assert ((lam >= 0.25) & (lam < 1.75)).all()
    fl = np.floor(lam)
    assert (fl == 0).any() and (fl == 1).any(), "choose another SEED: the first episode must hold both floor(lam) = 0 and floor(lam) = 1"
    # a uniform group stays in its range times the factor, a gaussian one scatters around its mean
    assert (np.abs(beta[:, 3:6]) <= 0.2).all() and ((beta[:, 18:] >= -0.05) & (beta[:, 18:] <= 0.03)).all()
    assert abs(beta[:, 6:18].mean() - 0.01) < 0.01 and 0.02 < beta[:, 6:18].std() < 0.04 and 0.03 < beta[:, :3].std() < 0.07
    # entry s & 3 of stream base + (s >> 2): column 5 is entry 1 of stream 1, column 29 entry 1 of stream 7
    u1, _ = rand4(seed, np.arange(N_GPU), 0, RS_SENSOR_RESET + 1)
    assert np.allclose(beta[:, 5], -0.2 + 0.4 * u1[:, 1].astype(np.float64), rtol=0, atol=1e-15)
    u7, _ = rand4(seed, np.arange(N_GPU), 0, RS_SENSOR_RESET + 7)
    assert np.allclose(beta[:, 29], (-0.5 + 0.8 * u7[:, 1].astype(np.float64)) * 0.1, rtol=0, atol=1e-15)
    # a step's reset draws from the other base and its own counter; a group without an entry has no bias
    b2, l2 = host_draws(seed, N_GPU, 5, False, {"ang_vel": FULL_BIAS["ang_vel"]}, [1.0, 1.0], norms)
    assert not b2[:, :3].any() and not b2[:, 6:].any() and b2[:, 3:6].any() and not np.array_equal(b2[:, 3:6], beta[:, 3:6]) and (l2 == 1.0).all()
    u0, _ = rand4(seed, np.arange(N_GPU), 5, RS_SENSOR + 0)
    assert np.allclose(b2[:, 3], -0.2 + 0.4 * u0[:, 3].astype(np.float64), rtol=0, atol=1e-15)
    from booster_gym_amd.utils import sensors

    assert (sensors.RS_SENSOR, sensors.RS_SENSOR_RESET, sensors.RS_SENSOR_LATENCY) == (RS_SENSOR, RS_SENSOR_RESET, LAT_STREAM)
