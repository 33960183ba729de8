"""distillation.student_sensors at the env (bg_env_cfg.sensor_model = 2): the student's row of bg_obs_assemble<.., SENSOR> against
tests/test_sensors.py's float64 restatement of the row rule and of the episode's draws, against the actor's row of the env its student re-enters
(bg_obs_sensor, bit for bit), and everything the key must leave alone (the teacher's row, the privileged row, the physics).

Shapes: N = 37 (a ragged last block of ASM_ENVS = 4) and N = 1, the teacher's H in (1, 2), Hs in (H, 3), a scan of 3 x 2 points (P = 6) on trimesh
terrain, reset-all and 14 steps under rewards.episode_length_s: 0.1, so every env resets at its sixth step (envs that fall reset earlier and are taken
as they come: every check reads the run's own done flags), one case under sim.state_dtype: fp16.  Actions are a seeded tensor per step.

BOUNDS (tests/test_gpu_sensors.py's, derived there).  Rows: 4 x 2^-24 x (|a| + |b| + |beta|) per sensor element (b - a, f x, a +, + beta: four fp32
roundings on operands no larger than that sum); zero frames and the 17 other columns are exact; no element is left out.  Draws: a gaussian bias
inherits the device's normal draw (4 x 2.27e-6, tests/test_gpu_action_noise.py) times std x norm plus four fp32 roundings of the affine map; the
uniforms are exact bits, so a uniform bias and the latency carry the roundings alone."""
import numpy as np
import pytest
import torch

from test_sensors import FULL_BIAS, GAUSS, SEED, SENSOR_COLUMNS, UNIF, env_seed, host_draws, sensor_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, N_BIG, P = 14, 37, 6
REST = [c for c in range(47) if c not in SENSOR_COLUMNS]
NORMAL_DRAW = 2.27e-6  # tests/test_gpu_action_noise.py MEASURED: the device's normal draw against the oracle's, bounded there by 4 x this
LAT = [0.0, 1.5]
FULL = {"bias": FULL_BIAS, "latency_steps": LAT}
ABSENT = "absent"
SHAPES = [(N_BIG, 1, 1, False), (N_BIG, 1, 3, False), (N_BIG, 2, 2, False), (N_BIG, 2, 3, False), (1, 1, 1, False), (1, 2, 3, False), (N_BIG, 1, 3, True)]


def _base(n, H, Hs, sensors, fp16):
    """The distillation's config: the perceptive teacher's, with distillation.student_frame_stack and distillation.student_sensors."""
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": n, "basic.sim_device": DEV, "basic.rl_device": DEV, "basic.seed": SEED, "rewards.episode_length_s": 0.1, "terrain.type": "trimesh",
          "env.frame_stack": H, "terrain.measure_heights": True, "terrain.actor_heights": True, "terrain.measured_points_x": [-0.2, 0.0, 0.2],
          "terrain.measured_points_y": [-0.1, 0.1], "env.num_observations": 47 * H + P, "env.num_privileged_obs": 14 + P,
          "distillation.student_frame_stack": Hs}
    if fp16:
        ov["sim.state_dtype"] = "fp16"
    cfg = load_cfg("T1", ov)
    if isinstance(sensors, str) and sensors == ABSENT:
        del cfg["distillation"]["student_sensors"]
    else:
        cfg["distillation"]["student_sensors"] = sensors
    return cfg, ov


def _teacher_cfg(n, H, Hs, sensors, fp16):
    """... as the Distiller hands it to the env: env.student_frame_stack (here also with the key absent: the comparisons need the row) and
    env.student_sensors."""
    from booster_gym_amd.utils.distill import student_sensors_of
    from booster_gym_amd.utils.sensors import sensors_as_section

    cfg, _ = _base(n, H, Hs, sensors, fp16)
    cfg["env"]["student_frame_stack"] = Hs
    sc = student_sensors_of(cfg)
    if sc is not None:
        cfg["env"]["student_sensors"] = sensors_as_section(sc)
    return cfg


def _student_cfg(n, H, Hs, sensors, fp16):
    """The config the student re-enters under: student_cfg_overrides of the same config."""
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import student_cfg_overrides

    cfg, ov = _base(n, H, Hs, sensors, fp16)
    return load_cfg("T1", {**ov, **student_cfg_overrides(cfg)})


def _actions(n, k, amp=0.6):
    g = torch.Generator(device="cpu").manual_seed(2000 + k)
    return ((torch.rand(n, 12, generator=g) * 2 - 1) * amp).to(DEV)


_RUNS = {}


def _run(n, H, Hs, sensors, tag, fp16=False, student_env=False, again=False):
    """Reset-all and STEPS steps; per call t (0 = reset-all) the outputs as CPU tensors.  One run per key, shared by the tests.  student_env: the env
    of the student's re-entry (no student row of its own: its actor's row is the one under test)."""
    key = (n, H, Hs, tag, fp16, student_env)
    if key in _RUNS and not again:
        return _RUNS[key]
    from booster_gym_amd.envs import T1

    env = T1((_student_cfg if student_env else _teacher_cfg)(n, H, Hs, sensors, fp16))
    out = {k: [] for k in ("rows", "student", "rew", "done", "tout", "priv", "bias", "lat")}
    out["norms"] = tuple(float(env.cfg["normalization"][g]) for g in ("gravity", "ang_vel", "dof_pos", "dof_vel"))
    out["models"] = (env.sensor_model, env.student_sensor_model, int(env._cfg_c.sensor_model))
    has_draws = env.sensor_model or env.student_sensor_model

    def take(obs, rew, done, x):
        torch.cuda.synchronize()
        out["rows"].append(obs.cpu().clone()); out["rew"].append(rew.cpu().clone()); out["done"].append(done.cpu().clone())
        out["tout"].append(x["time_outs"].cpu().clone()); out["priv"].append(x["privileged_obs"].cpu().clone())
        if "student_obs" in x:
            out["student"].append(x["student_obs"].cpu().clone())
        if has_draws:
            out["bias"].append(env.sensor_bias.cpu().clone()); out["lat"].append(env.sensor_latency.cpu().clone())

    obs, x = env.reset()
    take(obs, torch.zeros(n), torch.ones(n, dtype=torch.bool), x)
    for k in range(STEPS):
        take(*env.step(_actions(n, k)))
    out["launches"] = env.sensor_launches
    if not again:
        _RUNS[key] = out
    return out


def _same(a, b, keys):
    return all(torch.equal(x, y) for k in keys for x, y in zip(a[k][(1 if k in ("rew", "done") else 0):], b[k][(1 if k in ("rew", "done") else 0):]))


def _ids(shapes):
    return [f"n{n}-H{H}-Hs{Hs}" + ("-fp16" if fp16 else "") for n, H, Hs, fp16 in shapes]


def test_the_shapes_reset_where_they_promise_and_the_fields_exist():
    b = _run(N_BIG, 1, 3, FULL, "full")
    assert b["models"] == (False, True, 2) and b["launches"] == 0  # bg_obs_sensor never runs: the model is inside bg_obs_assemble
    assert tuple(b["bias"][0].shape) == (N_BIG, 30) and tuple(b["lat"][0].shape) == (N_BIG,) and tuple(b["student"][0].shape) == (N_BIG, 47 * 3)
    age, on_time = torch.zeros(N_BIG, dtype=torch.long), 0
    for t in range(1, STEPS + 1):  # the sixth step of an episode times out, whenever the episode began
        due = age == 5
        assert b["done"][t][due].all(), t
        on_time += int(due.sum())
        age = torch.where(b["done"][t], torch.zeros_like(age), age + 1)
    assert on_time >= N_BIG and sum(int(d.sum()) for d in b["done"][1:]) >= 2 * N_BIG


# ------------------------------------------------------------------ 1. the rule
def _check_rule(n, H, Hs, sensors, tag, fp16=False):
    b = _run(n, H, Hs, sensors, tag, fp16)
    obs = [r[:, 47 * (H - 1) : 47 * H].numpy() for r in b["rows"]]  # the single observation the env stored: the teacher's newest frame, which stays clean
    dones = [d.numpy() for d in b["done"]]
    rows, mags = sensor_rows_ref(obs, dones, [x.numpy() for x in b["bias"]], [x.numpy() for x in b["lat"]], Hs)
    compared, worst = 0, 0.0
    for t in range(STEPS + 1):
        got, want, mag = b["student"][t].numpy().astype(np.float64), rows[t], mags[t]
        exact = mag == 0.0
        assert np.array_equal(got[exact], want[exact]), (t, "zero frames and non-sensor columns are exact")
        err, bound = np.abs(got - want)[~exact], 4.0 * 2.0 ** -24 * mag[~exact]
        worst = max(worst, float((err / bound).max())) if err.size else worst
        assert (err <= bound).all(), (t, float((err / bound).max()))
        compared += int(exact.sum()) + int((~exact).sum())
    print(f"rule n={n} H={H} Hs={Hs} {tag}{' fp16' if fp16 else ''}: worst error / bound {worst:.3f}")
    assert compared == (STEPS + 1) * n * 47 * Hs  # the share of elements left out is 0
    return b


@pytest.mark.parametrize("n,H,Hs,fp16", SHAPES, ids=_ids(SHAPES))
def test_the_rule(n, H, Hs, fp16):
    b = _check_rule(n, H, Hs, FULL, "full", fp16)
    assert b["models"] == (False, True, 2) and b["launches"] == 0
    if n == N_BIG and Hs == 3:  # frames older than the episode were zeroed, and the oldest frame is in use before the first time-out
        d6 = b["done"][6]
        assert d6.any() and not b["student"][6][d6][:, :94].any() and b["student"][6][d6][:, 94:].any() and b["student"][5][:, :47].any()
        moved = sum(int((s[:, -47:][:, list(SENSOR_COLUMNS)] != r[:, 47 * (H - 1) : 47 * H][:, list(SENSOR_COLUMNS)]).sum()) for s, r in zip(b["student"], b["rows"]))
        assert moved > 0.9 * 30 * n * (STEPS + 1)  # ... and the sensor columns do move


# ------------------------------------------------------------------ 2. the draws
def _ulp23(x):
    return 2.0 ** -23 * float(x)


def test_the_draws():
    n, seed = N_BIG, env_seed(SEED)
    b = _run(n, 1, 3, FULL, "full")
    norms = b["norms"]
    assert norms == (1.0, 1.0, 1.0, 0.1)
    names = ("gravity", "ang_vel", "dof_pos", "dof_vel")
    bound = np.zeros(30)
    for s in range(30):
        g = 0 if s < 3 else 1 if s < 6 else 2 if s < 18 else 3
        e, lo_hi = FULL_BIAS[names[g]], np.abs(FULL_BIAS[names[g]]["range"])
        if e["distribution"] == "gaussian":  # |mean| + 6 std: the largest operand a draw of 37 x 12 can reach
            bound[s] = norms[g] * (lo_hi[1] * 4.0 * NORMAL_DRAW + 4.0 * _ulp23(lo_hi[0] + 6.0 * lo_hi[1]))
        else:
            bound[s] = max(norms[g], 1.0) * 4.0 * _ulp23(lo_hi.sum())
    lat_bound = 4.0 * _ulp23(sum(LAT))
    resets, floors = 0, set()
    for t in range(STEPS + 1):
        done = b["done"][t].numpy().astype(bool)
        beta, lam = host_draws(seed, n, max(t - 1, 0), t == 0, FULL_BIAS, LAT, norms)  # call t >= 1 is step t - 1 of the counter; reset-all shares 0
        gb, gl = b["bias"][t].numpy(), b["lat"][t].numpy()
        assert (np.abs(gb[done].astype(np.float64) - beta[done]) <= bound).all(), t
        assert (np.abs(gl[done].astype(np.float64) - lam[done]) <= lat_bound).all(), t
        assert ((gl >= np.float32(LAT[0])) & (gl <= np.float32(LAT[1]))).all()
        floors |= set(np.floor(gl).astype(int).tolist())
        if t:  # an env that did not reset keeps both, bit for bit
            assert np.array_equal(gb[~done], b["bias"][t - 1].numpy()[~done]) and np.array_equal(gl[~done], b["lat"][t - 1].numpy()[~done]), t
            resets += int(done.sum())
            if done.any():  # a new episode, new values
                assert (gb[done] != b["bias"][t - 1].numpy()[done]).mean() > 0.99 and (gl[done] != b["lat"][t - 1].numpy()[done]).all()
    assert resets >= 2 * n and floors == {0, 1}  # both integer parts of the latency are in the run
    # the draws do not depend on H, Hs or the state's format: the streams are keyed by seed, env and step count alone
    for other in (_run(n, 2, 2, FULL, "full"), _run(n, 2, 3, FULL, "full")):
        assert _same(b, other, ("done", "bias", "lat"))


# ------------------------------------------------------------------ 3. the deployment claim
@pytest.mark.parametrize("n,H,Hs,fp16", SHAPES, ids=_ids(SHAPES))
def test_the_student_row_is_the_actor_row_of_the_env_the_student_re_enters(n, H, Hs, fp16):
    b, s = _run(n, H, Hs, FULL, "full", fp16), _run(n, H, Hs, FULL, "full", fp16, student_env=True)
    assert s["models"] == (True, False, 1) and s["launches"] == STEPS + 1 and not s["student"]  # bg_obs_sensor wrote every row there
    assert tuple(s["rows"][0].shape) == (n, 47 * Hs)
    for t in range(STEPS + 1):
        assert torch.equal(b["student"][t], s["rows"][t]), t
        assert torch.equal(b["bias"][t], s["bias"][t]) and torch.equal(b["lat"][t], s["lat"][t]), t
    assert _same(b, s, ("rew", "done", "tout"))


# ------------------------------------------------------------------ 4. the teacher is clean, 5. nothing configured
@pytest.mark.parametrize("n,H,Hs,fp16", SHAPES, ids=_ids(SHAPES))
def test_the_teacher_is_clean_and_an_empty_section_is_the_key_absent(n, H, Hs, fp16):
    a, b = _run(n, H, Hs, ABSENT, "absent", fp16), _run(n, H, Hs, FULL, "full", fp16)
    assert a["models"] == (False, False, 0) and a["launches"] == 0 and not a["bias"]
    assert _same(a, b, ("rows", "priv", "rew", "done", "tout"))  # teacher rows, privileged rows (scan included), the physics
    assert not _same(a, b, ("student",))
    for sa, sb in zip(a["student"], b["student"]):  # the 17 controller columns of the newest frame are untouched
        assert torch.equal(sa[:, -47:][:, REST], sb[:, -47:][:, REST])
    e = _run(n, H, Hs, {}, "empty", fp16)
    assert e["models"] == (False, True, 2) and e["launches"] == 0
    assert _same(a, e, ("student", "rows", "priv", "rew", "done", "tout"))
    assert all(not x.any() for x in e["bias"]) and all(not x.any() for x in e["lat"])
    null = _run(n, H, Hs, None, "null", fp16)
    assert null["models"] == (False, False, 0) and _same(a, null, ("student", "rows", "priv", "rew", "done", "tout"))


# ------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("tag,sensors", [
    ("whole2", {"bias": {"dof_pos": UNIF(-0.05, 0.05)}, "latency_steps": [2, 2]}),   # lam = 2 exactly: f = 0, the deepest plane, one group
    ("upto1", {"latency_steps": [0.0, 1.0]}),                                        # one more plane, no bias at all
    ("bias_only", {"bias": {"gravity": GAUSS(0.02, 0.0), "dof_vel": GAUSS(0.0, 1.0)}}),  # no interpolation on the path; a std of 0
])
def test_the_rule_at_the_edges_of_the_ranges(tag, sensors):
    b = _check_rule(N_BIG, 2, 3, sensors, tag)
    a = _run(N_BIG, 2, 3, ABSENT, "absent")
    assert _same(a, b, ("rows", "priv", "rew", "done", "tout"))
    if tag == "whole2":
        assert all((x == 2.0).all() for x in b["lat"])
    if tag == "upto1":
        assert all(not x.any() for x in b["bias"]) and any(x.any() for x in b["lat"])
    if tag == "bias_only":
        assert all((x[:, :3] == float(np.float32(0.02))).all() and not x[:, 3:18].any() and x[:, 18:].any() for x in b["bias"])
        assert all(not x.any() for x in b["lat"])


# ------------------------------------------------------------------ 7. step_to, 8. determinism
def test_step_to_writes_every_row_and_nothing_past_n():
    from booster_gym_amd.envs import T1

    n, H, Hs = N_BIG, 2, 3
    env, b = T1(_teacher_cfg(n, H, Hs, FULL, False)), _run(n, H, Hs, FULL, "full")
    env.reset()
    rew, done, tout = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV)
    for k in range(3):
        big = torch.full((n + 5, 47 * Hs), float("nan"), device=DEV)  # a different destination at every step, as the rows of a rollout buffer
        obs, priv = torch.full((n + 5, 47 * H + P), float("nan"), device=DEV), torch.full((n + 5, 14 + P), float("nan"), device=DEV)
        env.step_to(_actions(n, k), obs[:n], priv[:n], rew, done, tout, student_obs=big[:n])
        torch.cuda.synchronize()
        assert torch.isnan(big[n:]).all() and torch.isnan(obs[n:]).all() and torch.isnan(priv[n:]).all(), k
        assert torch.equal(big[:n].cpu(), b["student"][k + 1]) and torch.equal(obs[:n].cpu(), b["rows"][k + 1]) and torch.equal(priv[:n].cpu(), b["priv"][k + 1]), k
    with pytest.raises(RuntimeError, match="student"):
        env.step_to(_actions(n, 3), obs[:n], priv[:n], rew, done, tout)


@pytest.mark.parametrize("n,H,Hs", [(N_BIG, 1, 1), (N_BIG, 2, 3)])
def test_the_same_run_twice_gives_the_same_bits(n, H, Hs):
    b, again = _run(n, H, Hs, FULL, "full"), _run(n, H, Hs, FULL, "full", again=True)
    assert _same(b, again, ("rows", "student", "rew", "done", "tout", "priv", "bias", "lat"))
