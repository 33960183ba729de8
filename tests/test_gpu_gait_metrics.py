"""The gait record on the GPU: the kernel (bg_env_gait_begin / bg_env_gait_step) against the numpy restatement of its rule (tests/gait_ref.py) after
every step, identities of the record under a policy that walks, the evaluation loop with the key on and off, and a training run that calls neither
entry point.

Bounds.  Counters, flags, carries and PEAK are exact.  The fp32 running sums (D1, D2, TAU2, TILT, WOBBLE, IMP, SLIP) against the float64
restatement: 2 (n + 12) 2^-24 sum|terms| with n the terms added so far, tests/test_gpu_evaluate.py's bound and argument (an fp32 sum of n terms
costs at most n - 1 roundings, a term at most 12 of its own: 12 products and 11 adds; the factor 2 is slack for the higher-order terms).  SWMAX and
CLR are exact on a plane (the clearance is p.z itself; CLR against the float32 sum of the same terms in the same order).  On a height field the
kernel's fp32 bilinear height stands against float64: 1e-4 m per term on top, the bound tests/test_gpu_height_scan.py holds the scan to."""
import numpy as np
import pytest
import torch

from gait_ref import GaitRestatement
# the first record's tests own the configurations, the checkpoint helper and the library spy: these tests run the second record under the same ones, so
# an edit of tests/test_gpu_evaluate.py's BASE, CONFIGS, EPISODE (through _overrides), _save_runner or _spy_lib changes them too
from test_gpu_evaluate import BASE, CONFIGS, DEV, N, _overrides, _save_runner, _spy_lib

pytestmark = pytest.mark.gpu
A = 12


# ------------------------------------------------------------------ 5. the kernel
def _ground(env, xy):
    """The terrain height under world xy [n, 2] in float64 (utils/terrain.py's bilinear rule, indices clamped); 0 on a plane."""
    t = env.terrain
    if t.height_field_raw is None:
        return np.zeros(len(xy))
    hf = t.height_field_raw.astype(np.float64)
    px, py = t.border_pixels + xy[:, 0] / t.horizontal_scale, t.border_pixels + xy[:, 1] / t.horizontal_scale
    x1 = np.clip(np.floor(px).astype(np.int64), 0, hf.shape[0] - 2)
    y1 = np.clip(np.floor(py).astype(np.int64), 0, hf.shape[1] - 2)
    fx, fy = px - x1, py - y1
    return ((1 - fx) * (1 - fy) * hf[x1, y1] + fx * (1 - fy) * hf[x1 + 1, y1] + (1 - fx) * fy * hf[x1, y1 + 1] + fx * fy * hf[x1 + 1, y1 + 1]) * t.vertical_scale


def _script(t, i, xy0):
    """The scripted feet of robots 64 + i at step t (len = t): (contact [m, 2], forces [m, 6], feet_pos [m, 6]).  Robots with i % 3 != 1 stand 5 steps
    and swing 3 (double support twice a period), the others stand 3 and swing 5 (flight twice a period), the right foot half a period ahead, the
    phase shifted by i; a stance foot creeps 2 to 10 mm a step and carries 300 to 420 N, a swing foot is 3 to 6 cm up; from step 12 on the feet of
    robots with i % 4 == 0 stand 0.8 m further along x: for a foot in stance at steps 11 and 12 that is the teleport wrap, not slip."""
    m = len(i)
    stance = np.where(i % 3 != 1, 5, 3)
    contact, forces, pos = np.zeros((m, 2), np.float32), np.zeros((m, 6), np.float32), np.zeros((m, 6), np.float32)
    for f in range(2):
        c = ((t + 4 * f + i) % 8) < stance
        contact[:, f] = c
        forces[:, 3 * f + 0], forces[:, 3 * f + 1] = 5.0 * c, -3.0 * c
        forces[:, 3 * f + 2] = np.where(c, 300.0 + 10.0 * ((7 * t + 3 * i + f) % 13), 0.0)
        pos[:, 3 * f + 0] = xy0[:, 2 * f] + 0.002 * (1 + i % 5) * t + np.where((i % 4 == 0) & (t >= 12), 0.8, 0.0)
        pos[:, 3 * f + 1] = xy0[:, 2 * f + 1] - 0.001 * t
        pos[:, 3 * f + 2] = np.where(c, 0.0, 0.03 + 0.01 * ((t + i) % 4))
    return contact, forces, pos


@pytest.mark.parametrize("name", list(CONFIGS))
def test_gait_record_follows_the_rule_after_every_step(name):
    """N = 130 is no multiple of the wave or of the block; the episode is 25 steps, settle_steps 5, 30 steps, actions drawn afresh every step; at
    step 8 robots 0 to 31 are laid on their side; robots 32 to 63 keep what the physics stored; the feet of robots 64 to 129 are scripted (and every
    sixth of them commanded to stand still, the others to walk) between the env step and the record's launch, which is a function of the stored fields."""
    from booster_gym_amd import _lib as L
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    n, steps, settle, lay, fallen, first = 130, 30, 5, 8, 32, 64
    over = CONFIGS[name]
    env = T1(load_cfg("T1", dict(BASE, **{"env.num_envs": n, "rewards.episode_length_s": 0.5}, **over)))
    plane = over["terrain.type"] == "plane"
    if over.get("terrain.curriculum"):
        env.terrain_levels = torch.arange(n) % 3
    env.reset()
    pad = 64  # the record in the middle of a poisoned allocation: nothing before plane 0 or past plane 59 may be written
    store = torch.full((pad + L.GAIT_PLANES * n + pad,), float("nan"), device=DEV)
    record = store[pad : pad + L.GAIT_PLANES * n].view(L.GAIT_PLANES, n)
    assert env.gait_begin(record) is record
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    assert not host(record).any()
    poison_intact = lambda: bool(torch.isnan(store[:pad]).all()) and bool(torch.isnan(store[-pad:]).all())
    assert poison_intact()
    ref = GaitRestatement(n)
    ref.begin()
    i = np.arange(n - first)
    xy0 = host(env.get_field("feet_pos"))[first:][:, [0, 1, 3, 4]].astype(np.float64)
    still = (i % 6 == 5)
    gen = torch.Generator(device="cpu").manual_seed(77)
    frozen, worst, prev, changed = {}, 0.0, host(record).copy(), np.zeros(L.GAIT_PLANES, bool)
    for k in range(steps):
        if k == lay:
            root = host(env.root_states).copy()
            root[:fallen, 2] -= 0.4
            root[:fallen, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
            env.set_field("root_states", torch.from_numpy(root).float())
        actions = ((torch.rand(n, A, generator=gen) * 2 - 1) * 0.3).to(DEV)
        _, _, done, _ = env.step(actions)
        contact, forces, pos = host(env.get_field("feet_contact")), host(env.get_field("feet_contact_forces")), host(env.get_field("feet_pos"))
        contact[first:], forces[first:], pos[first:] = _script(k + 1, i, xy0)
        cmd = host(env.get_field("commands"))
        cmd[first:] = np.where(still[:, None], 0.0, np.float32([0.4, 0.0, -0.2]))
        for fname, v in (("feet_contact", contact), ("feet_contact_forces", forces), ("feet_pos", pos), ("commands", cmd)):
            env.set_field(fname, torch.from_numpy(v))
        env.gait_step(record, settle)
        torch.cuda.synchronize()
        fld = {f: host(env.get_field(f)) for f in ("actions", "torques", "projected_gravity", "base_ang_vel", "commands", "feet_contact",
                                                   "feet_contact_forces", "feet_pos")}
        p = fld["feet_pos"].astype(np.float64)
        clr = np.stack([p[:, 2] - _ground(env, p[:, 0:2]), p[:, 5] - _ground(env, p[:, 3:5])], axis=1)
        ref.step(host(done).astype(bool), fld["actions"], fld["torques"], fld["projected_gravity"], fld["base_ang_vel"], fld["commands"],
                 fld["feet_contact"], fld["feet_contact_forces"], fld["feet_pos"], clr, settle)
        got = host(record)
        worst = max(worst, ref.compare(got, f"step {k + 1}", height_slack=0.0 if plane else 1e-4))
        changed |= (got[:, first:].view(np.uint32) != prev[:, first:].view(np.uint32)).any(axis=1)
        prev = got.copy()
        for e in np.nonzero(got[L.GAIT_STATE] != 0)[0]:  # a finished record is frozen: not a bit of it moves after its last step
            if e not in frozen:
                frozen[e] = got[:, e].copy()
            assert np.array_equal(frozen[e].view(np.uint32), got[:, e].view(np.uint32)), (k + 1, e)
    print(f"{name}: worst error / bound of the bounded planes {worst:.3f}")
    assert poison_intact()
    # not vacuous.  Every plane of some scripted robot changed; the laid robots ended at their ninth step (one that the random actions threw
    # earlier, earlier); everybody finished
    assert changed.all(), np.nonzero(~changed)[0]
    assert np.all(got[L.GAIT_STATE, :fallen] == 1) and np.all(got[L.GAIT_LEN, :fallen] <= lay + 1) and not (got[L.GAIT_STATE] == 0).any()
    assert (got[L.GAIT_LEN, :fallen] == lay + 1).sum() >= fallen // 2 and got[L.GAIT_LEN].max() >= 25
    s = got[:, first:]
    FP = L.gait_foot_plane
    for f in range(2):  # touchdowns, closed swings, impacts and slip on both feet
        for q in (L.GAIT_STANCE, L.GAIT_TD, L.GAIT_IMP, L.GAIT_PEAK, L.GAIT_SLIP, L.GAIT_CLR, L.GAIT_SWT, L.GAIT_SWC):
            assert s[FP(q, f)].max() > 0, (q, f)
        assert ref.slip_skipped[f, first:].sum() > 0  # a stance displacement above half a metre met the guard ...
        assert 0 < s[FP(L.GAIT_SLIP, f)].max() < 0.5  # ... and those below it were added
    assert s[L.GAIT_DS].max() > 0 and s[L.GAIT_FL].max() > 0
    # a swing that began before settle_steps and landed after it counts whole
    assert any(e >= first and t > settle and t - swn <= settle for t, e, _, swn in ref.touchdowns)
    assert np.all(s[L.GAIT_MOV][still] == 0) and np.all(s[L.GAIT_MOV][~still] > 0) and np.all(s[L.GAIT_TAU2] > 0)
    # the physics' own fields (robots 32 to 63) gave samples too
    assert got[L.GAIT_TAU2, fallen:first].min() > 0 and got[FP(L.GAIT_PEAK, 0), fallen:first].max() > 0


def test_record_arguments_are_checked():
    from booster_gym_amd import _lib as L
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    env = T1(load_cfg("T1", dict(BASE, **{"env.num_envs": 64, "terrain.type": "plane"})))
    env.reset()
    with pytest.raises(ValueError, match="gait_begin needs"):
        env.gait_begin(torch.zeros(L.GAIT_PLANES, 65, device=DEV))
    with pytest.raises(ValueError, match="gait_begin needs"):
        env.gait_begin(torch.zeros(L.GAIT_PLANES, 64, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="gait_step needs"):
        env.gait_step(torch.zeros(L.EVAL_PLANES, 64, device=DEV), 5)
    rec = env.gait_begin()
    assert tuple(rec.shape) == (L.GAIT_PLANES, 64) and not bool(rec.any())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. identities under a policy that walks
def test_identities_of_the_record_under_the_packaged_actor():
    """tests/golden/t1_actor.npz on a plane, 256 robots, 150 steps (100 of them after settling).  Nothing numeric about the gait itself is asserted:
    nobody has measured one."""
    import os

    from booster_gym_amd import _lib as L
    from booster_gym_amd.utils.evaluate import Evaluator, format_report

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with np.load(os.path.join(root, "tests", "golden", "t1_actor.npz")) as W:
        ev = Evaluator(actor={k: W[k] for k in W.files}, overrides=dict(BASE, **{"env.num_envs": 256, "terrain.type": "plane", "evaluation.gait": True}))
    rep = ev.run(150)
    print(format_report(rep))
    g = ev.gait_record.cpu().numpy().astype(np.float64)
    FP = L.gait_foot_plane
    assert np.array_equal(g[FP(L.GAIT_STANCE, 0)] + g[FP(L.GAIT_STANCE, 1)], g[L.GAIT_MOV] + g[L.GAIT_DS] - g[L.GAIT_FL])
    for f in range(2):
        assert np.all(g[FP(L.GAIT_TD, f)] <= g[L.GAIT_MOV]) and g[FP(L.GAIT_TD, f)].sum() > 0
    assert np.array_equal(g[L.GAIT_LEN], ev.record.cpu().numpy()[L.EVAL_LEN])  # the two records count the same steps
    a = rep["all"]["gait"]
    assert all(0 < d < 1 for d in a["duty_factor"]), a["duty_factor"]
    assert np.isfinite(a["cost_of_transport"]) and a["cost_of_transport"] > 0
    assert 0 <= a["stance_asymmetry"] <= 1
    assert rep["by_level"][0]["gait"] == a and rep["by_type"][0]["gait"] == a
    m = ev.mass()
    assert m.shape == (256,) and m.dtype == np.float64 and 20 < m.min() <= m.max() < 60


# ------------------------------------------------------------------ 7. the loop
def test_loop_with_the_key_on_and_off(monkeypatch, tmp_path):
    from booster_gym_amd import _lib as L
    from booster_gym_amd.utils.evaluate import Evaluator, main

    # (the episode of _overrides is 20 steps and settle_steps 50: MOV and every gait counter stay 0 in these runs, so the bit-equality below rests on
    # D1, D2, TAU2, TILT, WOBBLE, PEAK and the carries; the counters are the rule test's and the identity test's business)
    kind = {"terrain.type": "plane"}
    path = _save_runner(str(tmp_path / "model.pth"), **kind)
    counts = _spy_lib(monkeypatch, ("bg_env_gait_begin", "bg_env_gait_step", "bg_env_eval_begin", "bg_env_eval_step", "bg_env_step"))
    runs = []
    for gait in (True, True, False):
        ev = Evaluator(checkpoint=path, overrides=_overrides(**kind, **({"evaluation.gait": True} if gait else {}), **{"basic.seed": 5}))
        before = dict(counts)
        rep = ev.run()
        K = ev.max_episode_length + 2
        got = {k: counts[k] - before[k] for k in counts}
        assert got == {"bg_env_gait_begin": int(gait), "bg_env_gait_step": K * int(gait), "bg_env_eval_begin": 1, "bg_env_eval_step": K, "bg_env_step": K}, got
        runs.append((ev.record.clone(), ev.gait_record.clone() if gait else None, rep))
        if gait and not runs[:-1]:
            out = str(tmp_path / "records.npz")
            ev.save_records(out)
            with np.load(out) as z:
                assert sorted(z.files) == ["dt", "gait_planes", "gait_record", "mass", "record", "record_planes", "seed", "settle_steps"]
                assert np.array_equal(z["record"].view(np.uint32), ev.record.cpu().numpy().view(np.uint32))
                assert np.array_equal(z["gait_record"].view(np.uint32), ev.gait_record.cpu().numpy().view(np.uint32))
                assert list(z["gait_planes"]) == L.gait_plane_names() and list(z["record_planes"]) == L.eval_plane_names()
                assert (float(z["dt"]), int(z["settle_steps"]), int(z["seed"])) == (ev.env.dt, 50, 5) and np.array_equal(z["mass"], ev.mass())
        del ev
    (r0, g0, p0), (r1, g1, p1), (r2, g2, p2) = runs
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)) and p0 == p1  # equal seeds: bit-equal gait records
    assert torch.equal(r0.view(torch.int32), r2.view(torch.int32))              # the first record does not know about the second
    assert g2 is None and "gait" in p0["all"] and "gait" not in p2["all"]
    strip = lambda grp: {k: v for k, v in grp.items() if k != "gait"}
    assert set(p2) == set(p0) and set(p2["all"]) == set(p0["all"]) - {"gait"}  # with the key off the report's keys are those of before
    assert strip(p0["all"]) == p2["all"] and [strip(x) for x in p0["by_level"]] == p2["by_level"]
    assert float(g0[L.GAIT_LEN].min()) >= 1 and float(g0[L.GAIT_TAU2].max()) > 0

    # the command line: --gait and --record_out, against an Evaluator of the same seed
    out, npz = str(tmp_path / "evaluation.json"), str(tmp_path / "cli.npz")
    rep = main(["--task", "T1", "--checkpoint", path, "--num_envs", "64", "--seed", "5", "--steps", "12", "--gait", "--out", out, "--record_out", npz])
    ev = Evaluator(checkpoint=path, overrides={"env.num_envs": 64, "basic.seed": 5, "evaluation.gait": True})
    ev.run(12)
    with np.load(npz) as z:
        assert np.array_equal(z["record"].view(np.uint32), ev.record.cpu().numpy().view(np.uint32))
        assert np.array_equal(z["gait_record"].view(np.uint32), ev.gait_record.cpu().numpy().view(np.uint32))
    assert "gait" in rep["all"]
    rep = main(["--task", "T1", "--checkpoint", path, "--num_envs", "64", "--seed", "5", "--steps", "12", "--out", out, "--record_out", npz])
    with np.load(npz) as z:  # without --gait: the first record alone, equal to the one beside the gait record
        assert "gait_record" not in z.files and "gait_planes" not in z.files
        assert np.array_equal(z["record"].view(np.uint32), ev.record.cpu().numpy().view(np.uint32))
    assert "gait" not in rep["all"]


# ------------------------------------------------------------------ 8. training is untouched
def test_training_calls_neither_entry_point(monkeypatch):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    counts = _spy_lib(monkeypatch, ("bg_env_gait_begin", "bg_env_gait_step", "bg_env_step_to"))
    r = Runner(cfg=load_cfg("T1", dict(BASE, **{"env.num_envs": 128, "terrain.type": "plane", "runner.mini_epochs": 2})))
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs)
    r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    for _ in range(2):
        stats = r.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all()
    assert counts == {"bg_env_gait_begin": 0, "bg_env_gait_step": 0, "bg_env_step_to": 2 * r.cfg["runner"]["horizon_length"]}, counts
