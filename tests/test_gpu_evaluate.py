"""evaluate.py on the GPU: the record's kernel (bg_env_eval_begin / bg_env_eval_step) against a numpy restatement of its rule after every step, the
evaluation loop (reproducible, one launch per step, the actor's mean as the action), every checkpoint kind through the Evaluator, and a training
run that calls neither entry point.

Bounds.  The record's counters and positions are exact.  Its fp32 running sums (REW, POWER, SQ_*) against the float64 restatement:
2 (n + 12) 2^-24 sum|terms| with n the terms added so far -- an fp32 sum of n terms costs at most n - 1 roundings, a term carries at most 12 of its
own (the power term: 12 products and 11 adds; a squared difference: 3), and the factor 2 is slack for the bound's higher-order terms.  The actor's
mean against float64: 2e-5 max(1, |ref|max), tests/test_gpu_distill.py's bound for this launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 12
GRID_5x3 = {"terrain.measured_points_x": [-0.2, -0.1, 0.0, 0.1, 0.2], "terrain.measured_points_y": [-0.1, 0.0, 0.1]}
BASE = {"basic.sim_device": DEV, "basic.rl_device": DEV}


# ------------------------------------------------------------------ 1. the kernel
class Restatement:
    """The rule of bg_eval_step in numpy, sums in float64, from the values the env has stored (get_field) and the step's outputs.  Beside every sum
    it keeps sum|terms| and the number of terms, for the bound."""

    def __init__(self, n):
        from booster_gym_amd import _lib as L

        self.L, self.n = L, n
        self.rec = np.zeros((L.EVAL_PLANES, n))
        self.mag = np.zeros((L.EVAL_PLANES, n))
        self.terms = np.zeros((L.EVAL_PLANES, n))

    def _add(self, plane, who, values):
        self.rec[plane, who] += values
        self.mag[plane, who] += np.abs(values)
        self.terms[plane, who] += 1

    def begin(self, level, typ, xy):
        L = self.L
        self.rec[:] = 0
        self.rec[L.EVAL_LEVEL], self.rec[L.EVAL_TYPE] = level, typ
        self.rec[L.EVAL_X0] = self.rec[L.EVAL_X1] = xy[:, 0]
        self.rec[L.EVAL_Y0] = self.rec[L.EVAL_Y1] = xy[:, 1]

    def step(self, rew, done, tout, cmd, v, xy, torques, dof_vel, settle_steps):
        L, r = self.L, self.rec
        run = r[L.EVAL_STATE] == 0
        r[L.EVAL_LEN, run] += 1
        self._add(L.EVAL_REW, run, rew[run].astype(np.float64))
        end = run & done
        r[L.EVAL_STATE, end] = np.where(tout[end], 1, 2)
        live = run & ~done
        m = np.abs(cmd).max(axis=1)  # float32, compared as the kernel compares
        c = np.where(m <= np.float32(1e-6), 0, np.where(m <= np.float32(0.5), 1, 2))
        r[L.EVAL_CLASS, live] = c[live]
        r[L.EVAL_X1, live], r[L.EVAL_Y1, live] = xy[live, 0], xy[live, 1]
        self._add(L.EVAL_POWER, live, np.abs(torques.astype(np.float64) * dof_vel.astype(np.float64)).sum(axis=1)[live])
        track = live & (r[L.EVAL_LEN] > settle_steps)
        d2 = (cmd.astype(np.float64) - v.astype(np.float64)) ** 2
        for k in range(L.EVAL_CLASSES):
            who = track & (c == k)
            r[L.eval_track_plane(k, 0), who] += 1
            for a in range(3):
                self._add(L.eval_track_plane(k, 1 + a), who, d2[who, a])

    def compare(self, got, where):
        L = self.L
        exact = [L.EVAL_STATE, L.EVAL_LEN, L.EVAL_LEVEL, L.EVAL_TYPE, L.EVAL_CLASS, L.EVAL_X0, L.EVAL_Y0, L.EVAL_X1, L.EVAL_Y1] + \
                [L.eval_track_plane(k, 0) for k in range(L.EVAL_CLASSES)]
        sums = [p for p in range(L.EVAL_PLANES) if p not in exact]
        for p in exact:  # (the positions are float32 values in both: equal here is bit-equal)
            assert np.array_equal(got[p].astype(np.float64), self.rec[p]), (where, "plane", p)
        worst = 0.0
        for p in sums:
            bound = 2.0 * (self.terms[p] + 12.0) * 2.0 ** -24 * self.mag[p]
            err = np.abs(got[p].astype(np.float64) - self.rec[p])
            assert np.all(err <= bound), (where, "plane", p, float(err.max()), float(bound[err.argmax()]))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        return worst


CONFIGS = {
    "plane-fp32": {"terrain.type": "plane"},
    "curriculum-fp32": {"terrain.type": "trimesh", "terrain.curriculum": True, "terrain.num_levels": 3, "terrain.max_init_level": 2},
    "plane-fp16": {"terrain.type": "plane", "sim.state_dtype": "fp16"},
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_record_follows_the_rule_after_every_step(name):
    """N = 130 is no multiple of the wave or of the block; the episode is 25 steps, settle_steps 5, 30 steps with small fixed actions; at step 8
    robots 0 to 31 are laid on their side."""
    from booster_gym_amd import _lib as L
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    n, steps, settle, lay, fallen = 130, 30, 5, 8, 32
    over = CONFIGS[name]
    env = T1(load_cfg("T1", dict(BASE, **{"env.num_envs": n, "rewards.episode_length_s": 0.5}, **over)))
    curriculum = bool(over.get("terrain.curriculum"))
    if curriculum:
        env.terrain_levels = torch.arange(n) % 3
    env.reset()
    # the record in the middle of a poisoned allocation: nothing before plane 0 or past plane 22 may be written
    pad = 64
    store = torch.full((pad + L.EVAL_PLANES * n + pad,), float("nan"), device=DEV)
    record = store[pad : pad + L.EVAL_PLANES * n].view(L.EVAL_PLANES, n)
    assert env.eval_begin(record) is record
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    xy0 = host(env.get_field("root_states"))[:, :2]
    ref = Restatement(n)
    if curriculum:
        level, typ = host(env.terrain_levels), host(env.terrain_types)
        assert np.array_equal(level, np.arange(n) % 3)
        centres = env.terrain.tile_centres(level, typ)
        lo, hi = env.cfg["randomization"]["init_base_pos_xy"]["range"]
        off = xy0 - centres[:, :2]
        assert np.all(off >= lo - 1e-4) and np.all(off <= hi + 1e-4), (off.min(), off.max())  # every robot starts on its own tile
    else:
        level = typ = np.zeros(n)
    ref.begin(level, typ, xy0)
    ref.compare(host(record), "begin")
    assert bool(torch.isnan(store[:pad]).all()) and bool(torch.isnan(store[-pad:]).all())

    g = torch.Generator(device="cpu").manual_seed(77)
    actions = ((torch.rand(n, A, generator=g) * 2 - 1) * 0.1).to(DEV)
    frozen, first_time_out, worst = {}, None, 0.0
    for k in range(steps):
        if k == lay:
            root = host(env.root_states).copy()
            root[:fallen, 2] -= 0.4
            root[:fallen, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
            env.set_field("root_states", torch.from_numpy(root).float())
        _, rew, done, extras = env.step(actions)
        env.eval_step(record, settle)
        torch.cuda.synchronize()
        rew, done, tout = host(rew), host(done).astype(bool), host(extras["time_outs"]).astype(bool)
        if first_time_out is None and (done & tout).any():
            first_time_out = k + 1
        v = np.concatenate([host(env.get_field("filtered_lin_vel"))[:, :2], host(env.get_field("filtered_ang_vel"))[:, 2:3]], axis=1)
        ref.step(rew, done, tout, host(env.get_field("commands")), v, host(env.get_field("root_states"))[:, :2], host(env.get_field("torques")),
                 host(env.get_field("dof_vel")), settle)
        got = host(record)
        worst = max(worst, ref.compare(got, f"step {k + 1}"))
        for e in np.nonzero(got[L.EVAL_STATE] != 0)[0]:  # a finished record is frozen: not a bit of it moves after its last step
            if e not in frozen:
                frozen[e] = got[:, e].copy()
            assert np.array_equal(frozen[e].view(np.uint32), got[:, e].view(np.uint32)), (k + 1, e)
    print(f"{name}: worst error / bound of the sums {worst:.3f}; first time-out at step {first_time_out}")
    assert bool(torch.isnan(store[:pad]).all()) and bool(torch.isnan(store[-pad:]).all())
    # not vacuous: the laid robots fell at their ninth step, somebody ran to the env's own time-out, everybody finished, something was tracked
    assert np.all(got[L.EVAL_STATE, :fallen] == 2) and np.all(got[L.EVAL_LEN, :fallen] == lay + 1)
    assert first_time_out is not None
    timed_out = got[L.EVAL_STATE] == 1
    assert timed_out.any() and np.all(got[L.EVAL_LEN, timed_out] == first_time_out)
    assert not (got[L.EVAL_STATE] == 0).any()
    cnt = sum(got[L.eval_track_plane(c, 0)] for c in range(L.EVAL_CLASSES))
    assert np.all(cnt[timed_out] == first_time_out - 1 - settle) and np.all(cnt[:fallen] == lay - settle)
    assert got[L.EVAL_POWER].max() > 0 and len(np.unique(got[L.EVAL_CLASS])) >= 2


def test_stale_time_outs_is_refused_by_eval_begin():
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    env = T1(load_cfg("T1", dict(BASE, **{"env.num_envs": 64, "terrain.type": "plane", "parallel.stale_time_outs": True})))
    env.reset()
    with pytest.raises(ValueError, match="parallel.stale_time_outs"):
        env.eval_begin()
    env2 = T1(load_cfg("T1", dict(BASE, **{"env.num_envs": 64, "terrain.type": "plane"})))
    with pytest.raises(ValueError, match="record"):
        env2.eval_begin(torch.zeros(23, 65, device=DEV))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. - 3. the loop and the checkpoint kinds
N = 64
EPISODE = {"env.num_envs": N, "rewards.episode_length_s": 0.4, "runner.horizon_length": 4}  # 20 steps: K = 22


def _overrides(**over):
    return dict(BASE, **EPISODE, **over)


def _save_runner(path, seed=3, normaliser=False, **over):
    """The checkpoint of a seeded, untrained Runner; with a normaliser, one whose statistics are not the identity."""
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    r = Runner(test=True, cfg=load_cfg("T1", _overrides(**{"basic.seed": seed}, **over)))
    if normaliser:
        rng = np.random.default_rng(11)
        c = r.obs_norm.cols
        r.obs_norm.load_state_dict({"mean": torch.from_numpy(rng.normal(size=c) * 0.3), "var": torch.from_numpy(rng.uniform(0.5, 2.0, c)), "count": 100.0,
                                    "eps": r.obs_norm.eps})
    torch.save(r.checkpoint_dict(), path)
    del r
    torch.cuda.synchronize()
    return path


def _spy_actions(monkeypatch, ev):
    """Keeps (the observation the env holds, the actions it is given) of every env step of ev."""
    seen, step = [], ev.env.step

    def wrap(actions):
        seen.append((ev.env.obs_buf.clone(), actions.clone()))
        return step(actions)

    monkeypatch.setattr(ev.env, "step", wrap)
    return seen


def _check_actions(ev, seen):
    from test_gpu_frame_stack import _actor_f64

    worst = 0.0
    for obs, act in seen:
        x = obs.double()
        if ev.obs_norm is not None:
            k = obs.shape[1]
            x = (x - ev.obs_norm.mean_dev[:k].double()) * ev.obs_norm.inv_std_dev[:k].double()
        ref = _actor_f64(ev.model, x)
        err, scale = (act.double() - ref).abs().max().item(), max(1.0, ref.abs().max().item())
        worst = max(worst, err / scale)
        assert err <= 2e-5 * scale, (err, scale)
    return worst


def _spy_lib(monkeypatch, names):
    from booster_gym_amd import _lib

    lib, counts = _lib.load(), {name: 0 for name in names}
    for name in names:
        def wrap(*a, _fn=getattr(lib, name), _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


def test_loop_is_reproducible_launches_once_per_step_and_acts_with_the_mean(monkeypatch, tmp_path):
    from booster_gym_amd.utils.evaluate import Evaluator

    path = _save_runner(str(tmp_path / "model.pth"), **{"terrain.type": "plane"})
    counts = _spy_lib(monkeypatch, ("bg_env_eval_begin", "bg_env_eval_step", "bg_env_step", "bg_actor_sample", "bg_actor_pack"))
    runs = []
    for seed in (5, 5, 6):
        ev = Evaluator(checkpoint=path, overrides=_overrides(**{"terrain.type": "plane", "basic.seed": seed}))
        seen = _spy_actions(monkeypatch, ev) if not runs else None
        before = dict(counts)
        rep = ev.run()
        K = ev.max_episode_length + 2
        assert K == 22 and rep["steps"] == K and ev.settle_steps == 50 and ev.loop_s > 0
        got = {k: counts[k] - before[k] for k in counts}
        assert got == {"bg_env_eval_begin": 1, "bg_env_eval_step": K, "bg_env_step": K, "bg_actor_sample": K, "bg_actor_pack": 1}, got
        if seen is not None:
            assert len(seen) == K
            print("actor mean: worst error / (2e-5 scale) =", _check_actions(ev, seen) / 2e-5)
        runs.append((ev.record.clone(), rep))
        del ev
    (r0, p0), (r1, p1), (r2, p2) = runs
    assert torch.equal(r0.view(torch.int32), r1.view(torch.int32)) and p0 == p1
    assert not torch.equal(r0, r2) and p2["seed"] == 6
    a = p0["all"]
    assert a["unfinished"] == 0 and a["robots"] == N and a["fell"] + a["timed_out"] == N
    assert (p0["checkpoint"], p0["seed"], p0["num_envs"], p0["settle_s"], p0["overrides"], p0["nonfinite_resets"]) == (path, 5, N, 1.0, {}, 0.0)
    assert len(p0["by_level"]) == 1 and len(p0["by_type"]) == 1 and p0["by_level"][0] == a


@pytest.fixture(scope="module")
def teacher_ck(tmp_path_factory):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.terrain import height_scan_points

    torch.manual_seed(5)
    P = 15
    m = ActorCritic(A, 47 + P, 14 + P)
    cfg = load_cfg("T1", dict({"terrain.measure_heights": True}, **GRID_5x3))
    pts = torch.tensor(height_scan_points(cfg["terrain"])[1], dtype=torch.float).reshape(P, 2)
    path = str(tmp_path_factory.mktemp("teacher") / "teacher.pth")
    torch.save({"model": m.state_dict(), "height_points": pts}, path)
    return path


def test_frame_stack_with_a_normaliser_evaluates(monkeypatch, tmp_path):
    from booster_gym_amd.utils.evaluate import Evaluator

    kind = {"terrain.type": "plane", "env.frame_stack": 2, "env.num_observations": 94, "algorithm.empirical_normalization": True}
    path = _save_runner(str(tmp_path / "model.pth"), normaliser=True, **kind)
    counts = _spy_lib(monkeypatch, ("bg_obs_normalize", "bg_actor_sample_mlp", "bg_env_eval_step"))
    ev = Evaluator(checkpoint=path, overrides=_overrides(**kind))
    assert ev.obs_norm is not None and ev.env.frame_stack == 2 and float(np.abs(ev.obs_norm.mean).max()) > 0
    seen = _spy_actions(monkeypatch, ev)
    rep = ev.run()
    assert counts == {"bg_obs_normalize": 22, "bg_actor_sample_mlp": 22, "bg_env_eval_step": 22}, counts
    print("actor mean on normalised rows: worst error / (2e-5 scale) =", _check_actions(ev, seen) / 2e-5)
    assert rep["all"]["unfinished"] == 0 and rep["all"]["robots"] == N
    # the same checkpoint under a config without the key: Runner._load's refusal, unchanged
    with pytest.raises(ValueError, match="empirical_normalization"):
        Evaluator(checkpoint=path, overrides=_overrides(**dict(kind, **{"algorithm.empirical_normalization": False})))


def test_perceptive_actor_evaluates_per_level(monkeypatch, tmp_path):
    from booster_gym_amd.utils.evaluate import Evaluator

    P = 15
    kind = dict({"terrain.type": "trimesh", "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 + P,
                 "env.num_privileged_obs": 14 + P, "terrain.curriculum": True, "terrain.num_levels": 4, "terrain.max_init_level": 1}, **GRID_5x3)
    path = _save_runner(str(tmp_path / "model.pth"), **kind)
    counts = _spy_lib(monkeypatch, ("bg_actor_sample_mlp_scan",))
    ev = Evaluator(checkpoint=path, overrides=_overrides(**kind))
    assert ev.env.num_scan_obs == P and "env.terrain_levels" in ev.applied
    seen = _spy_actions(monkeypatch, ev)
    rep = ev.run()
    assert counts == {"bg_actor_sample_mlp_scan": 22}
    _check_actions(ev, seen)
    assert rep["all"]["unfinished"] == 0 and [g["robots"] for g in rep["by_level"]] == [16, 16, 16, 16]  # spread: every level the same number
    assert len(rep["by_type"]) == 8 and sum(g["robots"] for g in rep["by_type"]) == N
    for key in ("fell", "timed_out"):
        assert sum(g[key] for g in rep["by_level"]) == rep["all"][key] == sum(g[key] for g in rep["by_type"])
    # evaluation.spread_terrain_levels: false keeps the checkpoint's levels (the initial draw in [0, max_init_level] here)
    ev2 = Evaluator(checkpoint=path, overrides=_overrides(**dict(kind, **{"evaluation.spread_terrain_levels": False})))
    assert ev2.applied == {} and int(ev2.env.terrain_levels.max()) <= 1
    torch.cuda.synchronize()


def test_student_checkpoint_evaluates_from_its_path_under_the_teachers_config(teacher_ck, tmp_path):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import Distiller, student_cfg_overrides
    from booster_gym_amd.utils.evaluate import Evaluator

    P, Hs = 15, 3
    teacher = dict({"terrain.type": "trimesh", "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 + P,
                    "env.num_privileged_obs": 14 + P, "distillation.student_frame_stack": Hs, "distillation.num_epochs": 1}, **GRID_5x3)
    cfg = load_cfg("T1", _overrides(**teacher, **{"distillation.teacher_checkpoint": teacher_ck}))
    want = student_cfg_overrides(cfg)
    d = Distiller(cfg=cfg)

    class _Rec:
        def record_episode_statistics(self, env, names, it, stats=None):
            env.episode_stats(reset=True)

        def record_statistics(self, summary, it):
            pass

        def save(self, d, it):
            pass

    d.begin(recorder=_Rec())
    d.train_iteration(0)
    path = str(tmp_path / "student.pth")
    torch.save(d.checkpoint_dict(), path)
    sd = {k: v.clone() for k, v in d.student.state_dict().items()}
    del d
    ev = Evaluator(checkpoint=path, overrides=_overrides(**teacher))  # the teacher's config; nothing of the student's but the path
    assert ev.applied == want == {"terrain.actor_heights": False, "env.frame_stack": Hs, "env.num_observations": 47 * Hs}
    assert ev.env.frame_stack == Hs and ev.env.num_scan_obs == 0 and ev.model.actor[0].in_features == 47 * Hs
    for k, v in ev.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    rep = ev.run()
    assert rep["overrides"] == want and rep["all"]["unfinished"] == 0 and rep["all"]["robots"] == N


def test_a_checkpoint_of_other_widths_is_still_refused_and_an_actor_state_dict_is_accepted(tmp_path):
    from booster_gym_amd.utils.evaluate import Evaluator

    path = _save_runner(str(tmp_path / "model.pth"), **{"terrain.type": "plane"})
    with pytest.raises(ValueError, match="hidden widths"):
        Evaluator(checkpoint=path, overrides=_overrides(**{"terrain.type": "plane", "algorithm.actor_hidden": [128, 128]}))
    with pytest.raises(ValueError, match="one of the two"):
        Evaluator()
    actor = {k[len("actor."):]: v.cpu().numpy() for k, v in torch.load(path, weights_only=True)["model"].items() if k.startswith("actor.")}
    by_path = Evaluator(checkpoint=path, overrides=_overrides(**{"terrain.type": "plane", "basic.seed": 9}))
    rec = by_path.run() and by_path.record.clone()
    del by_path
    by_dict = Evaluator(actor=actor, overrides=_overrides(**{"terrain.type": "plane", "basic.seed": 9}))
    rep = by_dict.run()
    assert torch.equal(rec, by_dict.record) and rep["checkpoint"] is None  # the same actor either way: the same record


# ------------------------------------------------------------------ 4. training is untouched
def test_training_calls_neither_entry_point(monkeypatch):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    counts = _spy_lib(monkeypatch, ("bg_env_eval_begin", "bg_env_eval_step", "bg_env_step_to"))
    r = Runner(cfg=load_cfg("T1", dict(BASE, **{"env.num_envs": 128, "terrain.type": "plane", "runner.mini_epochs": 2})))
    obs, infos = r.env.reset()
    r.buffer["obses"][0].copy_(obs)
    r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
    for _ in range(2):
        stats = r.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all()
    assert counts == {"bg_env_eval_begin": 0, "bg_env_eval_step": 0, "bg_env_step_to": 2 * r.cfg["runner"]["horizon_length"]}, counts
