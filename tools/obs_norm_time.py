"""Timing of the empirical observation normalisation (README "Observation normalisation"):

  python tools/obs_norm_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      (1) bg_obs_moments alone (HIP events around 50 back-to-back launch pairs, best of 5) on the 24 x num_envs rows of the default shape (47 + 14
          columns) and of env.frame_stack 5 with the height scan (235 + 201 columns): us per call, bytes read, fraction of an 8 TB/s HBM roof;
      (2) bg_obs_normalize alone: one rollout step ([num_envs][47] into the sampling scratch) and one update call (the padded critic and actor
          inputs of 25 / 24 steps: three launches), us per call;
      (3) the rollout pair "sample + env step" with the key true against false (HIP events around 48 steps, best of 5, alternating);
      (4) the training loop (no instrumentation), key true against false, two runners on one GPU, alternating runs of K iterations after W
          warm-up iterations each: ms per iteration, iterations per second, ratio.  The forward passes during the rollout stay on with the key."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

DEV = "cuda:0"
KEYS = (False, True)


def _cfg(N, on):
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "trimesh", "algorithm.empirical_normalization": on})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    return cfg


def _best(fn, reps, rounds=5):
    b = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(reps):
            fn(k)
        e1.record(); torch.cuda.synchronize()
        b = min(b, e0.elapsed_time(e1) / reps * 1e3)
    return b


def kernels(N=4096, T=24):
    from booster_gym_amd.utils.obs_norm import ObsNormalizer

    for no, npv, what in ((47, 14, "default shape"), (235, 201, "frame_stack 5 + height scan")):
        norm = ObsNormalizer(no + npv, 1.0e-2, DEV)
        obs, priv = torch.randn(T + 1, N, no, device=DEV), torch.randn(T + 1, N, npv, device=DEV)
        us = _best(lambda k: norm.moments_into(obs[:T], priv[:T]), 50)
        nbytes = 4 * T * N * (no + npv)
        print(f"bg_obs_moments (+ finish + row-count fill), {what}, {T * N} rows x {no + npv} columns: {us:.2f} us per call, {nbytes / 1e6:.1f} MB read, "
              f"{nbytes / us / 1e6:.3f} TB/s = {nbytes / us / 1e6 / 8 * 100:.1f} % of 8 TB/s", flush=True)
        from booster_gym_amd.utils.runner import pad_input

        pa, pc = pad_input(no), pad_input(no + npv)
        scratch, ci, ai = torch.zeros(N, no, device=DEV), torch.zeros(T + 1, N, pc, device=DEV), torch.zeros(T, N, pa, device=DEV)
        us_step = _best(lambda k: norm.normalize_into(obs[k % T], scratch), 200)

        def update_form(k):
            norm.normalize_into(obs, ci[:, :, :no])
            norm.normalize_into(priv, ci[:, :, no:], col0=no, dst_cols=pc - no)
            norm.normalize_into(obs[:T], ai, dst_cols=pa)
        us_upd = _best(update_form, 20)
        us_copy = _best(lambda k: (ci[:, :, :no].copy_(obs), ci[:, :, no : no + npv].copy_(priv), ai[:, :, :no].copy_(obs[:T])), 20)
        print(f"bg_obs_normalize, {what}: rollout step [{N}][{no}] {us_step:.2f} us; update inputs (critic {T + 1} x {N} x {pc}, actor {T} x {N} x {pa}: three "
              f"launches) {us_upd:.2f} us against {us_copy:.2f} us for the three copies they replace", flush=True)


def rollout_pair(pairs=3, N=4096):
    from booster_gym_amd.utils.runner import Runner

    rs = {on: Runner(cfg=_cfg(N, on)) for on in KEYS}
    for r in rs.values():
        obs, infos = r.env.reset()
        r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
        r._rollout_forward = False  # the two launches of a step alone
        r.rollout()

    def step(r, k):
        b, n = r.buffer, k % 24
        src = b["obses"][n] if r.obs_norm is None else r.obs_norm.normalize_into(b["obses"][n], r._obs_normed)
        r.model.sample_actions(src, b["actions"][n], 1, k)
        r.env.step_to(b["actions"][n], b["obses"][n + 1], b["privileged_obses"][n + 1], b["rewards"][n], b["dones"][n], b["time_outs"][n])

    for p in range(pairs):
        us = {on: _best(lambda k, r=rs[on]: step(r, k), 48) for on in (KEYS if p % 2 == 0 else KEYS[::-1])}
        print(f"sample + env step, {N} envs, trimesh: key false {us[False]:.2f} us, key true {us[True]:.2f} us, true / false = {us[True] / us[False]:.4f}", flush=True)
    del rs


def _runner(N, on):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, on)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_obs_norm_"), rank=0))
    return r


def loop(K=20, W=5, pairs=3, N=4096):
    runners = {on: _runner(N, on) for on in KEYS}
    it = {on: 0 for on in KEYS}

    def run(on, n):
        r = runners[on]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it[on]); it[on] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for on in KEYS:
        run(on, W)
    assert runners[True]._resolve_plan().ahead and runners[False]._resolve_plan().ahead
    for p in range(pairs):
        ms = {on: run(on, K) for on in (KEYS if p % 2 == 0 else KEYS[::-1])}
        for on in KEYS:
            print(f"empirical_normalization {str(on).lower():5s}, {N} envs: {ms[on]:.3f} ms per iteration = {1e3 / ms[on]:.2f} iterations/s", flush=True)
        print(f"round {p}: true / false = {ms[True] / ms[False]:.4f}", flush=True)
    for r in runners.values():
        r._flush_log()
    del runners


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    pairs, N = (a[2] if len(a) > 2 else 3), (a[3] if len(a) > 3 else 4096)
    kernels(N)
    rollout_pair(pairs, N)
    loop(*a)
