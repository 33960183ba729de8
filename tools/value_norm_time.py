"""Timing of value normalisation (README "Value normalisation"):

  python tools/value_norm_time.py [K=20] [W=5] [pairs=3] [num_envs=4096]
      (1) bg_critic_values_gae_norm beside bg_critic_values_gae in one run at 24 x num_envs, both forms (h given: the output layer on the stored
          activations, 16 envs per workgroup; h = NULL: the scan alone, 64 envs per workgroup, what the training loop runs): HIP events around 50
          back-to-back launches, best of 5, the sides alternating over `pairs` pairs; and bg_value_norm_update alone;
      (2) the training loop (no instrumentation), key true against false, two runners on one GPU, alternating runs of K iterations after W
          warm-up iterations each: ms per iteration, iterations per second, ratio.  The forward passes during the rollout stay on with the key;
      (3) the SHA-256 over parameters and Adam moments of the key-false runner's first two iterations (a fresh runner, default config), to hold
          beside another tree's."""
import hashlib
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

    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.type": "trimesh", **({"algorithm.normalize_value": True} if on else {})})
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


def kernels(pairs=3, N=4096, T=24):
    from booster_gym_amd.utils.utils import critic_head_forward, critic_values_gae, critic_values_gae_norm, value_norm_update
    from booster_gym_amd.utils.value_norm import triple_of

    g = torch.Generator().manual_seed(1)
    h = torch.nn.functional.elu(torch.randn((T + 1) * N, 128, generator=g)).to(DEV)
    w, b = (torch.randn(1, 128, generator=g) * 0.1).to(DEV), torch.randn(1, generator=g).to(DEV)
    rew = torch.randn(T, N, generator=g).to(DEV)
    dones = (torch.rand(T, N, generator=g) < 0.05).to(DEV)
    touts = ((torch.rand(T, N, generator=g) < 0.03).to(DEV)) & dones
    u = critic_head_forward(h, w, b, torch.empty((T + 1) * N, device=DEV))
    adv, ret = torch.empty(T, N, device=DEV), torch.empty(T, N, device=DEV)
    st = torch.from_numpy(triple_of(2.5, 0.13, 1.0e-2)).to(DEV)
    s3, s6 = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    g16 = (N + 15) // 16
    sc3, sc6 = torch.zeros(3 * g16 + 1, dtype=torch.float64, device=DEV), torch.zeros(6 * g16 + 1, dtype=torch.float64, device=DEV)
    for form, hh in (("h given (16 envs per workgroup)", h), ("h = NULL (64 envs per workgroup)", None)):
        side = {False: lambda k: critic_values_gae(hh, w, b, rew, dones, touts, 0.995, 0.95, u, adv, ret, s3, sc3),
                True: lambda k: critic_values_gae_norm(hh, w, b, rew, dones, touts, 0.995, 0.95, u, adv, ret, st, s6, sc6)}
        for p in range(pairs):
            us = {on: _best(side[on], 50) for on in (KEYS if p % 2 == 0 else KEYS[::-1])}
            print(f"{T} x {N}, {form}, pair {p}: bg_critic_values_gae {us[False]:.2f} us, bg_critic_values_gae_norm {us[True]:.2f} us, "
                  f"norm / plain = {us[True] / us[False]:.4f}", flush=True)
    state = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=DEV)
    print(f"bg_value_norm_update: {_best(lambda k: value_norm_update(s6, state, st, 1.0e-2), 200):.2f} us per call (once per iteration)", flush=True)


def _runner(N, on):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, on)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_value_norm_"), rank=0))
    return r


def digest(r):
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


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
        run(on, 2)
        print(f"normalize_value {str(on).lower():5s}: sha256 over parameters and Adam moments after two iterations {digest(runners[on])}", flush=True)
        run(on, max(W - 2, 0))
    assert runners[True]._resolve_plan().ahead and runners[False]._resolve_plan().ahead and runners[True]._resolve_plan().value_norm
    for p in range(pairs):
        ms = {on: run(on, K) for on in (KEYS if p % 2 == 0 else KEYS[::-1])}
        for on in KEYS:
            print(f"normalize_value {str(on).lower():5s}, {N} envs: {ms[on]:.3f} ms per iteration = {1e3 / ms[on]:.2f} iterations/s", flush=True)
        print(f"round {p}: true / false = {ms[True] / ms[False]:.4f}", flush=True)
    for r in runners.values():
        r._flush_log()
    print("value normaliser after the run:", runners[True].value_norm.scalars(), flush=True)
    del runners


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    pairs, N = (a[2] if len(a) > 2 else 3), (a[3] if len(a) > 3 else 4096)
    kernels(pairs, N)
    loop(*a)
