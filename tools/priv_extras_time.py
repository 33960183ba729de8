"""Timing of the critic's privileged extras (README "Privileged extras", env.privileged_extras); writes profiles/priv_extras_time.txt.

  python tools/priv_extras_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/priv_extras_time.txt] [only]
      (1) the env step alone (HIP events around 48 steps of fixed random actions, best of 5, as tools/height_scan_time.py) with the key off and
          with all three groups, alternating: us per step;
      (2) the launches alone: HIP events around 200 back-to-back T1.reset() calls (the reset-all launch sequence: no physics), best of 5, in one run
          and alternating: the key off, ["feet"], all three groups, and terrain.measure_heights at the default 17 x 11 grid (P = 187); the
          differences to the key-off sequence are the bg_priv_extras launch (feet alone, all three) and, beside it, the bg_height_scan launch;
      (3) the training loop (Runner.train_iteration, no instrumentation): W warm-up iterations, then K iterations, and rollout() / update() alone,
          of five configs: the default, all three groups, terrain.measure_heights alone (critic input 248, padded to 256), with ["feet"] (254: still
          256) and with all three groups (272: padded to 512); a Runner each in a process of its own (as a training run is; DESIGN.md 6.17 on
          several Runners in one process), `pairs` times alternating.
  `only` = "kernels" runs (1) and (2), "loop" (3).  The committed profile carries two more sections that this tool does not write: bench.py of
  this tree against a checkout of its parent commit in alternating processes, and the digests of two default iterations in both."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

P = 187
ALL = ["feet", "ground", "joints"]
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _cfg(N, groups=None, scan=False, **over):
    from booster_gym_amd.utils.config import load_cfg

    X = {"feet": 6, "ground": 6, "joints": 12}
    ov = {"env.num_envs": N, "terrain.type": "trimesh", "terrain.measure_heights": scan,
          "env.num_privileged_obs": 14 + (P if scan else 0) + sum(X[g] for g in groups or ())}
    if groups:
        ov["env.privileged_extras"] = list(groups)
    ov.update(over)
    cfg = load_cfg("T1", ov)
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


def _orders(p, keys):
    return keys if p % 2 == 0 else tuple(reversed(keys))


def kernels(pairs=3, N=4096):
    from booster_gym_amd.envs import T1

    envs = {"off": T1(_cfg(N)), "feet": T1(_cfg(N, ["feet"])), "all": T1(_cfg(N, ALL)), "scan": T1(_cfg(N, scan=True))}
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = [(torch.rand(N, 12, generator=g) * 0.6 - 0.3).to("cuda:0") for _ in range(8)]
    for env in envs.values():
        env.reset()
        for k in range(40):
            env.step(acts[k % 8])
    for p in range(pairs):
        us = {k: _best(lambda i, e=envs[k]: e.step(acts[i % 8]), 48) for k in _orders(p, ("off", "all"))}
        say(f"env step, {N} envs, trimesh: key off {us['off']:.2f} us, all three groups {us['all']:.2f} us, on / off = {us['all'] / us['off']:.4f}")
    for p in range(pairs):
        us = {k: _best(lambda i, e=envs[k]: e.reset(), 200) for k in _orders(p, ("off", "feet", "all", "scan"))}
        say(f"reset-all, {N} envs: key off {us['off']:.2f} us, [feet] {us['feet']:.2f} us, all three {us['all']:.2f} us, height scan (P = {P}) "
            f"{us['scan']:.2f} us; differences to the key-off sequence: bg_priv_extras [feet] {us['feet'] - us['off']:.2f} us, all three "
            f"{us['all'] - us['off']:.2f} us, bg_height_scan {us['scan'] - us['off']:.2f} us")
    del envs


SIDES = (("default", dict(groups=None, scan=False)), ("all three groups", dict(groups=ALL, scan=False)),
         ("terrain.measure_heights", dict(groups=None, scan=True)), ("terrain.measure_heights + [feet]", dict(groups=["feet"], scan=True)),
         ("terrain.measure_heights + all three groups", dict(groups=ALL, scan=True)))


def loop(name, side, K=20, W=5, N=4096):
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = _cfg(N, **side)
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_priv_extras_"), rank=0))
    it = 0

    def run(n):
        nonlocal it
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            r.train_iteration(it); it += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    run(W)
    ms = run(K)
    plan = r._resolve_plan()
    T, E = cfg["runner"]["horizon_length"], cfg["runner"]["mini_epochs"]
    phases = {}
    for ph, fn in (("rollout", r.rollout), ("update", r.update)):
        best = 1e9
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        phases[ph] = best
    say(f"training loop, {name}, {N} envs, horizon {T}, {E} mini-epochs (critic input {r.model.critic[0].in_features} padded to {r._critic_in.shape[-1]}: "
        f"critic {plan.critic.fwd} / {plan.critic.bwd}, actor {plan.actor.fwd} / {plan.actor.bwd}, ahead {plan.ahead}): {ms:.3f} ms per iteration = "
        f"{1e3 / ms:.2f} iterations/s; rollout alone {phases['rollout']:.3f} ms, update alone {phases['update']:.3f} ms (best of 3 each)")
    r._flush_log()
    del r
    return ms


if __name__ == "__main__":
    a = sys.argv[1:]
    K, W, pairs, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((20, 5, 3, 4096)))
    out = a[4] if len(a) > 4 and a[4] != "-" else os.path.join(ROOT, "profiles", "priv_extras_time.txt")
    only = a[5] if len(a) > 5 else ""
    if only.startswith("one:"):  # a child of the loop section: one Runner in a process of its own, its line on stdout
        name, side = SIDES[int(only[4:])]
        print("MS %.6f" % loop(name, side, K, W, N), flush=True)
        sys.exit(0)
    say(f"tools/priv_extras_time.py {K} {W} {pairs} {N}{' ' + only if only else ''} on {torch.cuda.get_device_name(0)}")
    if only != "loop":
        kernels(pairs, N)
    if only != "kernels":
        import subprocess

        got = {}
        for q in range(pairs):
            for k, (name, side) in _orders(q, tuple(enumerate(SIDES))):
                res = subprocess.run([sys.executable, os.path.abspath(__file__), str(K), str(W), "1", str(N), os.devnull, f"one:{k}"], capture_output=True, text=True,
                                     timeout=300, check=True)
                for line in res.stdout.splitlines():
                    if line.startswith("training loop"):
                        say(line)
                    elif line.startswith("MS "):
                        got.setdefault(name, []).append(float(line[3:]))
        for name, ms in got.items():
            say(f"  {name}: {min(ms):.3f} to {max(ms):.3f} ms per iteration")
        for on, off in ((SIDES[1][0], SIDES[0][0]), (SIDES[3][0], SIDES[2][0]), (SIDES[4][0], SIDES[2][0])):
            say(f"  {on} against {off}: best {min(got[on]) / min(got[off]):.4f}x, pair by pair " + ", ".join(f"{x / y:.4f}x" for x, y in zip(got[on], got[off])))
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
