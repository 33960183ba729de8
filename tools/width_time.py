"""Timing of configurable network widths (README "Network widths"), two modes:

  python tools/width_time.py actor [reps=200]       the fused rollout actor at 4,096 rows: bg_actor_sample at the default widths and bg_actor_sample_mlp
                                                    at 512-256-128 / 128-128 / 512-512-256-128, against the torch path actor(obs) + torch.normal at the
                                                    same widths (HIP events, us per call; run under rocprofv3 --kernel-trace --stats for kernel times)
  python tools/width_time.py loop [K=20] [W=5] [reps=2] [num_envs=4096]
                                                    the training loop (as tools/loop_time.py, no instrumentation) with actor AND critic at the default
                                                    widths, 512-256-128 and 512-512-256-128: ms per iteration, iterations per second"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import torch

ACTOR_ARCHS = [(256, 128, 128), (512, 256, 128), (128, 128), (512, 512, 256, 128)]
LOOP_ARCHS = [None, (512, 256, 128), (512, 512, 256, 128)]


def _events(fn, reps):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def actor(reps=200):
    from booster_gym_amd.utils.model import ACTOR_HIDDEN, ActorCritic

    n = 4096
    torch.manual_seed(0)
    obs = torch.randn(n, 47, device="cuda:0")
    mu, act = torch.empty(n, 12, device="cuda:0"), torch.empty(n, 12, device="cuda:0")
    for h in ACTOR_ARCHS:
        m = ActorCritic(12, 47, 14, actor_hidden=h).to("cuda:0")
        counter = [0]

        def fused():
            m.sample_actions(obs, act, 7, counter[0], mu_out=mu)
            counter[0] += 1

        def torch_path():
            with torch.no_grad():
                mean = m.actor(obs)
                torch.normal(mean, torch.exp(m.logstd).expand_as(mean))

        name = "bg_actor_sample" if h == ACTOR_HIDDEN else "bg_actor_sample_mlp"
        print(f"actor {'-'.join(map(str, h))}, {n} rows: {name} {_events(fused, reps):.2f} us; torch actor(obs) + torch.normal {_events(torch_path, reps):.2f} us",
              flush=True)


def loop(K=20, W=5, reps=2, N=4096):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    for h in LOOP_ARCHS:
        over = {"env.num_envs": N, "terrain.type": "plane"}
        if h is not None:
            over.update({"algorithm.actor_hidden": list(h), "algorithm.critic_hidden": list(h)})
        cfg = load_cfg("T1", over)
        cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
        r = Runner(cfg=cfg)
        r.begin_training(Recorder(cfg, root=tempfile.mkdtemp(prefix="bg_width_"), rank=0))
        it = 0
        for _ in range(W):
            r.train_iteration(it); it += 1
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(K):
                r.train_iteration(it); it += 1
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) / K * 1e3
            name = "default" if h is None else "-".join(map(str, h))
            print(f"actor and critic {name}, {N} envs: {ms:.3f} ms per iteration = {1e3 / ms:.2f} iterations/s", flush=True)
        r._flush_log()
        del r
        torch.cuda.synchronize()


if __name__ == "__main__":
    mode, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    {"actor": actor, "loop": loop}[mode](*args)
