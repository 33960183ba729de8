"""Timing of the learned state estimator (README "State estimator"); writes profiles/estimator_time.txt.

  python tools/estimator_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/estimator_time.txt]
      (1) the rollout's launch, bg_actor_sample_est, at H = 1 / E = 4 and at H = 5 / E = 4 (estimator 256-128, actor 256-128-128) against the three
          launches it replaces (bg_actor_sample_mlp of the estimator, the concatenation copy, bg_actor_sample_mlp_scan) and against the launch of an
          actor without an estimator on the same rows (bg_actor_sample at H = 1, bg_actor_sample_mlp at H = 5): HIP events around 200 back-to-back
          calls, best of 5, the sides alternating, `pairs` times: us per env step's inference.  The outputs are compared bit for bit first;
      (2) the estimator's update of one iteration (estimator.num_epochs = 2 full-batch steps on 24 x num_envs rows) at H = 1 and H = 5, HIP events
          around it, best of 5, `pairs` times: ms per iteration;
      (3) the training loop (no instrumentation) with the key on and off at H = 1 and H = 5, one Runner after the other, the sides alternating,
          `pairs` times: W warm-up iterations, then K iterations: ms per iteration, iterations per second.
  The committed profile carries one more section that this tool does not write: bench.py of this tree against a checkout of its parent commit."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

DEV = "cuda:0"
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


def _descs(seq):
    from booster_gym_amd import _lib

    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    return (_lib.MlpLayerDesc * len(lin))(*[_lib.MlpLayerDesc(l.weight.data_ptr(), l.bias.data_ptr(), l.in_features, l.out_features) for l in lin]), len(lin)


def launch(pairs=3, N=4096, E=4):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p = _lib.load(), _lib.ptr
    for H in (1, 5):
        torch.manual_seed(H)
        F = 47 * H
        m, plain = ActorCritic(12, F, 14, estimator_hidden=(256, 128), estimator_cols=E).to(DEV), ActorCritic(12, F, 14).to(DEV)
        obs, rows = torch.randn(N, F, device=DEV), torch.zeros(N, F + E, device=DEV)
        (ed, ne), (ad, na) = _descs(m.estimator), _descs(m.actor)
        e1, a1, e2, a2, tmp, a3 = (torch.empty(N, 12, device=DEV) for _ in range(6))
        st = _lib.current_stream_ptr()
        packed = plain.pack_actor()

        def fused(k):
            _lib.check(lib.bg_actor_sample_est(N, p(obs), ne, ed, E, na, ad, p(m.logstd), 1, k, p(e1), None, p(a1), st), "bg_actor_sample_est")

        def separate(k):
            _lib.check(lib.bg_actor_sample_mlp(N, p(obs), ne, ed, p(m.logstd), 1, k, p(e2), p(tmp), st), "bg_actor_sample_mlp")
            rows[:, :F].copy_(obs)
            rows[:, F:].copy_(e2[:, :E])
            _lib.check(lib.bg_actor_sample_mlp_scan(N, p(rows), na, ad, E, p(m.logstd), 1, k, None, p(a2), st), "bg_actor_sample_mlp_scan")

        def without(k):
            plain.sample_actions(obs, a3, 1, k, packed=packed)

        fused(7); separate(7); torch.cuda.synchronize()
        assert torch.equal(a1, a2) and torch.equal(e1, e2), "bg_actor_sample_est differs from its stand-alone launches"
        name = "bg_actor_sample" if packed is not None else "bg_actor_sample_mlp"
        for q in range(pairs):
            us = {k: _best(f, 200) for k, f in _orders(q, (("fused", fused), ("separate", separate), ("without", without)))}
            say(f"rollout inference, {N} rows, H = {H}, E = {E}, estimator 256-128, actor 256-128-128: bg_actor_sample_est {us['fused']:.2f} us, "
                f"bg_actor_sample_mlp + 2 copies + bg_actor_sample_mlp_scan {us['separate']:.2f} us (fused / separate = {us['fused'] / us['separate']:.4f}), "
                f"{name} of an actor without an estimator {us['without']:.2f} us")


def _runner(H, on, N):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    class Rec:
        def record_episode_statistics(self, env, names, it, stats=None):
            pass

        def record_statistics(self, summary, it):
            pass

        def save(self, d, it):
            pass

    r = Runner(cfg=load_cfg("T1", {"env.num_envs": N, "env.frame_stack": H, "env.num_observations": 47 * H, "estimator.enabled": on}))
    r.begin_training(recorder=Rec())
    return r


def update(pairs=3, N=4096, W=3):
    for H in (1, 5):
        r = _runner(H, True, N)
        for it in range(W):
            r.train_iteration(it)
        T = r.cfg["runner"]["horizon_length"]
        et, obses, priv = r._est_trainer, r.buffer["obses"][:T], r.buffer["privileged_obses"][:T]
        for q in range(pairs):
            with torch.no_grad():
                ms = _best(lambda k: et.update(obses, priv), 5) * 1e-3
            say(f"estimator update, {T} x {N} rows, H = {H}, {r._est.num_epochs} epochs, plan {et.sup.plan.fwd} / {et.sup.plan.bwd}, weight gradients of "
                f"{et.sup.wgrad_terms} products: {ms:.3f} ms per iteration")
        del r


def loop(K=20, W=5, pairs=3, N=4096, frames=(1, 5)):
    for H in frames:
        for q in range(pairs):
            res = {}
            for on in _orders(q, (False, True)):
                r = _runner(H, on, N)
                for it in range(W):
                    r.train_iteration(it)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for it in range(W, W + K):
                    r.train_iteration(it)
                torch.cuda.synchronize()
                res[on] = (time.perf_counter() - t0) / K * 1e3
                r._flush_log()
                del r
            say(f"training loop, {N} envs, H = {H}, {K} iterations after {W}: key off {res[False]:.2f} ms per iteration ({1e3 / res[False]:.2f} it/s), key on "
                f"{res[True]:.2f} ms ({1e3 / res[True]:.2f} it/s), on / off = {res[True] / res[False]:.4f}")


if __name__ == "__main__":
    a = sys.argv[1:]
    K, W, pairs, N = (int(a[i]) if len(a) > i else d for i, d in enumerate((20, 5, 3, 4096)))
    out = a[4] if len(a) > 4 else os.path.join(ROOT, "profiles", "estimator_time.txt")
    say(f"# tools/estimator_time.py {K} {W} {pairs} {N} on {torch.cuda.get_device_name(0)}")
    launch(pairs, N)
    update(pairs, N)
    loop(K, W, pairs, N)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written " + out)
