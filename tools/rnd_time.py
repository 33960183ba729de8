"""Timing of curiosity by random network distillation (README "Curiosity"); writes profiles/rnd_time.txt.

  python tools/rnd_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/rnd_time.txt] [parent=DIR]
      (1) the rollout's launch, bg_rnd_reward, on state "critic" (47 + 14 columns) and on the height scan's 234 + 14 (the 512 LDS form), both networks
          256-128, against what it replaces on the same rows: the concatenation copy, two bg_actor_sample_mlp_scan launches on it and the elementwise
          tail (difference, norm, done mask, scaled add) in torch: HIP events around 200 back-to-back calls, best of 5, the sides alternating, `pairs`
          times: us per env step.  The outputs are compared first (the target's embedding bit for bit);
      (2) the predictor's update of one iteration (rnd.num_epochs = 1 full-batch step on 24 x num_envs rows, then the normaliser's move), HIP events
          around it, best of 5, `pairs` times: ms per iteration;
      (3) the training loop (no instrumentation) with the key on and off, one Runner after the other, the sides alternating, `pairs` times: W warm-up
          iterations, then K iterations: ms per iteration, iterations per second;
      with parent=DIR, a built checkout of the parent commit:
      (4) bench.py --gpus 1 --steps 20 --warmup 5 of this tree and of the parent in alternating processes, `pairs` pairs: env-steps/s;
      (5) the SHA-256 over parameters and Adam moments after two default iterations, this tree against the parent, each in a process of its own.
  python tools/rnd_time.py digest ROOT     prints (5)'s SHA for the tree at ROOT (the mode (5) starts)."""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "digest" else ROOT)
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


def launch(pairs=3, N=4096):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import _mlp

    lib, p = _lib.load(), _lib.ptr
    for oc, pc in ((47, 14), (234, 14)):
        torch.manual_seed(oc)
        K = oc + pc
        target, pred = _mlp(K, (256, 128), 12).to(DEV), _mlp(K, (256, 128), 12).to(DEV)
        obs, priv, rows = torch.randn(N, oc, device=DEV), torch.randn(N, pc, device=DEV), torch.zeros(N, K, device=DEV)
        rew0, dones = torch.randn(N, device=DEV), (torch.rand(N, device=DEV) < 0.05)
        d8, stats, w = dones.view(torch.uint8), torch.tensor([0.2, 0.4, 2.5], device=DEV), 0.5
        (td, nt), (pd, npr) = _descs(target), _descs(pred)
        t1, t2, p2, tmp = (torch.empty(N, 12, device=DEV) for _ in range(4))
        rho1, rho2, r1, r2, logstd = torch.empty(N, device=DEV), torch.empty(N, device=DEV), rew0.clone(), rew0.clone(), torch.zeros(12, device=DEV)
        st = _lib.current_stream_ptr()

        def fused(k):
            _lib.check(lib.bg_rnd_reward(N, p(obs), oc, p(priv), pc, nt, td, npr, pd, p(d8), p(stats), w, p(t1), p(rho1), p(r1), st), "bg_rnd_reward")

        def separate(k):
            rows[:, :oc].copy_(obs)
            rows[:, oc:].copy_(priv)
            _lib.check(lib.bg_actor_sample_mlp_scan(N, p(rows), nt, td, K % 47, p(logstd), 1, k, p(t2), p(tmp), st), "bg_actor_sample_mlp_scan")
            _lib.check(lib.bg_actor_sample_mlp_scan(N, p(rows), npr, pd, K % 47, p(logstd), 1, k, p(p2), p(tmp), st), "bg_actor_sample_mlp_scan")
            torch.linalg.vector_norm(p2 - t2, dim=1, out=rho2)
            rho2.masked_fill_(dones, 0.0)
            r2.add_(rho2, alpha=w * 2.5)

        fused(7); separate(7); torch.cuda.synchronize()
        assert torch.equal(t1, t2) and torch.allclose(rho1, rho2, rtol=2e-6, atol=0) and torch.allclose(r1, r2, rtol=1e-6, atol=1e-6), "bg_rnd_reward differs from the launches it replaces"
        for q in range(pairs):
            us = {k: _best(f, 200) for k, f in _orders(q, (("fused", fused), ("separate", separate)))}
            say(f"rollout reward, {N} rows, state {oc} + {pc} columns, target and predictor 256-128: bg_rnd_reward {us['fused']:.2f} us, 2 copies + 2 x "
                f"bg_actor_sample_mlp_scan + the elementwise tail {us['separate']:.2f} us (fused / separate = {us['fused'] / us['separate']:.4f})")


class _Rec:
    def record_episode_statistics(self, env, names, it, stats=None):
        pass

    def record_statistics(self, summary, it):
        pass

    def save(self, d, it):
        pass


def _runner(on, N, over=None):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": N, **({"rnd.enabled": True, "rnd.weight": 0.5} if on else {}), **(over or {})})
    cfg["runner"]["save_interval"] = 10 ** 9  # as bench.py: no checkpoint inside the timed region
    r = Runner(cfg=cfg)
    r.begin_training(recorder=_Rec())
    return r


def update(pairs=3, N=4096, W=3):
    r = _runner(True, N)
    for it in range(W):
        r.train_iteration(it)
    rt, b = r._rnd_trainer, r.buffer
    for q in range(pairs):
        with torch.no_grad():
            ms = _best(lambda k: rt.update(b["obses"][1:], b["privileged_obses"][1:], b["dones"], b["rnd_targets"], b["intrinsic_rewards"]), 5) * 1e-3
        say(f"predictor update + normaliser, {r.cfg['runner']['horizon_length']} x {N} rows, {r._rnd.num_epochs} epoch, plan {rt.sup.plan.fwd} / {rt.sup.plan.bwd}, "
            f"weight gradients of {rt.sup.wgrad_terms} products: {ms:.3f} ms per iteration")
    del r


def loop(K=20, W=5, pairs=3, N=4096):
    for q in range(pairs):
        res = {}
        for on in _orders(q, (False, True)):
            r = _runner(on, N)
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
        say(f"training loop, {N} envs, {K} iterations after {W}: key off {res[False]:.2f} ms per iteration ({1e3 / res[False]:.2f} it/s), key on "
            f"{res[True]:.2f} ms ({1e3 / res[True]:.2f} it/s), on / off = {res[True] / res[False]:.4f}")


def digest(N=4096):
    """SHA-256 over parameters and Adam moments after two iterations of the default config (of whichever tree is first on sys.path)."""
    r = _runner(False, N)
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def against_parent(parent, pairs=3, N=4096):
    trees = (("this tree", ROOT), ("parent", os.path.abspath(parent)))
    for q in range(pairs):
        val = {}
        for name, root in _orders(q, trees):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root, check=True, capture_output=True, text=True).stdout
            val[name] = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"]
        say(f"bench.py --gpus 1 --steps 20 --warmup 5, pair {q}: this tree {val['this tree']:.0f} env-steps/s, parent {val['parent']:.0f} env-steps/s, "
            f"this / parent = {val['this tree'] / val['parent']:.4f}")
    sha = {name: subprocess.run([sys.executable, os.path.abspath(__file__), "digest", root], cwd=root, check=True, capture_output=True, text=True).stdout.split()[-1]
           for name, root in trees}
    say(f"sha256 over parameters and Adam moments after two default iterations at {N} envs: this tree {sha['this tree']}, parent {sha['parent']}: "
        + ("equal" if sha["this tree"] == sha["parent"] else "DIFFERENT"))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "digest":
        print(digest())
        sys.exit(0)
    pos = [x for x in sys.argv[1:] if "=" not in x]
    named = dict(x.split("=", 1) for x in sys.argv[1:] if "=" in x)
    K, W, pairs, N = (int(pos[i]) if len(pos) > i else d for i, d in enumerate((20, 5, 3, 4096)))
    out = named.get("out", os.path.join(ROOT, "profiles", "rnd_time.txt"))
    say(f"# tools/rnd_time.py {K} {W} {pairs} {N} on {torch.cuda.get_device_name(0)}")
    launch(pairs, N)
    update(pairs, N)
    loop(K, W, pairs, N)
    if named.get("parent"):
        against_parent(named["parent"], pairs, N)
    else:
        say("bench.py against the parent commit and the SHA-256 against the parent: not measured in this run (no parent=DIR given)")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("written " + out)
