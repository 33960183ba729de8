"""Timing of a recurrent critic beside the recurrent actor (README "Recurrent actor", algorithm.rnn_critic); writes profiles/rnn_critic_time.txt.

  python tools/rnn_critic_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/rnn_critic_time.txt] [only] [parent=DIR]
      (1) the grouped recurrences: both cells' recurrences as ONE launch (bg_gru_sequence_forward_group / _backward_group, two problems) against the
          same two single launches back to back, at 1,024 and 4,096 envs per problem, T = 24, H = 128: HIP events around 20 back-to-back calls, best
          of 5, the sides alternating, `pairs` pairs, in this process; the outputs are compared first (bit-equal);
      (2) the training loop (Runner.train_iteration, no instrumentation) with algorithm.rnn_hidden_size 128 and the key off and on, at
          runner.num_env_mini_batches 1 and 4, and at 4 with BG_GRU_GROUP=0 and =2: W warm-up iterations, then K, every Runner in a process of its own,
          `pairs` times alternating: ms per iteration, and rollout() / update() alone;
      (3) with parent=DIR, a built checkout of the parent commit: `bench.py --gpus 1 --steps K --warmup W` of this tree against it, in alternating
          processes, `pairs` pairs;
      (4) with parent=DIR: SHA-256 over parameters and Adam's moments after two iterations at 128 envs of the default config, of rnn_hidden_size 128
          and of rnn_hidden_size 128 with num_env_mini_batches 4, this tree against the parent (the key off changes no bit).
  `only` = "group", "loop", "bench" or "digest" runs that section alone (the committed profile is ONE call with every section).  Whether a recurrent
  critic trains a better walker is evaluate.py's study, not this tool's."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LINES = []
RNN = {"algorithm.rnn_hidden_size": 128}
SIDES = (("rnn_hidden_size 128, K = 1", RNN, {}), ("... with rnn_critic, K = 1", {**RNN, "algorithm.rnn_critic": True}, {}),
         ("rnn_hidden_size 128, K = 4", {**RNN, "runner.num_env_mini_batches": 4}, {}),
         ("... with rnn_critic, K = 4", {**RNN, "algorithm.rnn_critic": True, "runner.num_env_mini_batches": 4}, {}),
         ("... with rnn_critic, K = 4, BG_GRU_GROUP=0", {**RNN, "algorithm.rnn_critic": True, "runner.num_env_mini_batches": 4}, {"BG_GRU_GROUP": "0"}),
         ("... with rnn_critic, K = 4, BG_GRU_GROUP=2", {**RNN, "algorithm.rnn_critic": True, "runner.num_env_mini_batches": 4}, {"BG_GRU_GROUP": "2"}))
DIGESTS = (("default", {}), ("rnn_hidden_size 128", RNN), ("rnn_hidden_size 128, num_env_mini_batches 4", {**RNN, "runner.num_env_mini_batches": 4}))


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _orders(p, keys):
    return keys if p % 2 == 0 else tuple(reversed(keys))


def group(pairs=3, T=24, H=128):
    import torch

    from booster_gym_amd import _lib

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()

    def best(fn, reps=20, rounds=5):
        b = 1e9
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            b = min(b, e0.elapsed_time(e1) / reps * 1e3)
        return b

    for N in (1024, 4096):
        torch.manual_seed(N)
        B, cells = T * N, []
        for k in range(2):
            rnd = lambda *s: torch.randn(*s, device=DEV)
            c = dict(gi=rnd(B, 3 * H), h0=rnd(N, H) * 0.5, reset=(torch.rand(T, N, device=DEV) < 0.02).to(torch.uint8), W=rnd(3 * H, H) / H ** 0.5, b=rnd(3 * H) * 0.1,
                     dh_ext=rnd(B, H))
            for side in ("one", "grp"):
                c[side] = {n: torch.zeros(B, w, device=DEV) for n, w in (("h_prev", H), ("h", H), ("gates", 4 * H), ("dgi", 3 * H), ("dgh", 3 * H))}
            cells.append(c)
        fw = (_lib.GruForwardProblem * 2)(*[_lib.GruForwardProblem(T, N, p(c["gi"]), p(c["h0"]), p(c["reset"]), p(c["W"]), p(c["b"]), p(c["grp"]["h_prev"]),
                                                                  p(c["grp"]["h"]), p(c["grp"]["gates"])) for c in cells])
        bw = (_lib.GruBackwardProblem * 2)(*[_lib.GruBackwardProblem(T, N, p(c["dh_ext"]), p(c["grp"]["gates"]), p(c["grp"]["h_prev"]), p(c["reset"]), p(c["W"]),
                                                                    p(c["grp"]["dgi"]), p(c["grp"]["dgh"]), None) for c in cells])

        def fwd_single():
            for c in cells:
                o = c["one"]
                _lib.check(lib.bg_gru_sequence_forward(T, N, H, p(c["gi"]), p(c["h0"]), p(c["reset"]), p(c["W"]), p(c["b"]), p(o["h_prev"]), p(o["h"]), p(o["gates"]), st), "forward")

        def bwd_single():
            for c in cells:
                o = c["one"]
                _lib.check(lib.bg_gru_sequence_backward(T, N, H, p(c["dh_ext"]), p(o["gates"]), p(o["h_prev"]), p(c["reset"]), p(c["W"]), p(o["dgi"]), p(o["dgh"]), None, st),
                           "backward")

        fwd_group = lambda: _lib.check(lib.bg_gru_sequence_forward_group(fw, 2, H, st), "bg_gru_sequence_forward_group")
        bwd_group = lambda: _lib.check(lib.bg_gru_sequence_backward_group(bw, 2, H, st), "bg_gru_sequence_backward_group")
        fwd_single(); bwd_single(); fwd_group(); bwd_group(); torch.cuda.synchronize()
        assert all(torch.equal(c["one"][n], c["grp"][n]) for c in cells for n in c["one"]), "the group's outputs are not the single launches'"
        for q in range(pairs):
            us = {m: best(f) for m, f in _orders(q, (("fwd single", fwd_single), ("fwd group", fwd_group), ("bwd single", bwd_single), ("bwd group", bwd_group)))}
            say(f"two recurrences, {N} envs each, T = {T}, H = {H}, pair {q}: forward as two single launches {us['fwd single']:.1f} us, as one group "
                f"{us['fwd group']:.1f} us (group / single = {us['fwd group'] / us['fwd single']:.3f}); backward {us['bwd single']:.1f} us against "
                f"{us['bwd group']:.1f} us ({us['bwd group'] / us['bwd single']:.3f})")


def _runner(over, N, tmp):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    cfg = load_cfg("T1", {"env.num_envs": N, **over})
    cfg["runner"]["save_interval"] = 10 ** 9  # no checkpoint inside the timed region
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tmp, rank=0))
    return r, cfg


def loop(name, over, K=20, W=5, N=4096):
    import torch

    r, cfg = _runner(over, N, tempfile.mkdtemp(prefix="bg_rnn_critic_"))
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
    r._resolve_plan()
    # what a step issues: grouped recurrences exist in the one-stream steps of runner.num_env_mini_batches with both cells only
    grp = {0: "none", 1: "forward", 2: "forward and backward"}[int(r._mb_plan.gru_group) if r._env_mini_batches > 1 else 0]
    say(f"training loop, {name}, {N} envs, horizon {T}, {E} mini-epochs (grouped recurrences: {grp}): {ms:.3f} ms per iteration = "
        f"{N * T / ms / 1e3:.3f} M env-steps/s; rollout alone {phases['rollout']:.3f} ms, update alone {phases['update']:.3f} ms (best of 3 each)")
    return ms


def digest(over, N=128):
    """SHA-256 over parameters and Adam's moments after two iterations; runs in whichever tree is first on sys.path."""
    import torch

    r, _ = _runner({"terrain.type": "plane", "runner.horizon_length": 8, "runner.mini_epochs": 2, **over}, N, tempfile.mkdtemp(prefix="bg_rnn_critic_"))
    for it in range(2):
        r.train_iteration(it)
    r._flush_log()
    torch.cuda.synchronize()
    o, h = r.optimizer, hashlib.sha256()
    for t in list(r.model.state_dict().values()) + [o.flat, o.exp_avg, o.exp_avg_sq, o.lr]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _child(tree, args, env=None, timeout=600):
    """This file's code on the tree `tree` (its package first on the path), in a process of its own."""
    envv = dict(os.environ, **(env or {}), BG_TIME_TREE=tree)
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout, check=True, env=envv, cwd=tree).stdout


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("BG_TIME_TREE", ROOT))
    a = [x for x in sys.argv[1:] if not x.startswith("parent=")]
    parent = next((x[7:] for x in sys.argv[1:] if x.startswith("parent=")), None)
    K, W, pairs, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((20, 5, 3, 4096)))
    out = a[4] if len(a) > 4 and a[4] != "-" else os.path.join(ROOT, "profiles", "rnn_critic_time.txt")
    only = a[5] if len(a) > 5 else ""
    if only.startswith("one:"):  # a child of the loop section: one Runner in a process of its own, its line on stdout
        name, over, _ = SIDES[int(only[4:])]
        print("MS %.6f" % loop(name, over, K, W, N), flush=True)
        sys.exit(0)
    if only.startswith("sha:"):  # a child of the digest section
        print("SHA " + digest(DIGESTS[int(only[4:])][1]), flush=True)
        sys.exit(0)
    import torch

    say(f"tools/rnn_critic_time.py {K} {W} {pairs} {N}{' ' + only if only else ''}{' with a parent checkout' if parent else ''} on {torch.cuda.get_device_name(0)}")
    if only in ("", "group"):
        group(pairs)
    if only in ("", "loop"):
        got = {}
        for q in range(pairs):
            for k, (name, over, env) in _orders(q, tuple(enumerate(SIDES))):
                for line in _child(ROOT, [str(K), str(W), "1", str(N), os.devnull, f"one:{k}"], env).splitlines():
                    if line.startswith("training loop"):
                        say(line)
                    elif line.startswith("MS "):
                        got.setdefault(name, []).append(float(line[3:]))
        for name, ms in got.items():
            say(f"  {name}: {min(ms):.3f} to {max(ms):.3f} ms per iteration")
    if only in ("", "bench") and parent:
        got = {}
        for q in range(pairs):
            for side, tree in _orders(q, (("this tree", ROOT), ("parent", parent))):
                res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W)], capture_output=True, text=True, timeout=900,
                                     check=True, cwd=tree)
                value = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])["value"]
                got.setdefault(side, []).append(value)
                say(f"bench.py --gpus 1 --steps {K} --warmup {W}, pair {q}, {side}: {value:.0f} env-steps/s")
        for side, v in got.items():
            say(f"  {side}: {min(v):.0f} to {max(v):.0f} env-steps/s")
    if only in ("", "digest") and parent:
        for k, (name, _) in enumerate(DIGESTS):
            sha = {side: _child(tree, ["1", "1", "1", "128", os.devnull, f"sha:{k}"]).split("SHA ")[-1].strip() for side, tree in (("this tree", ROOT), ("parent", parent))}
            say(f"two iterations at 128 envs, {name}: this tree {sha['this tree']}, parent {sha['parent']} ({'equal' if sha['this tree'] == sha['parent'] else 'DIFFERENT'})")
    say("not measured: whether a recurrent critic trains a better walker (evaluate.py's study), H = 256 in the loop")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
