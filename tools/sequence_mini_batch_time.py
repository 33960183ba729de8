"""Timing of the env-wise sequence mini-batches of a recurrent actor (README "Recurrent actor", runner.num_env_mini_batches); writes
profiles/sequence_mini_batch_time.txt.

  python tools/sequence_mini_batch_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/sequence_mini_batch_time.txt] [only]
      (1) bg_gather_sequences at 4 mini-batches on the recurrent update's nine streams (the critic's and the cell's padded rows of 64 columns, actions,
          old mu, three scalars: 155 floats per row; the state [N][128]; the one-byte reset flags) against bg_gather_rows on the seven per-row float
          streams with a random row permutation: HIP events around 50 back-to-back launches, best of 5, alternating; the outputs are compared with
          torch indexing first; time, bytes (every row read once and written once, the permutation read once per stream and row) and TB/s of both;
      (2) the recurrence at fewer envs: bg_gru_sequence_forward and bg_gru_sequence_backward at num_envs, num_envs / 2 and num_envs / 4 envs, horizon
          24, H = 128, likewise;
      (3) the training loop (Runner.train_iteration, no instrumentation) of algorithm.rnn_hidden_size 128 with runner.num_env_mini_batches absent, 2
          and 4: W warm-up iterations, then K iterations, a Runner each in a process of its own (DESIGN 6.17 says why), `pairs` times alternating: ms per
          iteration, optimiser steps per second, and rollout() / update() alone.
  `only` = "kernels" runs (1) and (2), "loop" (3).  The committed profile carries one more section that this tool does not write: bench.py and the
  digests of this tree against a checkout of its parent commit, in alternating processes."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

DEV = "cuda:0"
LINES = []
T, H = 24, 128


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


def gather(pairs=3, N=4096, K=4):
    from booster_gym_amd import _lib

    lib, B, n, st = _lib.load(), T * N, N // K, _lib.current_stream_ptr()
    torch.manual_seed(N)
    widths = (64, 64, 12, 12, 1, 1, 1)
    srcs = [torch.randn(T, N, w, device=DEV) for w in widths]
    h0, resets = torch.randn(N, H, device=DEV), (torch.rand(T, N, device=DEV) < 0.02).to(torch.uint8)
    seq_src = srcs + [h0, resets]
    seq_dst = [torch.empty_like(s) for s in seq_src]
    seq = (_lib.SequenceStream * 9)(*[_lib.SequenceStream(s.data_ptr(), d.data_ptr(), s.shape[-1] if s.dim() == 3 else (H if s is h0 else 1), s.element_size(),
                                                          1 if s is h0 else 0, 0) for s, d in zip(seq_src, seq_dst)])
    row_dst = [torch.empty_like(s) for s in srcs]
    rows = (_lib.GatherStream * 7)(*[_lib.GatherStream(s.data_ptr(), d.data_ptr(), w, 0) for s, d, w in zip(srcs, row_dst, widths)])
    # (fresh permutations per launch, as in the loop: filled outside the timed launches)
    sigmas = [torch.randperm(N, device=DEV).to(torch.int32) for _ in range(4)]
    perms = [torch.randperm(B, device=DEV).to(torch.int32) for _ in range(4)]
    new = lambda k: _lib.check(lib.bg_gather_sequences(T, N, K, _lib.ptr(sigmas[k % 4]), seq, 9, st), "bg_gather_sequences")
    old = lambda k: _lib.check(lib.bg_gather_rows(B, B, _lib.ptr(perms[k % 4]), rows, 7, st), "bg_gather_rows")
    new(1); old(1); torch.cuda.synchronize()
    by_envs = lambda s, sg: s[:, sg.long()].reshape(T, K, n, *s.shape[2:]).transpose(0, 1).reshape(s.shape)
    for s, d in zip(seq_src, seq_dst):
        assert torch.equal(d, s[sigmas[1].long()] if s is h0 else by_envs(s, sigmas[1]))
    for s, d in zip(srcs, row_dst):
        assert torch.equal(d.view(B, -1), s.view(B, -1)[perms[1].long()])
    new_bytes = 4 * B * (2 * sum(widths) + len(widths)) + B * (2 + 4) + 4 * N * (2 * H + 1)
    old_bytes = 4 * B * (2 * sum(widths) + len(widths))
    for q in range(pairs):
        us = {m: _best(f, 50) for m, f in _orders(q, (("new", new), ("old", old)))}
        say(f"gather, {N} envs x {T} steps: bg_gather_sequences at {K} mini-batches, nine streams ({sum(widths)} floats and a byte per row, the state [{N}][{H}]) "
            f"{us['new']:.2f} us, {new_bytes / 1e6:.1f} MB, {new_bytes / us['new'] / 1e6:.3f} TB/s; bg_gather_rows, the seven per-row float streams by a random "
            f"row permutation {us['old']:.2f} us, {old_bytes / 1e6:.1f} MB, {old_bytes / us['old'] / 1e6:.3f} TB/s; time per byte new / old = "
            f"{(us['new'] / new_bytes) / (us['old'] / old_bytes):.3f}")


def recurrence(pairs=3, N=4096):
    from booster_gym_amd import _lib

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()
    torch.manual_seed(N + 1)
    w_hh, b_hh = torch.randn(3 * H, H, device=DEV) * 0.05, torch.randn(3 * H, device=DEV) * 0.05
    sides = []
    for n in (N, N // 2, N // 4):
        B = T * n
        gi, h0, rs = torch.randn(B, 3 * H, device=DEV), torch.randn(n, H, device=DEV) * 0.1, (torch.rand(T, n, device=DEV) < 0.02).to(torch.uint8)
        h_prev, h, gates = torch.zeros(B, H, device=DEV), torch.zeros(B, H, device=DEV), torch.zeros(B, 4 * H, device=DEV)
        dh, dgi, dgh = torch.randn(B, H, device=DEV) * 0.01, torch.zeros(B, 3 * H, device=DEV), torch.zeros(B, 3 * H, device=DEV)
        fwd = lambda k, a=(T, n, H, p(gi), p(h0), p(rs), p(w_hh), p(b_hh), p(h_prev), p(h), p(gates), st): _lib.check(lib.bg_gru_sequence_forward(*a), "bg_gru_sequence_forward")
        bwd = lambda k, a=(T, n, H, p(dh), p(gates), p(h_prev), p(rs), p(w_hh), p(dgi), p(dgh), None, st): _lib.check(lib.bg_gru_sequence_backward(*a), "bg_gru_sequence_backward")
        fwd(0); bwd(0); torch.cuda.synchronize()
        sides.append((n, fwd, bwd, (gi, h0, rs, h_prev, h, gates, dh, dgi, dgh)))
    for q in range(pairs):
        us = {}
        for n, fwd, bwd, _ in _orders(q, tuple(sides)):
            us[n] = (_best(fwd, 20), _best(bwd, 20))
        say(f"recurrence, horizon {T}, H = {H}: " + "; ".join(f"{n} envs ({(n + 15) // 16} workgroups) forward {us[n][0]:.1f} us, backward {us[n][1]:.1f} us" for n, *_ in sides)
            + f"; {N // 4} envs / {N} envs: forward {us[N // 4][0] / us[N][0]:.3f}, backward {us[N // 4][1] / us[N][1]:.3f}")


def loop(name, over, K=20, W=5, N=4096):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    tmp = tempfile.mkdtemp(prefix="bg_sequence_mini_batch_")
    cfg = load_cfg("T1", {"env.num_envs": N, "algorithm.rnn_hidden_size": H, **over})
    cfg["runner"]["save_interval"] = 10 ** 9  # no checkpoint inside the timed region
    r = Runner(cfg=cfg)
    r.begin_training(Recorder(cfg, root=tmp, rank=0))
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
    E, steps = cfg["runner"]["mini_epochs"], r.optimizer.step_count // it
    phases = {}
    for ph, fn in (("rollout", r.rollout), ("update", r.update)):
        best = 1e9
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        phases[ph] = best
    say(f"training loop, {name}, {N} envs, horizon {T}, H = {H}, {E} mini-epochs, {steps} optimiser steps per iteration: {ms:.3f} ms per iteration = "
        f"{steps / ms * 1e3:.0f} optimiser steps/s = {N * T / ms / 1e3:.3f} M env-steps/s; rollout alone {phases['rollout']:.3f} ms, update alone {phases['update']:.3f} ms "
        f"= {phases['update'] / steps:.3f} ms per step (best of 3 each)")
    return ms


SIDES = (("runner.num_env_mini_batches absent", {}), ("runner.num_env_mini_batches 2", {"runner.num_env_mini_batches": 2}),
         ("runner.num_env_mini_batches 4", {"runner.num_env_mini_batches": 4}))


if __name__ == "__main__":
    a = sys.argv[1:]
    K, W, pairs, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((20, 5, 3, 4096)))
    out = a[4] if len(a) > 4 and a[4] != "-" else os.path.join(ROOT, "profiles", "sequence_mini_batch_time.txt")
    only = a[5] if len(a) > 5 else ""
    if only.startswith("one:"):  # a child of the loop section: one Runner in a process of its own, its line on stdout
        name, over = SIDES[int(only[4:])]
        print("MS %.6f" % loop(name, over, K, W, N), flush=True)
        sys.exit(0)
    say(f"tools/sequence_mini_batch_time.py {' '.join(a) or f'{K} {W} {pairs} {N}'} on {torch.cuda.get_device_name(0)}")
    if only != "loop":
        gather(pairs, N)
        recurrence(pairs, N)
    if only != "kernels":
        import subprocess

        got = {}
        for q in range(pairs):
            for k, (name, over) in _orders(q, tuple(enumerate(SIDES))):
                res = subprocess.run([sys.executable, os.path.abspath(__file__), str(K), str(W), "1", str(N), os.devnull, f"one:{k}"], capture_output=True, text=True,
                                     timeout=300, check=True)
                for line in res.stdout.splitlines():
                    if line.startswith("training loop"):
                        say(line)
                    elif line.startswith("MS "):
                        got.setdefault(name, []).append(float(line[3:]))
        base = min(got[SIDES[0][0]])
        for name, ms in got.items():
            say(f"  {name}: {min(ms):.3f} to {max(ms):.3f} ms per iteration, best = {min(ms) / base:.3f}x the absent key's best")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
