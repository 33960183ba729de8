"""Timing of PPO on a recurrent actor (README "Recurrent actor", algorithm.rnn_hidden_size); writes profiles/actor_memory_time.txt.

  python tools/actor_memory_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/actor_memory_time.txt] [only]
      (1) the cell's bias gradients at B = 98,304 rows, H = 128 and 256: bg_gru_bias_partial with a bg_reduce_group of its own descriptor (the whole
          finish: in the update it shares a launch with the other deferred reductions) against the four launches it replaces (bg_elu_backward_colsum
          on dgi and on dgh: a kernel and a finish each), HIP events around 50 back-to-back calls, best of 5, alternating; the outputs are compared
          first (1e-4 of the largest entry);
      (2) the rollout's launch on num_envs rows, 200 calls, best of 5, alternating: bg_actor_sample (the default actor on 47 columns),
          bg_actor_sample_mlp at env.frame_stack 5 (235 columns) and bg_actor_sample_gru with a cell of 128 and of 256, trunks 256-128-128;
      (3) the training loop (Runner.train_iteration, no instrumentation) of the default config, of env.frame_stack 5 and of rnn_hidden_size 128: W
          warm-up iterations, then K iterations, a Runner each in a process of its own (as a training run is), `pairs` times alternating: ms per
          iteration, and rollout() / update() alone.
  `only` = "kernels" runs (1) and (2), "loop" (3).  The committed profile carries one more section that this tool does not write: bench.py of this
  tree against a checkout of its parent commit, in alternating processes."""
import os
import sys
import tempfile
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


def _descs(model):
    from booster_gym_amd import _lib

    lin = [m for m in model.actor if isinstance(m, torch.nn.Linear)]
    return (_lib.MlpLayerDesc * len(lin))(*[_lib.MlpLayerDesc(l.weight.data_ptr(), l.bias.data_ptr(), l.in_features, l.out_features) for l in lin]), len(lin)


def bias(pairs=3, B=98304):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import reduce_group

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()
    for H in (128, 256):
        torch.manual_seed(H)
        C, nb = 3 * H, (B + 127) // 128
        dgi, dgh = torch.randn(B, C, device=DEV), torch.randn(B, C, device=DEV)
        records, cs = torch.empty(nb * 2 * C, device=DEV), torch.empty(nb * C, device=DEV)
        new_i, new_h, old_i, old_h = (torch.zeros(C, device=DEV) for _ in range(4))
        fin = _lib.ReduceProblem()
        fin.partial, fin.groups, fin.record, fin.n_out = records.data_ptr(), nb, 2 * C, 2 * C
        fin.out[0], fin.out[1], fin.n[0], fin.n[1] = new_i.data_ptr(), new_h.data_ptr(), C, C

        def new(k):
            _lib.check(lib.bg_gru_bias_partial(B, H, p(dgi), p(dgh), p(records), st), "bg_gru_bias_partial")
            reduce_group([fin])

        def partial_only(k):
            _lib.check(lib.bg_gru_bias_partial(B, H, p(dgi), p(dgh), p(records), st), "bg_gru_bias_partial")

        def old(k):
            for g, o in ((dgi, old_i), (dgh, old_h)):
                _lib.check(lib.bg_elu_backward_colsum(B, C, p(g), None, p(o), p(cs), st), "bg_elu_backward_colsum")

        new(0); old(0); torch.cuda.synchronize()
        for a, b in ((new_i, old_i), (new_h, old_h)):
            assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()
        mb = 2.0 * B * C * 4 / 1e6
        for q in range(pairs):
            us = {m: _best(f, 50) for m, f in _orders(q, (("new", new), ("partial", partial_only), ("old", old)))}
            say(f"cell bias gradients, B = {B}, H = {H} ({mb:.0f} MB read): bg_gru_bias_partial + a bg_reduce_group of its own {us['new']:.1f} us (the launch alone "
                f"{us['partial']:.1f} us = {mb / us['partial']:.2f} TB/s), the four launches it replaces (bg_elu_backward_colsum x 2) {us['old']:.1f} us "
                f"(new / old = {us['new'] / us['old']:.3f})")


def rollout_launch(pairs=3, N=4096):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()
    torch.manual_seed(1)
    plain, stack = ActorCritic(12, 47, 14).to(DEV), ActorCritic(12, 235, 14).to(DEV)
    cells = {H: ActorCritic(12, 47, 14, memory_hidden=H).to(DEV) for H in (128, 256)}
    obs, sobs = torch.randn(N, 47, device=DEV), torch.randn(N, 235, device=DEV)
    reset = (torch.rand(N, device=DEV) < 0.02).to(torch.uint8)
    act = torch.empty(N, 12, device=DEV)
    packed = plain.pack_actor()
    (sd, ns) = _descs(stack)
    gd = {H: (m.gru_descriptor(),) + _descs(m) + (torch.zeros(N, H, device=DEV),) for H, m in cells.items()}

    def default(k):
        _lib.check(lib.bg_actor_sample(N, p(obs), p(packed), 1, k, None, p(act), st), "bg_actor_sample")

    def frames(k):
        _lib.check(lib.bg_actor_sample_mlp(N, p(sobs), ns, sd, p(stack.logstd), 1, k, None, p(act), st), "bg_actor_sample_mlp")

    def gru(H):
        g, d, n, h = gd[H]
        return lambda k: _lib.check(lib.bg_actor_sample_gru(N, p(obs), 47, g, n, d, p(cells[H].logstd), 1, k, p(reset), p(h), p(h), None, p(act), st),
                                    "bg_actor_sample_gru")

    fns = (("default", default), ("frames", frames), ("gru 128", gru(128)), ("gru 256", gru(256)))
    for q in range(pairs):
        us = {m: _best(f, 200) for m, f in _orders(q, fns)}
        say(f"rollout launch, {N} rows, trunks 256-128-128: bg_actor_sample (47 columns) {us['default']:.2f} us, bg_actor_sample_mlp at env.frame_stack 5 "
            f"(235 columns) {us['frames']:.2f} us, bg_actor_sample_gru with a cell of 128 {us['gru 128']:.2f} us ({us['gru 128'] / us['default']:.3f}x default, "
            f"{us['gru 128'] / us['frames']:.3f}x frame stack), of 256 {us['gru 256']:.2f} us ({us['gru 256'] / us['default']:.3f}x default, "
            f"{us['gru 256'] / us['frames']:.3f}x frame stack)")


def loop(name, over, K=20, W=5, N=4096):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.runner import Runner

    tmp = tempfile.mkdtemp(prefix="bg_actor_memory_")
    cfg = load_cfg("T1", {"env.num_envs": N, **over})
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
    say(f"training loop, {name}, {N} envs, horizon {T}, {E} mini-epochs (actor {plan.actor.fwd} / {plan.actor.bwd}, critic {plan.critic.fwd} / {plan.critic.bwd}, "
        f"one_tail {plan.one_tail}, ahead {plan.ahead}): {ms:.3f} ms per iteration = {N * T / ms / 1e3:.3f} M env-steps/s; rollout alone {phases['rollout']:.3f} ms, "
        f"update alone {phases['update']:.3f} ms (best of 3 each)")
    del r
    torch.cuda.empty_cache()
    return ms


SIDES = (("default", {}), ("env.frame_stack 5", {"env.frame_stack": 5, "env.num_observations": 235}),
         ("algorithm.rnn_hidden_size 128", {"algorithm.rnn_hidden_size": 128}))


if __name__ == "__main__":
    a = sys.argv[1:]
    K, W, pairs, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((20, 5, 3, 4096)))
    out = a[4] if len(a) > 4 and a[4] != "-" else os.path.join(ROOT, "profiles", "actor_memory_time.txt")
    only = a[5] if len(a) > 5 else ""
    if not only.startswith("one:"):
        say(f"tools/actor_memory_time.py {' '.join(a) or f'{K} {W} {pairs} {N}'} on {torch.cuda.get_device_name(0)}")
    if only != "loop" and not only.startswith("one:"):
        bias(pairs)
        rollout_launch(pairs, N)
    if only.startswith("one:"):  # a child of the loop section: one Runner in a process of its own, its line on stdout
        name, over = SIDES[int(only[4:])]
        print("MS %.6f" % loop(name, over, K, W, N), flush=True)
        sys.exit(0)
    if only != "kernels":
        # a process each, as a training run is: with several Runners built one after the other in ONE process, the two-stream mini-epoch (every actor
        # but the default one) of the later ones ran in a slower mode (the same config at 53.7 against 39.1 ms, env.frame_stack 5 at 41.1 against
        # 31.8 ms, the default loop unaffected); why was not established (supposed: which hardware queue a later Runner's side stream lands on)
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
        base = min(got["default"])
        for name, ms in got.items():
            say(f"  {name}: {min(ms):.3f} to {max(ms):.3f} ms per iteration, best = {min(ms) / base:.3f}x the default loop's best")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
