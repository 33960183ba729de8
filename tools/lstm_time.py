"""Timing of PPO on an LSTM actor (README "Recurrent actor", algorithm.rnn_cell: "lstm") beside the GRU at the same H; writes profiles/lstm_time.txt.

  python tools/lstm_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/lstm_time.txt] [only]
      every figure stands beside the GRU's at the same H in the same run, the sides alternating, `pairs` times; HIP events, best of 5:
      (1) the rollout's launch on num_envs rows, 200 calls: bg_actor_sample_lstm against bg_actor_sample_gru, trunks 256-128-128;
      (2) the forward and the backward recurrence at T = 24 on num_envs envs, 20 calls: bg_lstm_sequence_forward / _backward against the GRU's; beside
          them the 24 bg_mlp_layer_forward(num_envs, H, 4H) launches a recurrence replaces, and the fp32-MFMA time of its FLOPs at the peak below;
      (3) the cell's bias gradients at B = 24 num_envs rows, 50 calls: bg_lstm_bias_partial with a bg_reduce_group of its two descriptors against
          bg_gru_bias_partial with its one;
      (4) the training loop (tools/actor_memory_time.py's `loop`), rnn_hidden_size 128 with rnn_cell "gru" and "lstm": a Runner each in a process of
          its own, every child under its own time limit.
  `only` = "kernels" runs (1) to (3), "loop" (4); "wide" (out: profiles/lstm_512_time.txt) runs the LSTM at H = 512 (algorithm.rnn_hidden_size: 512)
  beside the LSTM at H = 256 in the same run: the rollout launch, both recurrences, the bias sums, the 24 bg_mlp_layer_forward(num_envs, H, 4H)
  launches and the peak time of the FLOPs at either width, then the training loop at 256 and 512; "wide_kernels" / "wide_loop" run its halves.
  "row" (out: profiles/rnn_input_time.txt; algorithm.rnn_input: "row") runs every cell's _row launch at K = 234 (47 + the 187-point height scan) beside
  the same cell's 47-input launch and beside bg_actor_sample_mlp_scan at that K, then the training loop of the LSTM at H = 256 on the perceptive env
  with the cell on the observation and on the row; "row_kernels" / "row_loop" run its halves.
  The committed profile carries sections this tool does not write: bench.py of this tree against a
  checkout of its parent commit, and the SHA-256 digests."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from actor_memory_time import DEV, LINES, _best, _descs, _orders, loop, say

PEAK_FP32_MFMA = 157.3e12  # MI355X, fp32 matrix FLOP/s (vendor figure)
T = 24
SIDES = (("rnn_cell gru", {"algorithm.rnn_hidden_size": 128}), ("rnn_cell lstm", {"algorithm.rnn_hidden_size": 128, "algorithm.rnn_cell": "lstm"}),
         ("lstm 256", {"algorithm.rnn_hidden_size": 256, "algorithm.rnn_cell": "lstm"}), ("lstm 512", {"algorithm.rnn_hidden_size": 512, "algorithm.rnn_cell": "lstm"}),
         ("lstm 256, critic scan", {"algorithm.rnn_hidden_size": 256, "algorithm.rnn_cell": "lstm", "terrain.measure_heights": True, "env.num_privileged_obs": 201}),
         ("lstm 256, row 234", {"algorithm.rnn_hidden_size": 256, "algorithm.rnn_cell": "lstm", "algorithm.rnn_input": "row", "terrain.measure_heights": True,
                                "terrain.actor_heights": True, "env.num_observations": 234, "env.num_privileged_obs": 201}))


def rollout_launch(pairs, N):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()
    torch.manual_seed(1)
    obs, act = torch.randn(N, 47, device=DEV), torch.empty(N, 12, device=DEV)
    reset = (torch.rand(N, device=DEV) < 0.02).to(torch.uint8)
    for H in (128, 256):
        m = {c: ActorCritic(12, 47, 14, memory_hidden=H, memory_cell=c).to(DEV) for c in ("gru", "lstm")}
        d = {c: (m[c].gru_descriptor(),) + _descs(m[c]) for c in m}
        h, s = torch.zeros(N, H, device=DEV), torch.zeros(2, N, H, device=DEV)

        def gru(k):
            g, l, n = d["gru"]
            _lib.check(lib.bg_actor_sample_gru(N, p(obs), 47, g, n, l, p(m["gru"].logstd), 1, k, p(reset), p(h), p(h), None, p(act), st), "bg_actor_sample_gru")

        def lstm(k):
            g, l, n = d["lstm"]
            _lib.check(lib.bg_actor_sample_lstm(N, p(obs), 47, g, n, l, p(m["lstm"].logstd), 1, k, p(reset), p(s[0]), p(s[0]), p(s[1]), p(s[1]), None, p(act), st),
                       "bg_actor_sample_lstm")

        for q in range(pairs):
            us = {k: _best(f, 200) for k, f in _orders(q, (("gru", gru), ("lstm", lstm)))}
            say(f"rollout launch, {N} rows, H = {H}, trunk 256-128-128: bg_actor_sample_lstm {us['lstm']:.2f} us, bg_actor_sample_gru {us['gru']:.2f} us "
                f"(lstm / gru = {us['lstm'] / us['gru']:.3f})")


def recurrences(pairs, N):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import reduce_group

    lib, p, st, B = _lib.load(), _lib.ptr, _lib.current_stream_ptr(), T * N
    for H in (128, 256):
        torch.manual_seed(H)
        z = lambda *s: torch.zeros(*s, device=DEV)
        r = lambda *s: torch.randn(*s, device=DEV)
        reset, dh = (torch.rand(T, N, device=DEV) < 0.02).to(torch.uint8), r(B, H)
        G = dict(gi=r(B, 3 * H), W=r(3 * H, H) * H ** -0.5, b=r(3 * H) * 0.1, h0=r(N, H), hp=z(B, H), h=z(B, H), gates=z(B, 4 * H), dgi=z(B, 3 * H), dgh=z(B, 3 * H))
        L = dict(gi=r(B, 4 * H), W=r(4 * H, H) * H ** -0.5, b=r(4 * H) * 0.1, s0=r(2, N, H), hp=z(B, H), cp=z(B, H), h=z(B, H), c=z(B, H), gates=z(B, 5 * H), dg=z(B, 4 * H))
        x, Wl, yl = r(N, H), r(4 * H, H), z(N, 4 * H)
        nb = (B + 127) // 128
        rec_g, rec_l, sums = z(nb * 6 * H), z(nb * 4 * H), [z(4 * H) for _ in range(2)]
        fin_g = _lib.ReduceProblem()
        fin_g.partial, fin_g.groups, fin_g.record, fin_g.n_out = rec_g.data_ptr(), nb, 6 * H, 6 * H
        fin_g.out[0], fin_g.out[1], fin_g.n[0], fin_g.n[1] = sums[0].data_ptr(), sums[1].data_ptr(), 3 * H, 3 * H
        fins_l = []
        for s in sums:
            f = _lib.ReduceProblem()
            f.partial, f.groups, f.record, f.n_out, f.out[0], f.n[0] = rec_l.data_ptr(), nb, 4 * H, 4 * H, s.data_ptr(), 4 * H
            fins_l.append(f)
        ck = _lib.check
        fns = {
            "gru fwd": lambda k: ck(lib.bg_gru_sequence_forward(T, N, H, p(G["gi"]), p(G["h0"]), p(reset), p(G["W"]), p(G["b"]), p(G["hp"]), p(G["h"]), p(G["gates"]), st), "gru fwd"),
            "lstm fwd": lambda k: ck(lib.bg_lstm_sequence_forward(T, N, H, p(L["gi"]), p(L["s0"][0]), p(L["s0"][1]), p(reset), p(L["W"]), p(L["b"]), p(L["hp"]), p(L["cp"]), p(L["h"]),
                                                                  p(L["c"]), p(L["gates"]), st), "lstm fwd"),
            "gru bwd": lambda k: ck(lib.bg_gru_sequence_backward(T, N, H, p(dh), p(G["gates"]), p(G["hp"]), p(reset), p(G["W"]), p(G["dgi"]), p(G["dgh"]), None, st), "gru bwd"),
            "lstm bwd": lambda k: ck(lib.bg_lstm_sequence_backward(T, N, H, p(dh), p(L["gates"]), p(L["cp"]), p(reset), p(L["W"]), p(L["dg"]), None, None, st), "lstm bwd"),
            "layers": lambda k: [ck(lib.bg_mlp_layer_forward(N, H, 4 * H, p(x), p(Wl), p(L["b"]), p(yl), 0, st), "bg_mlp_layer_forward") for _ in range(T)],
            "gru bias": lambda k: (ck(lib.bg_gru_bias_partial(B, H, p(G["dgi"]), p(G["dgh"]), p(rec_g), st), "gru bias"), reduce_group([fin_g])),
            "lstm bias": lambda k: (ck(lib.bg_lstm_bias_partial(B, H, p(L["dg"]), p(rec_l), st), "lstm bias"), reduce_group(fins_l)),
        }
        flops = 2.0 * T * N * H * 4 * H
        for q in range(pairs):
            us = {k: _best(f, 50 if "bias" in k else 20) for k, f in _orders(q, tuple(fns.items()))}
            say(f"recurrence, T = {T}, {N} envs, H = {H}: forward lstm {us['lstm fwd']:.1f} us, gru {us['gru fwd']:.1f} us ({us['lstm fwd'] / us['gru fwd']:.3f}); backward lstm "
                f"{us['lstm bwd']:.1f} us, gru {us['gru bwd']:.1f} us ({us['lstm bwd'] / us['gru bwd']:.3f}); the {T} bg_mlp_layer_forward({N}, {H}, {4 * H}) launches "
                f"{us['layers']:.1f} us; {flops / 1e9:.1f} GFLOP one way = {flops / PEAK_FP32_MFMA * 1e6:.1f} us at the fp32-MFMA peak")
            say(f"cell bias gradients, B = {B}, H = {H}: bg_lstm_bias_partial + its two finishes {us['lstm bias']:.1f} us ({B * 4 * H * 4 / 1e6:.0f} MB read), "
                f"bg_gru_bias_partial + its finish {us['gru bias']:.1f} us ({B * 6 * H * 4 / 1e6:.0f} MB read)")


def wide(pairs, N):
    """The LSTM's launches at H = 512 beside the same launches at H = 256 (a quarter of the FLOPs), the sides alternating."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.utils import reduce_group

    lib, p, st, B, ck = _lib.load(), _lib.ptr, _lib.current_stream_ptr(), T * N, _lib.check
    torch.manual_seed(1)
    obs, act = torch.randn(N, 47, device=DEV), torch.empty(N, 12, device=DEV)
    reset1, reset = (torch.rand(N, device=DEV) < 0.02).to(torch.uint8), (torch.rand(T, N, device=DEV) < 0.02).to(torch.uint8)
    z = lambda *s: torch.zeros(*s, device=DEV)
    r = lambda *s: torch.randn(*s, device=DEV)
    fns, keep = {}, []
    for H in (256, 512):
        m = ActorCritic(12, 47, 14, memory_hidden=H, memory_cell="lstm").to(DEV)
        d, s = (m.gru_descriptor(),) + _descs(m), z(2, N, H)
        L = dict(gi=r(B, 4 * H), W=r(4 * H, H) * H ** -0.5, b=r(4 * H) * 0.1, s0=r(2, N, H), hp=z(B, H), cp=z(B, H), h=z(B, H), c=z(B, H), gates=z(B, 5 * H), dg=z(B, 4 * H),
                 dh=r(B, H), x=r(N, H), Wl=r(4 * H, H), yl=z(N, 4 * H), rec=z((B + 127) // 128 * 4 * H), sums=[z(4 * H) for _ in range(2)])
        fins = []
        for sm in L["sums"]:
            f = _lib.ReduceProblem()
            f.partial, f.groups, f.record, f.n_out, f.out[0], f.n[0] = L["rec"].data_ptr(), (B + 127) // 128, 4 * H, 4 * H, sm.data_ptr(), 4 * H
            fins.append(f)
        keep.append((m, d, s, L, fins))
        fns[f"act {H}"] = lambda k, H=H, m=m, d=d, s=s: ck(lib.bg_actor_sample_lstm(N, p(obs), 47, d[0], d[2], d[1], p(m.logstd), 1, k, p(reset1), p(s[0]), p(s[0]), p(s[1]),
                                                                                      p(s[1]), None, p(act), st), "bg_actor_sample_lstm")
        fns[f"fwd {H}"] = lambda k, H=H, L=L: ck(lib.bg_lstm_sequence_forward(T, N, H, p(L["gi"]), p(L["s0"][0]), p(L["s0"][1]), p(reset), p(L["W"]), p(L["b"]), p(L["hp"]), p(L["cp"]),
                                                                               p(L["h"]), p(L["c"]), p(L["gates"]), st), "lstm fwd")
        fns[f"bwd {H}"] = lambda k, H=H, L=L: ck(lib.bg_lstm_sequence_backward(T, N, H, p(L["dh"]), p(L["gates"]), p(L["cp"]), p(reset), p(L["W"]), p(L["dg"]), None, None, st), "lstm bwd")
        fns[f"layers {H}"] = lambda k, H=H, L=L: [ck(lib.bg_mlp_layer_forward(N, H, 4 * H, p(L["x"]), p(L["Wl"]), p(L["b"]), p(L["yl"]), 0, st), "bg_mlp_layer_forward") for _ in range(T)]
        fns[f"bias {H}"] = lambda k, H=H, L=L, fins=fins: (ck(lib.bg_lstm_bias_partial(B, H, p(L["dg"]), p(L["rec"]), st), "lstm bias"), reduce_group(fins))
    for q in range(pairs):
        us = {k: _best(f, 200 if k.startswith("act") else 50 if k.startswith("bias") else 10) for k, f in _orders(q, tuple(fns.items()))}
        for what, k in (("rollout launch bg_actor_sample_lstm, trunk 256-128-128", "act"), (f"bg_lstm_sequence_forward, T = {T}", "fwd"),
                        (f"bg_lstm_sequence_backward, T = {T}", "bwd"), (f"bg_lstm_bias_partial + its two finishes, B = {B}", "bias"),
                        (f"the {T} bg_mlp_layer_forward({N}, H, 4H) launches a recurrence replaces", "layers")):
            say(f"{what}, {N} envs: H = 512 {us[k + ' 512']:.1f} us, H = 256 {us[k + ' 256']:.1f} us (512 / 256 = {us[k + ' 512'] / us[k + ' 256']:.2f})")
        for H in (256, 512):
            flops = 2.0 * T * N * H * 4 * H
            peak = flops / PEAK_FP32_MFMA * 1e6
            say(f"  H = {H}: {flops / 1e9:.1f} GFLOP one way = {peak:.0f} us at the fp32-MFMA peak; forward = {us[f'fwd {H}'] / peak:.2f}x, backward = {us[f'bwd {H}'] / peak:.2f}x that; "
                f"forward / layers = {us[f'fwd {H}'] / us[f'layers {H}']:.2f}, backward / layers = {us[f'bwd {H}'] / us[f'layers {H}']:.2f}")


def row_launch(pairs, N, K=234):
    """Every cell's _row launch at K inputs beside its 47-input launch and beside the feed-forward actor's launch on the same row, the sides alternating."""
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p, st, ck = _lib.load(), _lib.ptr, _lib.current_stream_ptr(), _lib.check
    torch.manual_seed(1)
    obs, row, act = torch.randn(N, 47, device=DEV), torch.randn(N, K, device=DEV), torch.empty(N, 12, device=DEV)
    reset = (torch.rand(N, device=DEV) < 0.02).to(torch.uint8)
    ff = ActorCritic(12, K, 14).to(DEV)
    fl, fn = _descs(ff)
    fns = {"mlp_scan": lambda k: ck(lib.bg_actor_sample_mlp_scan(N, p(row), fn, fl, K - 47, p(ff.logstd), 1, k, None, p(act), st), "bg_actor_sample_mlp_scan")}
    keep = []
    for cell, H in (("gru", 128), ("gru", 256), ("lstm", 128), ("lstm", 256), ("lstm", 512)):
        for x, kin, tail in ((obs, 47, ""), (row, K, "_row")):
            m = ActorCritic(12, kin, 14, memory_hidden=H, memory_cell=cell, memory_input=kin).to(DEV)
            d, s = (m.gru_descriptor(),) + _descs(m), torch.zeros(2, N, H, device=DEV)
            keep.append((m, d, s))
            states = (s[0], s[0], s[1], s[1]) if cell == "lstm" else (s[0], s[0])
            fns[f"{cell} {H}{tail}"] = lambda k, f=getattr(lib, f"bg_actor_sample_{cell}{tail}"), x=x, kin=kin, d=d, m=m, states=states: ck(
                f(N, p(x), kin, d[0], d[2], d[1], p(m.logstd), 1, k, p(reset), *[p(t) for t in states], None, p(act), st), "the cell's launch")
    for q in range(pairs):
        us = {k: _best(f, 200) for k, f in _orders(q, tuple(fns.items()))}
        for k in (k for k in fns if k.endswith("_row")):
            say(f"rollout launch, {N} rows, trunk 256-128-128, {k[:-4]}: bg_actor_sample_{k.split()[0]}_row at K = {K} {us[k]:.2f} us, the 47-input launch "
                f"{us[k[:-4]]:.2f} us (row / 47 = {us[k] / us[k[:-4]]:.3f}), bg_actor_sample_mlp_scan at K = {K} {us['mlp_scan']:.2f} us")


def loops(pairs, K, W, N, sides, base):
    got = {}
    for q in range(pairs):
        for k, (name, over) in _orders(q, tuple((k, SIDES[k]) for k in sides)):
            res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), str(K), str(W), "1", str(N), os.devnull, f"one:{k}"],
                                 capture_output=True, text=True, check=True)
            for line in res.stdout.splitlines():
                if line.startswith("training loop"):
                    say(line)
                elif line.startswith("MS "):
                    got.setdefault(name, []).append(float(line[3:]))
    for name, ms in got.items():
        say(f"  {name}: {min(ms):.3f} to {max(ms):.3f} ms per iteration, best = {min(ms) / min(got[base]):.3f}x the best of {base}")


if __name__ == "__main__":
    a = sys.argv[1:]
    K, W, pairs, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((20, 5, 3, 4096)))
    only = a[5] if len(a) > 5 else ""
    name = "rnn_input_time.txt" if only.startswith("row") else "lstm_512_time.txt" if only.startswith("wide") else "lstm_time.txt"
    out = a[4] if len(a) > 4 and a[4] != "-" else os.path.join(ROOT, "profiles", name)
    if only.startswith("one:"):  # a child of the loop section: one Runner in a process of its own
        name, over = SIDES[int(only[4:])]
        print("MS %.6f" % loop(name, over, K, W, N), flush=True)
        sys.exit(0)
    say(f"tools/lstm_time.py {' '.join(a) or f'{K} {W} {pairs} {N}'} on {torch.cuda.get_device_name(0)}")
    if only.startswith("row"):
        if only != "row_loop":
            row_launch(pairs, N)
        if only != "row_kernels":
            loops(pairs, K, W, N, (4, 5), "lstm 256, critic scan")
    elif only.startswith("wide"):
        if only != "wide_loop":
            wide(pairs, N)
        if only != "wide_kernels":
            loops(pairs, K, W, N, (2, 3), "lstm 256")
    else:
        if only != "loop":
            rollout_launch(pairs, N)
            recurrences(pairs, N)
        if only != "kernels":
            loops(pairs, K, W, N, (0, 1), "rnn_cell gru")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
