"""Timing of the teacher-student distillation (README "Distillation"); writes profiles/distill_time.txt.

  python tools/distill_time.py [K=20] [W=5] [pairs=3] [num_envs=4096] [out=profiles/distill_time.txt] [Hs] [only]
      (1) the rollout's launch, bg_distill_act, against the sum of its stand-alone launches on the same rows (bg_actor_sample_mlp_scan on the whole
          row, bg_actor_sample_mlp on a contiguous copy of the prefix columns, and that copy), HIP events around 200 back-to-back calls, best of 5,
          alternating, at H = 1 / P = 187 and at H = 3 / P = 45: us per env step's inference, both networks 256-128-128;
      (2) bg_distill_head against bg_actor_head mode 1 at B = 98,304 rows, the same way: us per launch pair (kernel + fixed-order finish);
      (3) the distillation loop (rollout of 24 steps + 5 epochs, no instrumentation) at H = 1 / P = 187 with a seeded teacher: W warm-up iterations,
          then runs of K iterations: ms per iteration, iterations per second.
  With Hs (distillation.student_frame_stack; out "-" = profiles/distill_history_time.txt) the sections are those of the longer history instead, all at
  H = 1 / P = 187:
      (4) the env step (bg_env_step_to, whose last launch is bg_obs_assemble) with the student's row [47 Hs] against the same env without it, HIP
          events around 200 back-to-back steps, best of 5, alternating, and the bytes bg_obs_assemble writes in each; `only` = "assemble" stops
          here (the run under a kernel trace, which gives the launch's own time);
      (5) bg_distill_act_hist on a buffer of the student's own against bg_distill_act at Hs = H (same networks, expected equal), and at Hs;
      (6) the loop of (3) with the key absent and with it, one Distiller after the other, `pairs` times each.
  With symmetric_coef=C and / or teacher_action_prob=BETA anywhere among the arguments (distillation.symmetric_coef / teacher_action_prob; out "-" =
  profiles/distill_symmetry_dagger_time.txt; each defaults to 10 / 0.5 when only the other is given) the sections are those of the two keys instead:
      (7) bg_distill_act_mix at beta = 0, 0.5 and 1 against bg_distill_act on the same rows at H = 1 / P = 187, and with Hs (5 unless given) against
          bg_distill_act_hist, the same way as (1);
      (8) bg_distill_head_sym at B = 98,304 (2B rows) against bg_distill_head at B and at 2B rows and against bg_actor_head_sym at B, and the bytes
          it moves as a fraction of the float4-copy rate;
      (9) the loop of (3) with neither key, with the loss, with the mixing, and with both, one Distiller after the other, `pairs` times each.
          `only` = "head" runs (8) alone, "loop" (9) alone.
  With student_memory=H among the arguments (distillation.student_memory; out "-" = profiles/distill_memory_time.txt) the sections are the recurrent
  student's instead, all at H = 1 / P = 187:
      (10) bg_distill_act_gru with a cell of 128 and of 256 against bg_distill_act (a memoryless student) and bg_distill_act_hist at Hs (5 unless
           given), the same way as (1);
      (11) bg_gru_sequence_forward / _backward at T = 24 on num_envs rows against 24 launches of bg_mlp_layer_forward(num_envs, H, 3H), the per-step
           form of the h-side GEMM they replace, and against their own fp32-MFMA time from the flop count (157.3 TFLOPS);
      (12) the loop of (3) with a memoryless student, with Hs, and with the cell of H, one Distiller after the other, `pairs` times each.
  With student_sensors=full (or =empty: a section with nothing configured) among the arguments (distillation.student_sensors; out "-" =
  profiles/student_sensors_time.txt) the sections are the student's sensor model's instead, all at H = 1 / P = 187:
      (13) the env step (bg_env_step_to, whose last launch is bg_obs_assemble) with the key (full bias and latency_steps [0, 1.5] for "full") against
           the same env without it, at Hs (5 unless given) and at Hs = H = 1 (without the key: no student's row at all), the way of (4), and the bytes
           bg_obs_assemble moves in each; `only` = "assemble" stops here (the run under a kernel trace, which gives the launch's own time);
      (14) the loop of (3) without the key and with it, at Hs = H and at Hs, one Distiller after the other, `pairs` times each.
  The outputs of (1) are compared bit for bit before they are timed.  The committed profile carries two more sections that this tool does not
  write: the figures tests/test_gpu_distill.py prints under -s, and bench.py of this tree against a checkout of its parent commit."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

DEV = "cuda:0"
GRID_9x5 = {"terrain.measured_points_x": [round(-0.4 + 0.1 * i, 1) for i in range(9)], "terrain.measured_points_y": [-0.2, -0.1, 0.0, 0.1, 0.2]}
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


def act(pairs=3, N=4096):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p = _lib.load(), _lib.ptr
    for H, P in ((1, 187), (3, 45)):
        torch.manual_seed(H)
        F = 47 * H
        teacher, student = ActorCritic(12, F + P, 14 + P).to(DEV), ActorCritic(12, F, 14 + P).to(DEV)
        obs, prefix = torch.randn(N, F + P, device=DEV), torch.empty(N, F, device=DEV)
        (sd, ns), (td, nt) = _descs(student), _descs(teacher)
        a1, t1, a2, t2, tmp = (torch.empty(N, 12, device=DEV) for _ in range(5))
        st = _lib.current_stream_ptr()

        def fused(k):
            _lib.check(lib.bg_distill_act(N, p(obs), F + P, ns, sd, nt, td, P, p(student.logstd), 1, k, None, p(a1), p(t1), st), "bg_distill_act")

        def separate(k):
            _lib.check(lib.bg_actor_sample_mlp_scan(N, p(obs), nt, td, P, p(teacher.logstd), 1, k, p(t2), p(tmp), st), "bg_actor_sample_mlp_scan")
            prefix.copy_(obs[:, :F])
            _lib.check(lib.bg_actor_sample_mlp(N, p(prefix), ns, sd, p(student.logstd), 1, k, None, p(a2), st), "bg_actor_sample_mlp")

        fused(7); separate(7); torch.cuda.synchronize()
        assert torch.equal(a1, a2) and torch.equal(t1, t2), "bg_distill_act differs from its stand-alone launches"
        for q in range(pairs):
            us = {m: _best(f, 200) for m, f in _orders(q, (("fused", fused), ("separate", separate)))}
            say(f"rollout inference, {N} rows, H = {H}, P = {P}, both 256-128-128: bg_distill_act {us['fused']:.2f} us, bg_actor_sample_mlp_scan + prefix copy + "
                f"bg_actor_sample_mlp {us['separate']:.2f} us, fused / separate = {us['fused'] / us['separate']:.4f}")


def head(pairs=3, B=98304):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.utils import actor_head_loss_backward, head_scratch

    g = torch.Generator(device="cpu").manual_seed(0)
    A = 12
    h = torch.nn.functional.elu(torch.randn(B, 128, generator=g)).to(DEV)
    W, b = (torch.randn(A, 128, generator=g) * 0.1).to(DEV), (torch.randn(A, generator=g) * 0.1).to(DEV)
    target = torch.randn(B, A, generator=g).to(DEV)
    logstd = torch.full((A,), -2.0, device=DEV)
    old_mu = h @ W.t() + b + 0.02 * torch.randn(B, A, generator=g).to(DEV)
    actions = old_mu + 0.135 * torch.randn(B, A, generator=g).to(DEV)
    old_logp = (-0.5 * ((actions - old_mu) / logstd.exp()) ** 2 - logstd - 0.9189385332046727).sum(-1)
    adv = torch.randn(B, generator=g).to(DEV)
    adv_stats = torch.stack([adv.double().sum(), (adv.double() ** 2).sum(), torch.tensor(float(B), dtype=torch.float64, device=DEV)])
    gh, dW, db, dbh = torch.empty(B, 128, device=DEV), torch.empty(A, 128, device=DEV), torch.empty(A, device=DEV), torch.empty(128, device=DEV)
    gls, st5, st1, scr = torch.zeros(A, dtype=torch.float64, device=DEV), torch.zeros(5, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV), head_scratch(DEV)
    lib, p = _lib.load(), _lib.ptr

    def distill(k):
        _lib.check(lib.bg_distill_head(B, p(h), p(W), p(b), p(target), None, p(gh), p(dW), p(db), p(dbh), p(st1), p(scr), _lib.current_stream_ptr()), "bg_distill_head")

    def actor(k):
        actor_head_loss_backward(h, W, b, logstd, actions, old_mu, logstd, old_logp, adv, adv_stats, 0.2, 1.0, -0.01, gh, dW, db, dbh, gls, st5, scr)

    for q in range(pairs):
        us = {m: _best(f, 100) for m, f in _orders(q, (("distill", distill), ("actor", actor)))}
        # the kernel reads h [B][128] and target [B][12] and writes g_hidden [B][128]
        gbs = B * (128 * 2 + 12) * 4 / (us["distill"] * 1e-6) / 1e9
        say(f"loss head, B = {B}: bg_distill_head {us['distill']:.2f} us ({gbs:.0f} GB/s of h + target read, g_hidden written, finish launch included), bg_actor_head mode 1 "
            f"{us['actor']:.2f} us, distill / actor = {us['distill'] / us['actor']:.4f}")


def assemble(pairs=3, N=4096, Hs=5, P=187):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 + P, "env.num_privileged_obs": 14 + P}
    envs = {"with": T1(load_cfg("T1", dict(ov, **{"env.student_frame_stack": Hs}))), "without": T1(load_cfg("T1", ov))}
    g = torch.Generator(device="cpu").manual_seed(0)
    a = ((torch.rand(N, 12, generator=g) * 2 - 1) * 0.3).to(DEV)
    obs, priv, sob = torch.empty(N, 47 + P, device=DEV), torch.empty(N, 14 + P, device=DEV), torch.empty(N, 47 * Hs, device=DEV)
    rew, done, tout = torch.empty(N, device=DEV), torch.empty(N, dtype=torch.bool, device=DEV), torch.empty(N, dtype=torch.bool, device=DEV)
    for e in envs.values():
        e.reset()
    fns = {"with": lambda k: envs["with"].step_to(a, obs, priv, rew, done, tout, student_obs=sob),
           "without": lambda k: envs["without"].step_to(a, obs, priv, rew, done, tout)}
    for f in fns.values():
        for k in range(20):
            f(k)
    torch.cuda.synchronize()
    # what bg_obs_assemble writes: the actor's row [47 H + P] and the critic's P clean scan columns; with the key the student's row [47 Hs] as well
    w0 = N * (47 + P + P) * 4
    w1 = w0 + N * 47 * Hs * 4
    say(f"bg_obs_assemble, {N} envs, H = 1, P = {P}: writes {w0 / 1e6:.3f} MB without the student's row, {w1 / 1e6:.3f} MB with Hs = {Hs} "
        f"(+{(w1 - w0) / 1e6:.3f} MB, x{w1 / w0:.3f}); ring reads {N * 47 * 4 / 1e6:.3f} MB against {N * 47 * (Hs + 1) * 4 / 1e6:.3f} MB")
    for q in range(pairs):
        us = {m: _best(fns[m], 200) for m in _orders(q, ("with", "without"))}
        say(f"env step (bg_env_step_to, all launches), {N} envs: with the student's row {us['with']:.2f} us, without {us['without']:.2f} us, "
            f"difference {us['with'] - us['without']:+.2f} us, with / without = {us['with'] / us['without']:.4f}")


FULL_SENSORS = {"bias": {"gravity": {"range": [0.0, 0.05], "operation": "additive", "distribution": "gaussian"},
                         "ang_vel": {"range": [-0.2, 0.2], "operation": "additive", "distribution": "uniform"},
                         "dof_pos": {"range": [0.01, 0.03], "operation": "additive", "distribution": "gaussian"},
                         "dof_vel": {"range": [-0.5, 0.3], "operation": "additive", "distribution": "uniform"}}, "latency_steps": [0.0, 1.5]}


def assemble_sensors(pairs=3, N=4096, Hs=5, P=187, sensors=None):
    """(13): the env step with distillation.student_sensors (as the Distiller hands it over: env.student_frame_stack and env.student_sensors)."""
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N, "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 47 + P, "env.num_privileged_obs": 14 + P}
    g = torch.Generator(device="cpu").manual_seed(0)
    a = ((torch.rand(N, 12, generator=g) * 2 - 1) * 0.3).to(DEV)
    obs, priv = torch.empty(N, 47 + P, device=DEV), torch.empty(N, 14 + P, device=DEV)
    rew, done, tout = torch.empty(N, device=DEV), torch.empty(N, dtype=torch.bool, device=DEV), torch.empty(N, dtype=torch.bool, device=DEV)
    lat_hi = float(sensors.get("latency_steps", [0.0, 0.0])[1])
    for hs in (Hs, 1):
        sob = torch.empty(N, 47 * hs, device=DEV)
        envs = {"with": T1(load_cfg("T1", dict(ov, **{"env.student_frame_stack": hs, "env.student_sensors": sensors}))),
                "without": T1(load_cfg("T1", dict(ov, **({"env.student_frame_stack": hs} if hs > 1 else {}))))}
        for e in envs.values():
            e.reset()
        fns = {"with": lambda k: envs["with"].step_to(a, obs, priv, rew, done, tout, student_obs=sob),
               "without": (lambda k: envs["without"].step_to(a, obs, priv, rew, done, tout, student_obs=sob)) if hs > 1 else
                          (lambda k: envs["without"].step_to(a, obs, priv, rew, done, tout))}
        for f in fns.values():
            for k in range(20):
                f(k)
        torch.cuda.synchronize()
        # writes: the actor's row [47 + P], the critic's P clean scan columns, the student's row [47 hs] (bias and latency only on a reset);
        # reads: the ring for the teacher's frame and for the student's frames, with the key a second plane for the 30 sensor columns of every frame
        # where the latency has a fraction, the env's 30 biases once and its reset flag, age and latency
        w0 = N * (47 + P + P) * 4 + (N * 47 * hs * 4 if hs > 1 else 0)
        r0 = N * 47 * 4 + (N * 47 * hs * 4 if hs > 1 else 0)
        w1, r1 = N * (47 + P + P) * 4 + N * 47 * hs * 4, N * 47 * 4 + N * 47 * hs * 4 + (N * 30 * hs * 4 if lat_hi > 0 else 0) + N * 30 * 4 + N * 9
        say(f"bg_obs_assemble, {N} envs, H = 1, P = {P}, Hs = {hs}: without the key {'(no student row) ' if hs == 1 else ''}writes {w0 / 1e6:.3f} MB + ring reads "
            f"{r0 / 1e6:.3f} MB = {(w0 + r0) / 1e6:.3f} MB; with it writes {w1 / 1e6:.3f} MB + reads {r1 / 1e6:.3f} MB = {(w1 + r1) / 1e6:.3f} MB "
            f"(= {(w1 + r1) / 6.29e12 * 1e6:.3f} us at the float4-copy rate of 6.29 TB/s)")
        for q in range(pairs):
            us = {m: _best(fns[m], 200) for m in _orders(q, ("with", "without"))}
            say(f"env step (bg_env_step_to, all launches), {N} envs, Hs = {hs}: with student_sensors {us['with']:.2f} us, without {us['without']:.2f} us, "
                f"difference {us['with'] - us['without']:+.2f} us, with / without = {us['with'] / us['without']:.4f}")
        del envs, fns


def act_hist(pairs=3, N=4096, Hs=5, P=187):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p = _lib.load(), _lib.ptr
    torch.manual_seed(1)
    teacher = ActorCritic(12, 47 + P, 14 + P).to(DEV)
    obs = torch.randn(N, 47 + P, device=DEV)
    (td, nt), st = _descs(teacher), _lib.current_stream_ptr()
    for hs in (1, Hs):
        student = ActorCritic(12, 47 * hs, 14 + P).to(DEV)
        sobs = torch.randn(N, 47 * hs, device=DEV)
        sobs[:, -47:] = obs[:, :47]
        (sd, ns) = _descs(student)
        a1, t1, a2, t2 = (torch.empty(N, 12, device=DEV) for _ in range(4))

        def hist(k):
            _lib.check(lib.bg_distill_act_hist(N, p(obs), 47 + P, p(sobs), 47 * hs, ns, sd, nt, td, P, p(student.logstd), 1, k, None, p(a1), p(t1), st), "bg_distill_act_hist")

        def plain(k):
            _lib.check(lib.bg_distill_act(N, p(obs), 47 + P, ns, sd, nt, td, P, p(student.logstd), 1, k, None, p(a2), p(t2), st), "bg_distill_act")

        if hs == 1:
            hist(7); plain(7); torch.cuda.synchronize()
            assert torch.equal(a1, a2) and torch.equal(t1, t2), "bg_distill_act_hist differs from bg_distill_act at Hs = H"
        for q in range(pairs):
            if hs == 1:
                us = {m: _best(f, 200) for m, f in _orders(q, (("hist", hist), ("plain", plain)))}
                say(f"rollout inference, {N} rows, H = 1, P = {P}, both 256-128-128, Hs = H: bg_distill_act_hist (student on its own [47] buffer) {us['hist']:.2f} us, "
                    f"bg_distill_act {us['plain']:.2f} us, hist / plain = {us['hist'] / us['plain']:.4f}")
            else:
                say(f"rollout inference, {N} rows, H = 1, P = {P}, both 256-128-128, Hs = {hs} ({47 * hs} student columns): bg_distill_act_hist {_best(hist, 200):.2f} us")


def act_mix(pairs=3, N=4096, Hs=5, P=187):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p = _lib.load(), _lib.ptr
    torch.manual_seed(1)
    teacher = ActorCritic(12, 47 + P, 14 + P).to(DEV)
    obs = torch.randn(N, 47 + P, device=DEV)
    (td, nt), st = _descs(teacher), _lib.current_stream_ptr()
    for hs in (1, Hs):
        student = ActorCritic(12, 47 * hs, 14 + P).to(DEV)
        sobs = obs if hs == 1 else torch.randn(N, 47 * hs, device=DEV)
        (sd, ns) = _descs(student)
        a1, t1, a2, t2 = (torch.empty(N, 12, device=DEV) for _ in range(4))
        base = "bg_distill_act" if hs == 1 else "bg_distill_act_hist"

        def plain(k):
            if hs == 1:
                _lib.check(lib.bg_distill_act(N, p(obs), 47 + P, ns, sd, nt, td, P, p(student.logstd), 1, k, None, p(a2), p(t2), st), base)
            else:
                _lib.check(lib.bg_distill_act_hist(N, p(obs), 47 + P, p(sobs), 47 * hs, ns, sd, nt, td, P, p(student.logstd), 1, k, None, p(a2), p(t2), st), base)

        def mix(beta):
            return lambda k: _lib.check(lib.bg_distill_act_mix(N, p(obs), 47 + P, p(sobs), sobs.shape[1], ns, sd, nt, td, P, p(student.logstd), 1, k, beta, 1, None, p(a1),
                                                               p(t1), st), "bg_distill_act_mix")

        mix(0.0)(7); plain(7); torch.cuda.synchronize()
        assert torch.equal(a1, a2) and torch.equal(t1, t2), f"bg_distill_act_mix at beta = 0 differs from {base}"
        fns = (("plain", plain), ("mix 0", mix(0.0)), ("mix 0.5", mix(0.5)), ("mix 1", mix(1.0)))
        for q in range(pairs):
            us = {m: _best(f, 200) for m, f in _orders(q, fns)}
            say(f"rollout inference, {N} rows, H = 1, P = {P}, both 256-128-128, student columns {47 * hs}: {base} {us['plain']:.2f} us, bg_distill_act_mix beta = 0 "
                f"{us['mix 0']:.2f} us ({us['mix 0'] / us['plain']:.4f}x), beta = 0.5 {us['mix 0.5']:.2f} us ({us['mix 0.5'] / us['plain']:.4f}x), beta = 1 "
                f"{us['mix 1']:.2f} us ({us['mix 1'] / us['plain']:.4f}x)")


def head_sym(pairs=3, B=98304, coef=10.0):
    import json

    from booster_gym_amd import _lib
    from booster_gym_amd.envs.mirror import mirror_maps
    from booster_gym_amd.utils.utils import actor_head_sym_loss_backward, head_scratch

    m = json.load(open(os.path.join(ROOT, "booster_gym_amd", "resources", "T1", "T1_locomotion.flat.json")))
    _, _, act_src, act_sign = mirror_maps(m["dof_names"], [a for a in m["joint_axis"] if a], [-0.2, 0, 0, 0.4, -0.25, 0] * 2, 47)
    import ctypes

    src, sign = (ctypes.c_int32 * 12)(*[int(v) for v in act_src]), (ctypes.c_float * 12)(*[float(v) for v in act_sign])
    g = torch.Generator(device="cpu").manual_seed(0)
    A = 12
    h = torch.nn.functional.elu(torch.randn(2 * B, 128, generator=g)).to(DEV)
    W, b = (torch.randn(A, 128, generator=g) * 0.1).to(DEV), (torch.randn(A, generator=g) * 0.1).to(DEV)
    target = torch.randn(2 * B, A, generator=g).to(DEV)
    logstd = torch.full((A,), -2.0, device=DEV)
    old_mu = h[:B] @ W.t() + b + 0.02 * torch.randn(B, A, generator=g).to(DEV)
    actions = old_mu + 0.135 * torch.randn(B, A, generator=g).to(DEV)
    old_logp = (-0.5 * ((actions - old_mu) / logstd.exp()) ** 2 - logstd - 0.9189385332046727).sum(-1)
    adv = torch.randn(B, generator=g).to(DEV)
    adv_stats = torch.stack([adv.double().sum(), (adv.double() ** 2).sum(), torch.tensor(float(B), dtype=torch.float64, device=DEV)])
    gh, dW, db, dbh = torch.empty(2 * B, 128, device=DEV), torch.empty(A, 128, device=DEV), torch.empty(A, device=DEV), torch.empty(128, device=DEV)
    gls, st6, st2, scr = torch.zeros(A, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV), head_scratch(DEV)
    lib, p = _lib.load(), _lib.ptr

    def sym(k):
        _lib.check(lib.bg_distill_head_sym(B, p(h), p(W), p(b), p(target), coef, src, sign, None, p(gh), p(dW), p(db), p(dbh), p(st2), p(scr), _lib.current_stream_ptr()),
                   "bg_distill_head_sym")

    def plain(rows):
        return lambda k: _lib.check(lib.bg_distill_head(rows, p(h), p(W), p(b), p(target), None, p(gh), p(dW), p(db), p(dbh), p(st2), p(scr), _lib.current_stream_ptr()),
                                    "bg_distill_head")

    def actor_sym(k):
        actor_head_sym_loss_backward(h, W, b, logstd, actions, old_mu, logstd, old_logp, adv, adv_stats, 0.2, 1.0, -0.01, coef, (act_src, act_sign), gh, dW, db, dbh, gls,
                                     st6, scr)

    fns = (("sym", sym), ("plain B", plain(B)), ("plain 2B", plain(2 * B)), ("actor sym", actor_sym))
    for q in range(pairs):
        us = {m: _best(f, 100) for m, f in _orders(q, fns)}
        # the kernel reads h [2B][128] and target [B][12] and writes g_hidden [2B][128]
        nbytes = (2 * B * 128 * 2 + B * 12) * 4
        tbs = nbytes / (us["sym"] * 1e-6) / 1e12
        say(f"loss head, B = {B}: bg_distill_head_sym (2B rows) {us['sym']:.2f} us ({nbytes / 1e6:.1f} MB of h + target read and g_hidden written = {tbs:.2f} TB/s, "
            f"{100 * tbs / 6.29:.0f} % of the 6.29 TB/s of a float4 copy; finish launch included), bg_distill_head at B rows {us['plain B']:.2f} us "
            f"(sym / plain = {us['sym'] / us['plain B']:.4f}), at 2B rows {us['plain 2B']:.2f} us (sym / plain = {us['sym'] / us['plain 2B']:.4f}), "
            f"bg_actor_head_sym at B {us['actor sym']:.2f} us (distill sym / actor sym = {us['sym'] / us['actor sym']:.4f})")


def act_gru(pairs=3, N=4096, Hs=5, P=187):
    from booster_gym_amd import _lib
    from booster_gym_amd.utils.model import ActorCritic

    lib, p = _lib.load(), _lib.ptr
    torch.manual_seed(1)
    teacher = ActorCritic(12, 47 + P, 14 + P).to(DEV)
    obs, sobs = torch.randn(N, 47 + P, device=DEV), torch.randn(N, 47 * Hs, device=DEV)
    plain_s, hist_s = ActorCritic(12, 47, 14 + P).to(DEV), ActorCritic(12, 47 * Hs, 14 + P).to(DEV)
    gru_s = {H: ActorCritic(12, 47, 14 + P, memory_hidden=H).to(DEV) for H in (128, 256)}
    state = {H: torch.zeros(N, H, device=DEV) for H in gru_s}
    (td, nt), st = _descs(teacher), _lib.current_stream_ptr()
    (pd, npl), (hd, nh) = _descs(plain_s), _descs(hist_s)
    gd = {H: (m.gru_descriptor(),) + _descs(m) for H, m in gru_s.items()}
    a1, t1 = (torch.empty(N, 12, device=DEV) for _ in range(2))

    def plain(k):
        _lib.check(lib.bg_distill_act(N, p(obs), 47 + P, npl, pd, nt, td, P, p(plain_s.logstd), 1, k, None, p(a1), p(t1), st), "bg_distill_act")

    def hist(k):
        _lib.check(lib.bg_distill_act_hist(N, p(obs), 47 + P, p(sobs), 47 * Hs, nh, hd, nt, td, P, p(hist_s.logstd), 1, k, None, p(a1), p(t1), st), "bg_distill_act_hist")

    def gru(H):
        g, sd, ns = gd[H]
        return lambda k: _lib.check(lib.bg_distill_act_gru(N, p(obs), 47 + P, nt, td, P, g, ns, sd, p(gru_s[H].logstd), 1, k, 0.0, 1, None, p(state[H]), p(state[H]), None,
                                                           p(a1), p(t1), st), "bg_distill_act_gru")

    fns = (("plain", plain), ("hist", hist), ("gru 128", gru(128)), ("gru 256", gru(256)))
    for q in range(pairs):
        us = {m: _best(f, 200) for m, f in _orders(q, fns)}
        say(f"rollout inference, {N} rows, H = 1, P = {P}, teacher and trunks 256-128-128: bg_distill_act (memoryless, 47 columns) {us['plain']:.2f} us, "
            f"bg_distill_act_hist at Hs = {Hs} {us['hist']:.2f} us, bg_distill_act_gru with a cell of 128 {us['gru 128']:.2f} us ({us['gru 128'] / us['plain']:.3f}x plain, "
            f"{us['gru 128'] / us['hist']:.3f}x hist), of 256 {us['gru 256']:.2f} us ({us['gru 256'] / us['plain']:.3f}x plain, {us['gru 256'] / us['hist']:.3f}x hist)")


def sequence(pairs=3, N=4096, T=24):
    from booster_gym_amd import _lib

    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream_ptr()
    for H in (128, 256):
        torch.manual_seed(H)
        cell = torch.nn.GRUCell(47, H).to(DEV)
        B = T * N
        gi, dh = torch.randn(B, 3 * H, device=DEV), torch.randn(B, H, device=DEV)
        h0, reset = torch.zeros(N, H, device=DEV), (torch.rand(T, N, device=DEV) < 0.02).to(torch.uint8)
        h_prev, h, gates = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV), torch.empty(B, 4 * H, device=DEV)
        dgi, dgh, gh = torch.empty(B, 3 * H, device=DEV), torch.empty(B, 3 * H, device=DEV), torch.empty(N, 3 * H, device=DEV)

        def fwd(k):
            _lib.check(lib.bg_gru_sequence_forward(T, N, H, p(gi), p(h0), p(reset), p(cell.weight_hh), p(cell.bias_hh), p(h_prev), p(h), p(gates), st), "bg_gru_sequence_forward")

        def bwd(k):
            _lib.check(lib.bg_gru_sequence_backward(T, N, H, p(dh), p(gates), p(h_prev), p(reset), p(cell.weight_hh), p(dgi), p(dgh), None, st), "bg_gru_sequence_backward")

        def steps(k):
            for t in range(T):
                _lib.check(lib.bg_mlp_layer_forward(N, H, 3 * H, p(h[t * N :]), p(cell.weight_hh), p(cell.bias_hh), p(gh), 0, st), "bg_mlp_layer_forward")

        fwd(0); torch.cuda.synchronize()
        floor = 2.0 * B * H * 3 * H / 157.3e12 * 1e6  # us of the h-side GEMM (forward) = of the carry's GEMM (backward) at the fp32 matrix rate
        for q in range(pairs):
            us = {m: _best(f, 20) for m, f in _orders(q, (("fwd", fwd), ("bwd", bwd), ("steps", steps)))}
            say(f"recurrence, T = {T}, {N} envs, H = {H}: bg_gru_sequence_forward {us['fwd']:.1f} us, bg_gru_sequence_backward {us['bwd']:.1f} us, {T} launches of "
                f"bg_mlp_layer_forward({N}, {H}, {3 * H}) {us['steps']:.1f} us (forward / per-step GEMMs = {us['fwd'] / us['steps']:.3f}); fp32-MFMA time of the "
                f"{2.0 * B * H * 3 * H / 1e9:.1f} GFLOP {floor:.1f} us (forward {us['fwd'] / floor:.1f}x, backward {us['bwd'] / floor:.1f}x)")


def loop(K=20, W=5, pairs=3, N=4096, Hs=None, coef=0.0, beta=0.0, memory=0, student_sensors=None):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.distill import Distiller
    from booster_gym_amd.utils.model import ActorCritic
    from booster_gym_amd.utils.recorder import Recorder
    from booster_gym_amd.utils.terrain import height_scan_points

    tmp = tempfile.mkdtemp(prefix="bg_distill_")
    cfg = load_cfg("T1", {"env.num_envs": N, "terrain.measure_heights": True, "terrain.actor_heights": True, "env.num_observations": 234, "env.num_privileged_obs": 201})
    cfg["runner"]["save_interval"] = 10 ** 9  # no checkpoint inside the timed region
    torch.manual_seed(0)
    ck = os.path.join(tmp, "teacher.pth")
    torch.save({"model": ActorCritic(12, 234, 201).state_dict(), "height_points": torch.tensor(height_scan_points(cfg["terrain"])[1], dtype=torch.float).reshape(-1, 2)}, ck)
    cfg["distillation"]["teacher_checkpoint"] = ck
    if Hs:
        cfg["distillation"]["student_frame_stack"] = Hs
    if coef:
        cfg["distillation"]["symmetric_coef"] = coef
    if beta:
        cfg["distillation"]["teacher_action_prob"] = beta
    if memory:
        cfg["distillation"]["student_memory"] = memory
    if student_sensors is not None:
        cfg["distillation"]["student_sensors"] = student_sensors
    d = Distiller(cfg=cfg)
    d.begin(Recorder(cfg, root=tmp, rank=0))
    it = 0

    def run(n):
        nonlocal it
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            d.train_iteration(it); it += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    run(W)
    T, E = cfg["runner"]["horizon_length"], d.dcfg.num_epochs
    for q in range(pairs):
        ms = run(K)
        keys = f"symmetric_coef {coef:g}, teacher_action_prob {beta:g}, " if coef or beta or KEYS else ""
        keys += f"student_memory {memory}, " if memory or MEMORY else ""
        keys += f"student_sensors {'absent' if student_sensors is None else SENSORS[0]}, " if SENSORS else ""
        say(f"distillation loop, {N} envs, H = 1, P = 187, {keys}student_frame_stack {Hs or 'absent'} ({d.student_obs} student columns padded to {d._student_in.shape[1]}), horizon {T}, {E} epochs, student 256-128-128 (plan {d._sup.mlp.plan.fwd} / {d._sup.mlp.plan.bwd}, weight "
            f"gradients {d._sup.wgrad_terms or 'fp32'}): {ms:.3f} ms per iteration = {1e3 / ms:.2f} iterations/s = {N * T / ms / 1e3:.3f} M env-steps/s; last loss "
            f"{d.last_loss:.6f}")
    for ph, fn in (("rollout", d.rollout), ("update", d.update)):
        best = 1e9
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        say(f"  {ph} alone: {best:.3f} ms (best of 3)")


KEYS = {}  # symmetric_coef / teacher_action_prob given on the command line: sections (7) to (9)
MEMORY = []  # student_memory given on the command line: sections (10) to (12)
SENSORS = []  # student_sensors given on the command line ("full" or "empty"): sections (13) and (14)


if __name__ == "__main__":
    KEYS.update({k: float(v) for k, v in (x.split("=", 1) for x in sys.argv[1:] if "=" in x) if k in ("symmetric_coef", "teacher_action_prob")})
    MEMORY.extend(int(v) for k, v in (x.split("=", 1) for x in sys.argv[1:] if "=" in x) if k == "student_memory")
    SENSORS.extend(v for k, v in (x.split("=", 1) for x in sys.argv[1:] if "=" in x) if k == "student_sensors")
    a = [x for x in sys.argv[1:] if "=" not in x]
    K, W, pairs, N = (int(a[i]) if len(a) > i else v for i, v in enumerate((20, 5, 3, 4096)))
    Hs, only = (int(a[5]) if len(a) > 5 else 0), (a[6] if len(a) > 6 else "")
    name = "student_sensors_time.txt" if SENSORS else "distill_memory_time.txt" if MEMORY else "distill_symmetry_dagger_time.txt" if KEYS else "distill_history_time.txt" if Hs else "distill_time.txt"
    out = a[4] if len(a) > 4 and a[4] != "-" else os.path.join(ROOT, "profiles", name)
    say(f"tools/distill_time.py {' '.join(sys.argv[1:]) or f'{K} {W} {pairs} {N}'} on {torch.cuda.get_device_name(0)}")
    if SENSORS:
        if SENSORS[0] not in ("full", "empty"):
            raise SystemExit("student_sensors=full or student_sensors=empty")
        section = FULL_SENSORS if SENSORS[0] == "full" else {}
        if only != "loop":
            assemble_sensors(pairs, N, Hs or 5, sensors=section)
        for q in range(pairs if only != "assemble" else 0):  # (a Distiller each: the env and the buffers are per configuration)
            for hs, sec in _orders(q, ((None, None), (None, section), (Hs or 5, None), (Hs or 5, section))):
                loop(K, W, 1, N, hs, student_sensors=sec)
    elif MEMORY:
        if only != "loop":
            act_gru(pairs, N, Hs or 5)
            sequence(pairs, N)
        for q in range(pairs):  # (a Distiller each: the env, the buffers and the plan are per configuration)
            for hs, mem in _orders(q, ((None, 0), (Hs or 5, 0), (None, MEMORY[0]))):
                loop(K, W, 1, N, hs, memory=mem)
    elif KEYS:
        coef, beta = KEYS.get("symmetric_coef", 10.0), KEYS.get("teacher_action_prob", 0.5)
        if only not in ("loop", "head"):
            act_mix(pairs, N, Hs or 5)
        if only != "loop":
            head_sym(pairs, coef=coef)
        for q in range(pairs if only != "head" else 0):  # (a Distiller each: the buffers and the plan are per configuration)
            for c, bt in _orders(q, ((0.0, 0.0), (coef, 0.0), (0.0, beta), (coef, beta))):
                loop(K, W, 1, N, None, c, bt)
    elif Hs:
        assemble(pairs, N, Hs)
        if only != "assemble":
            act_hist(pairs, N, Hs)
            for q in range(pairs):  # (a Distiller each: the env and the buffers are per configuration)
                for hs in _orders(q, (None, Hs)):
                    loop(K, W, 1, N, hs)
    else:
        act(pairs, N)
        head(pairs)
        loop(K, W, pairs, N)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
