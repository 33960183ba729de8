"""Bits of every loss head of bg_head.hip: calls each head on fixed inputs and prints one `name shape sha256` line per output array.  Two builds of the
library compute the same bits exactly when two runs of this script (BG_LIB = one library, then the other) print the same text.  Needs a GPU.
    BG_LIB=/path/to/libbooster_gym_amd.so python tools/head_identity.py > a.txt;  python tools/head_identity.py > b.txt;  diff a.txt b.txt
Inputs (seeded, made on the CPU) take every branch: |mu| beyond 1 in places (the bound term), ratios inside and on both sides of the clip range,
advantages of both signs, old_mu != mu, T1's action mirror, sym_coef 0.5.  Shapes: one live row (pair) in a tile; a full and a partial tile; more
tiles than HEAD_MAX_GRID = 768 workgroups with a partial last one (64 rows, or 32 pairs, per tile)."""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from booster_gym_amd import _lib  # noqa: E402
from booster_gym_amd.envs.mirror import mirror_maps  # noqa: E402
from booster_gym_amd.utils import utils as U  # noqa: E402

DEV, A, HK = "cuda:0", 12, 128
p = _lib.ptr


def inputs(rows, B, seed):
    """h of `rows` rows (B, or 2B for the paired heads) and the loss inputs of B rows"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = dict(h=torch.nn.functional.elu(rnd(rows, HK)), W=0.1 * rnd(A, HK), b=0.1 * rnd(A), logstd=-2.0 + 0.1 * rnd(A), old_logstd=torch.full((A,), -2.0))
    mu = d["h"][:B] @ d["W"].t() + d["b"]
    d["old_mu"] = mu + 0.02 * rnd(B, A)
    d["actions"] = mu + 0.135 * rnd(B, A)
    d["old_logp"] = (-0.5 * ((d["actions"] - mu) / d["logstd"].exp()) ** 2 - d["logstd"] - 0.9189385332046727).sum(-1) + 0.3 * rnd(B)
    d["adv"] = rnd(B)
    d["adv_stats"] = torch.stack([d["adv"].double().sum(), (d["adv"].double() ** 2).sum(), torch.tensor(float(max(B, 2)), dtype=torch.float64)])
    d["target"] = mu + 0.1 * rnd(B, A)
    d["values"], d["returns"] = rnd(B), rnd(B)
    return {k: v.contiguous().to(DEV) for k, v in d.items()}


def outputs(rows, n_out, n_stat, with_logstd):
    o = dict(mu_out=torch.full((rows, A), 7.0, device=DEV), g_hidden=torch.full((rows, HK), 7.0, device=DEV), grad_W=torch.empty(n_out, HK, device=DEV),
             grad_b=torch.empty(n_out, device=DEV), grad_b_hidden=torch.empty(HK, device=DEV), stats=torch.zeros(n_stat, dtype=torch.float64, device=DEV))
    if with_logstd:
        o["grad_logstd"] = torch.zeros(A, dtype=torch.float64, device=DEV)
    return o


def report(name, B, o):
    torch.cuda.synchronize()
    for k in ("mu_out", "g_hidden", "grad_W", "grad_b", "grad_b_hidden", "grad_logstd", "stats"):
        if k in o:
            print(f"{name}.{k} B={B} {tuple(o[k].shape)} {hashlib.sha256(o[k].cpu().numpy().tobytes()).hexdigest()}")


def main():
    lib = _lib.load()
    m = json.load(open(os.path.join(ROOT, "booster_gym_amd", "resources", "T1", "T1_locomotion.flat.json")))
    _, _, act_src, act_sign = mirror_maps(m["dof_names"], [a for a in m["joint_axis"] if a], [-0.2, 0, 0, 0.4, -0.25, 0] * 2, 47)
    src, sign = (C.c_int32 * A)(*[int(v) for v in act_src]), (C.c_float * A)(*[float(v) for v in act_sign])
    scr, st = U.head_scratch(DEV), _lib.current_stream_ptr()
    for B in (1, 100, 768 * 64 + 37):
        d = inputs(B, B, B)
        ppo = [d[k] for k in ("h", "W", "b", "logstd", "actions", "old_mu", "old_logstd", "old_logp", "adv", "adv_stats")] + [0.2, 1.0, -0.01]
        o = dict(mu_out=torch.full((B, A), 7.0, device=DEV))
        U.actor_head_forward(d["h"], d["W"], d["b"], o["mu_out"])
        report("bg_actor_head[0]", B, o)
        for name, fin in (("bg_actor_head[1]", None), ("bg_actor_head_partial+bg_reduce_group", _lib.ReduceProblem())):
            o = outputs(B, A, 5, True)
            U.actor_head_loss_backward(*ppo, o["g_hidden"], o["grad_W"], o["grad_b"], o["grad_b_hidden"], o["grad_logstd"], o["stats"], scr, mu_out=o["mu_out"], finish=fin)
            if fin is not None:
                U.reduce_group([fin])
            report(name, B, o)
        o = outputs(B, A, 1, False)
        _lib.check(lib.bg_distill_head(B, *[p(t) for t in (d["h"], d["W"], d["b"], d["target"], o["mu_out"], o["g_hidden"], o["grad_W"], o["grad_b"], o["grad_b_hidden"],
                                                          o["stats"], scr)], st), "bg_distill_head")
        report("bg_distill_head", B, o)
        o = outputs(B, 1, 1, False)
        del o["mu_out"]
        U.critic_head_backward(d["h"], d["W"][0].contiguous(), d["values"], d["returns"], o["g_hidden"], o["grad_W"], o["grad_b"], o["grad_b_hidden"], o["stats"], scr)
        report("bg_critic_head_backward", B, o)
    for B in (1, 100, 768 * 32 + 37):
        d = inputs(2 * B, B, 7 * B)
        ppo = [d[k] for k in ("h", "W", "b", "logstd", "actions", "old_mu", "old_logstd", "old_logp", "adv", "adv_stats")] + [0.2, 1.0, -0.01]
        o = outputs(2 * B, A, 6, True)
        U.actor_head_sym_loss_backward(*ppo, 0.5, (act_src, act_sign), o["g_hidden"], o["grad_W"], o["grad_b"], o["grad_b_hidden"], o["grad_logstd"], o["stats"], scr,
                                       mu_out=o["mu_out"])
        report("bg_actor_head_sym", B, o)
        o = outputs(2 * B, A, 2, False)
        _lib.check(lib.bg_distill_head_sym(B, *[p(t) for t in (d["h"], d["W"], d["b"], d["target"])], 0.5, src, sign,
                                           *[p(t) for t in (o["mu_out"], o["g_hidden"], o["grad_W"], o["grad_b"], o["grad_b_hidden"], o["stats"], scr)], st), "bg_distill_head_sym")
        report("bg_distill_head_sym", B, o)


if __name__ == "__main__":
    main()
