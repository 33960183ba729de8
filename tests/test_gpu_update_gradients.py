"""The gradient every optimiser step of Runner.update() assembles, against float64 autograd of the same loss on the step's own inputs
(tests/update_grad_ref.py), on every plan a switch can select, at the shapes where the slabs go ragged or odd, and under every feature key that rides
on the update.  The parameter-level tests (test_full_update_matches_reference_loop and its siblings) look at the update through Adam, whose step
lr m / sqrt(v) does not change when a tensor's gradient is scaled; these look at FlatAdam.grad itself.

Per case: one rollout(), then update() under record_steps, which leaves the plan as the runner resolves it (asserted).  For every step:
  (a) every tensor within 1e-4 of the float64 tensor's largest entry (tests/test_gpu_distill_memory._grad_bound's rule), printed beside the error of
      an fp32 torch-autograd twin of the same loss on the same record;
  (b) the squared norm the clip used (where the form of the step leaves it readable) within 1e-3 of the float64 gradient's norm;
  (c) the learning rate is raised (TUNED) until the float64 reference clips at least 5 % of the rows of the LAST step's surrogate and leaves at least
      5 % unclipped, with no row's ratio within 2e-5 of 0.8 / 1.2 (ten fp32 roundings of a log-probability of size 30: such a row may fall on the other
      side in fp32): the clipped branch of the surrogate's backward is compared, not only ratio = 1;
  (d) default case: the same comparison against a reference normalised with the population std (B for B - 1: a scale error of 1 / (2B) = 8e-4 on
      the surrogate's gradient) must FAIL (a) on the actor's largest weight tensor.
Terrain: plane, except terrain.actor_heights, whose scan needs a height field.

Measured on an MI355X, case plan:default (128 envs x 5 steps, B = 640, E = 3, seed 11, learning rate 1e-3), the largest of the three steps per tensor as
error / |ref|max, the fp32 twin's in brackets:
  logstd 1.05e-6 (3.67e-6)
  critic .0.weight 9.86e-7 (8.94e-7)  .0.bias 1.15e-6 (3.47e-7)  .2.weight 9.12e-7 (1.24e-6)  .2.bias 1.05e-6 (2.29e-7)
         .4.weight 9.63e-7 (1.23e-6)  .4.bias 1.06e-6 (3.49e-7)  .6.weight 8.69e-7 (9.93e-7)  .6.bias 9.80e-7 (2.37e-7)
  actor  .0.weight 1.28e-6 (4.38e-6)  .0.bias 9.22e-7 (3.06e-6)  .2.weight 1.26e-6 (4.11e-6)  .2.bias 8.73e-7 (3.26e-6)
         .4.weight 1.08e-6 (3.29e-6)  .4.bias 8.60e-7 (3.03e-6)  .6.weight 1.18e-6 (4.21e-6)  .6.bias 1.07e-6 (3.44e-6)
The clip's norm agrees with float64's to 8.4e-7.  Rows the reference clips: 0 / 86.9 % / 91.1 % in steps 0 / 1 / 2, the nearest ratio 2.9e-3 from a
boundary.  (d): against the population-std reference actor.2.weight is off by 7.81e-4 in every step, 7.8 x the bound.  The largest error of any case:
4.6e-5 (twin 1.0e-5) in critic.6.bias of key:hidden_widths' first step (the sum of v - ret over the rows, whose terms cancel).  No tensor of any case needed a bound of its own (BOUNDS is empty), and no gradient was found wrong.

A recurrent actor (RECURRENT: algorithm.rnn_hidden_size at 100 x 5 / H = 128 and 48 x 24 / H = 256, runner.num_env_mini_batches = 3 at 384 x 5): the record
carries the step's h0 and reset flags and the reference runs the cell through time (update_grad_ref.recurrent_means); one iteration runs in front of
the recorded one, so that every step starts from a state that is not zero and, under episodes of 7 control steps, some env enters a step behind the
first with a zero state (asserted, with the cell's four tensors, the trunk's eight and logstd among the compared).  Measured on an MI355X, the
largest error / |ref|max of any step and tensor (the twin's in brackets): 1.6e-6 (8.5e-7) in critic.6.weight / 4.3e-6 (2.9e-6) in critic.6.weight / 1.3e-6
(1.4e-7) in critic.4.bias; of the cell's four tensors alone 1.3e-6 (1.5e-6) / 8.0e-7 (1.4e-6) / 7.9e-7 (1.4e-6).  Control: against a restatement that detaches the
state between steps (no back-propagation through time) memory.weight_hh of key:rnn_hidden_size's first step is off by 0.277 of its largest entry, 2769 x the bound."""
import math

import pytest
import torch

from test_gpu_ppo import SWITCHES
from update_grad_ref import model_factory, record_steps, step_gradients_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND, TWIN_FLOOR, NORM_BOUND, MARGIN = 1e-4, 2.5e-5, 1e-3, 2e-5
SCHEDULING = ("rollout_forward_one_step_per_group", "rollout_forward_five_steps_per_group", "chain_one_workgroup_per_slab", "backward_chain_one_workgroup_per_slab")
PLAN_CASES = [k for k in SWITCHES if k not in SCHEDULING]


def _plain(n, T, E):
    def make(seed, lr):
        from booster_gym_amd.utils.config import load_cfg
        from booster_gym_amd.utils.runner import Runner

        return Runner(cfg=load_cfg("T1", {"env.num_envs": n, "terrain.type": "plane", "runner.mini_epochs": E, "runner.horizon_length": T, "basic.seed": seed,
                                          "algorithm.learning_rate": lr}))
    return make


def _common(T, E, seed, lr, plane=True):
    ov = {"runner.mini_epochs": E, "runner.horizon_length": T, "basic.seed": seed, "algorithm.learning_rate": lr}
    if plane:
        ov["terrain.type"] = "plane"
    return ov


def _symmetry(seed, lr):
    from test_gpu_symmetry import _runner

    return _runner(384, E=2, T=5, seed=seed, **{"algorithm.learning_rate": lr})


def _smoothness(seed, lr):
    from test_gpu_smoothness import _runner

    return _runner(128, E=2, T=5, seed=seed, pairs="next", **{"algorithm.learning_rate": lr})


def _obs_norm(seed, lr):
    from test_gpu_obs_norm import KEY, _runner

    return _runner(128, **{KEY: True}, **_common(5, 2, seed, lr))


def _frame_stack(seed, lr):
    from test_gpu_frame_stack import _runner

    return _runner(128, 3, **_common(5, 2, seed, lr))


def _actor_heights(seed, lr):
    from test_gpu_actor_heights import _runner

    return _runner(128, 3, **_common(5, 2, seed, lr, plane=False))


def _privileged_extras(seed, lr):
    from test_gpu_privileged_extras import ALL, _runner

    return _runner(128, ALL, **_common(5, 2, seed, lr))


def _widths(seed, lr):
    from test_gpu_network_widths import _runner

    return _runner(128, (512, 256, 128), (512, 256, 128), **_common(5, 2, seed, lr))


def _mini_batches(seed, lr):
    from test_gpu_mini_batches import KEY, _runner

    return _runner(256, **{KEY: 2}, **_common(5, 2, seed, lr))  # (two mini-batches of 640 rows: whole slabs)


def _recurrent(n, T, E, H, **over):
    """PPO on a recurrent actor (algorithm.rnn_hidden_size = H), under episodes of 7 control steps (tests/test_gpu_actor_memory.SHORT_EPISODES): every
    env times out on its 8th step, so resets fall inside the recorded horizon -- the second one at T = 5, the first at T = 24."""
    def make(seed, lr):
        from booster_gym_amd.utils.config import load_cfg
        from booster_gym_amd.utils.runner import Runner
        from test_gpu_actor_memory import KEY, SHORT_EPISODES

        return Runner(cfg=load_cfg("T1", {"env.num_envs": n, KEY: H, **SHORT_EPISODES, **over, **_common(T, E, seed, lr)}))
    return make


# name: (runner factory (seed, lr), key into SWITCHES, iterations run in front of the recorded one)
CASES = {f"plan:{k}": (_plain(128, 5, 3), k, 0) for k in PLAN_CASES}
CASES.update({"shape:100x5": (_plain(100, 5, 3), "default", 0),      # ragged last slab everywhere, no forward-ahead
              "shape:384x3": (_plain(384, 3, 3), "default", 0),      # 9 slabs: an odd count
              "shape:256x24": (_plain(256, 24, 3), "default", 0),    # the workload's horizon
              "key:symmetry_loss": (_symmetry, "default", 0),        # 15 slabs: the mirrored half starts on an odd slab
              "key:smoothness_loss": (_smoothness, "default", 0),
              "key:empirical_normalization": (_obs_norm, "default", 1),
              "key:frame_stack": (_frame_stack, "default", 0),
              "key:actor_heights": (_actor_heights, "default", 0),
              "key:privileged_extras": (_privileged_extras, "default", 0),
              "key:hidden_widths": (_widths, "default", 0),
              "key:num_mini_batches": (_mini_batches, "default", 0),
              # a recurrent actor: the cell's gradients through time, every optimiser step from its own parameters (ratios away from 1 after the first)
              "key:rnn_hidden_size": (_recurrent(100, 5, 3, 128), "default", 1),          # 6 tiles of the recurrence and a tail of 4 rows; B = 500: three
                                                                                          # 128-row blocks of bg_gru_bias_partial and a ragged one
              "key:rnn_hidden_size_wide_24": (_recurrent(48, 24, 2, 256), "default", 1),  # the workload's horizon; B = 1152: nine 128-row blocks
              # three env-wise mini-batches, six optimiser steps, each from its own gathered state and flags.  384 envs, not 96: a step's rows
              # T x envs / K must be whole 128-row slabs (runner.env_mini_batches refuses 5 x 32 = 160), so 128 envs a step is the smallest at T = 5
              "key:num_env_mini_batches": (_recurrent(384, 5, 2, 128, **{"runner.num_env_mini_batches": 3}), "default", 1)})
RECURRENT = ("key:rnn_hidden_size", "key:rnn_hidden_size_wide_24", "key:num_env_mini_batches")
# (basic.seed, algorithm.learning_rate) per case, chosen on the GPU so that (c) holds -- conditions on the float64 reference alone -- and kept fixed
SEED, LR = 11, 1e-3
TUNED = {"shape:256x24": (12, LR),           # seed 11: a row 1.86e-5 from the boundary
         "key:hidden_widths": (SEED, LR / 3)}  # at 1e-3 the wider networks move further: 96.7 % of the rows clipped, fewer than 5 % left
# The three recurrent cases hold (c) at the default pair (11, 1e-3), the first one tried: the float64 reference clips 47.2 % / 63.9 % / 58.1 % of the
# last step's rows (key:rnn_hidden_size / _wide_24 / key:num_env_mini_batches), the nearest ratio 7.3e-4 / 5.8e-5 / 1.9e-3 from a boundary.
# (case, tensor): a bound other than BOUND, 4 x the fp32 twin's measured error where the twin itself is above TWIN_FLOOR (see the docstring)
BOUNDS = {}


def run_case(name, seed=None, lr=None):
    """The case's measurements: per step {tensor: (error / |ref|max, the twin's, |ref|max)}, the norms, the last step's ratios; no assertions but on
    the plan."""
    from booster_gym_amd.utils.model import MLPTrainer

    make, switch, warm = CASES[name]
    s0, l0 = TUNED.get(name, (SEED, LR))
    seed, lr = s0 if seed is None else seed, l0 if lr is None else lr
    attrs, cls_attrs = SWITCHES[switch]
    saved = {k: getattr(MLPTrainer, k) for k in cls_attrs}
    try:
        for k, v in cls_attrs.items():
            setattr(MLPTrainer, k, v)
        r = make(seed, lr)
        for k, v in attrs.items():
            assert hasattr(r, k)
            setattr(r, k, v)
        obs, infos = r.env.reset()
        r.buffer["obses"][0].copy_(obs); r.buffer["privileged_obses"][0].copy_(infos["privileged_obs"])
        for _ in range(warm):
            r.iteration()
        r.rollout()
        plan, fwd_plan = r._resolve_plan(), r._fwd_plan
        K, E = max(r._mini_batches, r._env_mini_batches), r.cfg["runner"]["mini_epochs"]
        step_plan = r._mb_plan if K > 1 else plan
        with record_steps(r) as steps:
            assert r._resolve_plan() == plan and (K == 1 or r._mb_plan == step_plan), "the recorder changed the plan"
            r.update()
        torch.cuda.synchronize()
        assert "_epoch_gradients_and_step" not in vars(r) and r._resolve_plan() == plan
    finally:
        for k, v in saved.items():
            setattr(MLPTrainer, k, v)
    assert len(steps) == E * K and all(rec["plan"] == step_plan for rec in steps)
    B = r._old_logp.numel()
    assert all(rec["rows"] == B // K for rec in steps)
    if K > 1:  # each step of a mini-epoch on its own rows
        assert not torch.equal(steps[0]["x_c"], steps[1]["x_c"]) and not torch.equal(steps[0]["adv"], steps[1]["adv"])
    extra = None
    if r._smooth:
        extra = ("smoothness", r._smooth_coef)
    elif r._symmetry:
        extra = ("symmetry", r._symmetric_coef, r.env.mirror_maps())
    make_model, alg = model_factory(r), r.cfg["algorithm"]
    out = dict(name=name, seed=seed, lr=lr, plan=plan, ahead=fwd_plan == plan, B=B, steps=[], extra=extra,
               numel={k: p.numel() for k, p in r.model.named_parameters()})
    if name in RECURRENT:  # every step reads a state and flags of its own rows, and some env enters a step behind the first with a zero state
        T, n = r.cfg["runner"]["horizon_length"], r.env.num_envs // K
        assert all(tuple(rec["h0"].shape) == (n, r._memory) and tuple(rec["resets"].shape) == (T, n) for rec in steps)
        out["resets_inside"] = [int(rec["resets"][1:].sum()) for rec in steps]
        out["h0_max"] = [rec["h0"].abs().max().item() for rec in steps]
        if K > 1:
            assert not torch.equal(steps[0]["h0"], steps[1]["h0"])
        print(f"{name}: reset flags behind step 0 per optimiser step {out['resets_inside']}, |h0|max {out['h0_max']}")
    for s, rec in enumerate(steps):
        aux = {}
        ref = step_gradients_f64(rec, make_model, alg, extra, aux=aux)
        twin = step_gradients_f64(rec, make_model, alg, extra, dtype=torch.float32)
        assert list(ref) == list(rec["grads"])
        rows = {}
        for k, g in ref.items():
            top = g.abs().max().item()
            assert top > 0 and g.shape == rec["grads"][k].shape, k
            rows[k] = ((rec["grads"][k].double() - g).abs().max().item() / top, (twin[k].double() - g).abs().max().item() / top, top)
        norm_ref = math.sqrt(sum((g ** 2).sum().item() for g in ref.values()))
        used = None if rec["clip_sqnorm"] is None else math.sqrt(rec["clip_sqnorm"].item())
        ratio = aux["ratio"]
        m = dict(rows=rows, norm_ref=norm_ref, norm_used=used, form=rec["form"], clipped=((ratio < 0.8) | (ratio > 1.2)).double().mean().item(),
                 margin=torch.minimum((ratio - 0.8).abs(), (ratio - 1.2).abs()).min().item(), pair_loss=aux["pair_loss"])
        if name == "plan:default":
            wrong = step_gradients_f64(rec, make_model, alg, extra, unbiased=False)
            m["wrong"] = {k: (rec["grads"][k].double() - g).abs().max().item() / g.abs().max().item() for k, g in wrong.items()}
        if name == "key:rnn_hidden_size" and s == 0:  # the control: a restatement without back-propagation through time
            k, cut = "memory.weight_hh", step_gradients_f64(rec, make_model, alg, extra, bptt=False)
            m["no_bptt"] = (rec["grads"][k].double() - cut[k]).abs().max().item() / cut[k].abs().max().item()
        out["steps"].append(m)
        for k, (e, t, top) in rows.items():
            print(f"{name} step {s} {k}: error {e:.3e} of |ref|max {top:.3e}; fp32 twin {t:.3e}")
        print(f"{name} step {s}: norm {norm_ref:.6f}, the clip's {used} ({rec['form']}); clipped rows {m['clipped']:.3f}, nearest ratio to 0.8 / 1.2 {m['margin']:.2e}")
    return out


_PLANS = {}  # the plans the plan:* cases have resolved so far in this session


def check_case(m):
    name, plan = m["name"], m["plan"]
    if name.startswith("plan:"):  # every switch of these cases resolves a plan of its own at this shape (none is silently ignored)
        _PLANS[name] = plan
        same = [k for k, p in _PLANS.items() if k != name and p == plan]
        assert not same, (name, same)
    if name == "plan:default":  # the plan bench.py times
        assert plan.one_tail and plan.fused_opt and plan.ahead and m["ahead"] and plan.wgrad == 9
        assert plan.critic.fwd == plan.actor.fwd == "chain_split" and plan.critic.bwd == plan.actor.bwd == "chain_split"
    if m["extra"] is not None:
        assert all(s["pair_loss"] > 0 for s in m["steps"])
    if name in RECURRENT:
        assert all(n > 0 for n in m["resets_inside"]) and all(h > 1e-3 for h in m["h0_max"]), (name, m["resets_inside"], m["h0_max"])
        for st in m["steps"]:  # the cell's four tensors, the trunk's eight and the log-std are among the compared
            assert {"memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh", "logstd"} <= set(st["rows"])
            assert sum(k.startswith("actor.") for k in st["rows"]) == 8
    # (c): conditions on the float64 reference
    last = m["steps"][-1]
    assert 0.05 <= last["clipped"] <= 0.95, (name, last["clipped"])
    assert last["margin"] > MARGIN, (name, last["margin"])
    # (a), (b)
    missed = []
    for s, st in enumerate(m["steps"]):
        for k, (e, t, top) in st["rows"].items():
            if not e <= BOUNDS.get((name, k), BOUND):
                missed.append((s, k, e, t))
        if st["norm_used"] is not None:
            assert abs(st["norm_used"] - st["norm_ref"]) <= NORM_BOUND * st["norm_ref"], (name, s, st["norm_used"], st["norm_ref"])
    assert not missed, (name, missed)
    # (bg_optimizer_step alone keeps its norm in registers)
    assert all((st["norm_used"] is None) == (st["form"] == "fused") for st in m["steps"])
    if name == "key:rnn_hidden_size":  # the control: without back-propagation through time the recurrent weights' gradient is another one
        off = m["steps"][0]["no_bptt"]
        print(f"{name} step 0: against a restatement that detaches the state between steps memory.weight_hh is off by {off:.3e} ({off / BOUND:.0f} x the bound)")
        assert off > BOUND, off
    if name == "plan:default":  # (d)
        k = max((k for k in last["rows"] if k.startswith("actor.") and k.endswith(".weight")), key=m["numel"].get)
        for s, st in enumerate(m["steps"]):
            print(f"{name} step {s}: against the population-std reference {k} is off by {st['wrong'][k]:.3e} ({st['wrong'][k] / BOUND:.1f} x the bound)")
        assert all(st["wrong"][k] > BOUND for st in m["steps"]), [st["wrong"][k] for st in m["steps"]]


@pytest.mark.parametrize("name", list(CASES))
def test_every_step_of_the_update_leaves_the_float64_gradient(name):
    check_case(run_case(name))
