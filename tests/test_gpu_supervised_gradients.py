"""The gradient every optimiser step of SupervisedTrainer.step assembles (utils/supervised.py: the distilled student's and the state estimator's one
update), against float64 autograd of the same loss on the step's own inputs (tests/supervised_grad_ref.py), on every plan a switch can select, at the
shapes where the slabs go ragged or odd, with the symmetry loss, a longer history, a recurrent student, and for the estimator.  The iteration tests
(test_gpu_distill._check_one_iteration and its siblings) look at the update through Adam, whose step lr m / sqrt(v) does not change when a tensor's
gradient is scaled and whose first step is lr sign(g); these look at FlatAdam.grad itself, in front of bg_adam_step.

Per case: one small env, one rollout (two where a state must not be zero), then update() under record_supervised_steps, which leaves every switch and
the plan as they are (asserted).  For EVERY optimiser step of the update:
  (a) every trained tensor within BOUND = 1e-4 of the float64 tensor's largest entry (tests/test_gpu_update_gradients.py's bounds and BOUNDS rule),
      printed beside the error of an fp32 torch-autograd twin of the same loss on the same record;
  (b) sqrt of the squared norm the clip divided by (FlatAdam._gnorm) within 1e-3 of the float64 gradient's norm;
  (c) stats / (12 B) within 1e-4 relative of the float64 loss terms (both terms with the symmetry loss);
  (d) on the float64 reference alone: every tensor's |ref|max > 0; the last step's loss below the first's; with the symmetry loss the symmetric
      term's gradient alone carries at least 5 % of the whole gradient's norm in every step; a recurrent student starts from |h0|max > 1e-3 and some
      env enters a step behind the first with a zero state;
  (e) controls that must FAIL (a): a WRONG float64 reference on the same record leaves a named tensor off by more than BOUND --
      student:ragged_250     the loss divided by the padded row count (256 for 250: a scale error of 2.3 %, the kind Adam hides)
      student:symmetry_384   M_a net(x[:B]) detached: no gradient through the original half of the symmetric term
      student:default        every hidden bias gradient doubled (a column sum finished twice); and float64 copies stepped three times by clipped
                             Adam at the iteration tests' learning rate 1e-5 on the right and on the doubled gradient stay allclose(rtol 1e-3,
                             atol 2e-6) -- the iteration tests' check does not see it, which is the reason this file exists
      student:memory_128     no back-propagation through time.
The student cases run at the shipped distillation.learning_rate 1e-3 (the iteration tests' 1e-5 would leave the three steps' parameters all but equal),
the estimator cases at the shipped estimator.learning_rate.

In front of the recorded update every row behind the batch of the network's workspaces is set to NaN (_poison_pad_rows): the chained backward launch
multiplies whole 128-row slabs of the stored activations into accumulators that are zero behind row M, so a ragged batch gets finite bias gradients only
because the chained forward launch stores every slab in full; torch.empty would leave that to chance, NaN makes it a checked property.

Measured on an MI355X, case student:default (64 envs x 4 steps, B = 256, three steps at the learning rate 1e-3), the largest of the three steps per
tensor as error / |ref|max, the fp32 twin's in brackets:
  net.0.weight 1.74e-7 (4.65e-7)  net.0.bias 1.45e-7 (1.45e-7)  net.2.weight 2.07e-7 (5.16e-7)  net.2.bias 1.48e-7 (1.21e-7)
  net.4.weight 1.22e-7 (6.26e-7)  net.4.bias 1.14e-7 (1.19e-7)  net.6.weight 1.21e-7 (3.95e-7)  net.6.bias 1.05e-7 (1.08e-7)
The largest error of any case: 4.16e-7 (twin 1.07e-7) in net.2.bias of student:odd_slabs_384's third step; every case's largest lies between 1.3e-7 and
4.2e-7, the recurrent student's in memory.weight_hh (2.2e-7, H = 128) and memory.bias_hh (3.1e-7, H = 256).  The clip's norm agrees with float64's to
2.7e-7 in every step of every case (the symmetry cases' first steps have norms of 1.36 / 1.36 / 2.44: the clip is active there), stats / (12 B) with the
loss terms to 2.4e-7.  No tensor of any case needed a bound of its own (BOUNDS is empty; the largest twin 1.8e-6, net.2.weight of estimator:3072's first
step), and NO GRADIENT WAS FOUND WRONG: the ragged cases hold with 42 (student:ragged_250) to 672 (student:288) NaN pad rows in the workspaces, and so
do the four student:ragged_250:<switch> cases (the fp32 chain, the per-layer fp32 and split-bf16 kernels and the per-layer backward behind the chained
forward on the same 250 rows: largest error 2.6e-7 to 3.0e-7).
(d): the symmetric term's share of the gradient's norm at COEF = 10, steps 0 / 1 / 2: 0.965 / 0.975 / 0.994 (symmetry_384), 0.965 / 0.976 / 0.994
(symmetry_288), 0.969 / 0.970 / 1.024 (symmetry_per_layer); the recurrent cases start from |h0|max 0.408 (H = 128) / 0.287 (H = 256) with 40 reset flags
behind step 0 (every env times out on the horizon's third step).  Every case's loss falls from the first step to the last (student:wide: 0.0125, 0.0017,
0.0035).
(e): the controls' factors over BOUND, in every step: ragged_250 net.2.weight off by 2.40e-2 (240 x); symmetry_384 net.2.weight by 1.16 / 0.90 / 0.97
(11,611 / 8,954 / 9,700 x); default net.0.bias by 0.5 of the doubled reference (5,000 x), while the float64 copies stepped on the doubled gradient end
at most 4.3e-8 from the right ones (net.2.bias; each parameter moved 3.0e-5): allclose(rtol 1e-3, atol 2e-6) holds for all eight tensors; memory_128
memory.weight_hh by 0.316 / 0.343 / 0.314 (3,156 / 3,432 / 3,141 x)."""
import math

import pytest
import torch

from supervised_grad_ref import cell_factory, net_factory, record_supervised_steps, supervised_gradients_f64
from test_gpu_update_gradients import BOUND, NORM_BOUND, TWIN_FLOOR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 12
LOSS_BOUND, SHARE = 1e-4, 0.05
SMALL = {"env.num_envs": 100, "runner.horizon_length": 5}  # a case that does not name its shape: B = 500, three 128-row slabs and a ragged one


def _shape(n, T):
    return {"env.num_envs": n, "runner.horizon_length": T}


def _student(frames=1, over=None, switch=None, plan=None, rows=None, kin=64, warm=0, symmetry=False, memory=0):
    """A Distiller case: the teacher's env.frame_stack, overrides of tests/test_gpu_distill._cfg (without a shape: that module's own N = 64, T = 4), the
    one MLPTrainer switch set in front of the constructor, (fwd, bwd, wgrad_terms) the plan must be, the rows / padded width of the step's input."""
    return dict(kind="student", frames=frames, over=dict(over or {}), switch=dict(switch or {}), plan=plan, rows=rows, kin=kin, warm=warm, symmetry=symmetry, memory=memory)


def _estimator(H=1, n=100, over=None, plan=None, rows=None, kin=64):
    """A Runner case with estimator.enabled on tests/test_gpu_estimator._runner; the recorded trainer is the estimator's, PPO's step runs unrecorded."""
    return dict(kind="estimator", frames=H, n=n, over=dict(over or {}), switch={}, plan=plan, rows=rows, kin=kin, warm=0, symmetry=False, memory=0)


def _coef():
    from test_gpu_distill_symmetry import COEF

    return COEF


def _short_episodes():
    from test_gpu_actor_memory import SHORT_EPISODES  # every env times out on its 8th step: inside the second horizon of 5

    return SHORT_EPISODES


# one MLPTrainer switch each, at student:default's shape; every one must resolve a (plan, wgrad_terms) no other resolves (check_case)
SWITCH_CASES = {"CHAIN_SPLIT=False": {"CHAIN_SPLIT": False}, "CHAIN=False": {"CHAIN": False}, "CHAIN_SPLIT_BWD=False": {"CHAIN_SPLIT_BWD": False},
                "WGRAD_SPLIT=0": {"WGRAD_SPLIT": 0}, "CHAIN_ALTERNATE=False": {"CHAIN_ALTERNATE": False}, "SPLIT=9": {"SPLIT": 9}, "SPLIT=6": {"SPLIT": 6}}
CASES = {
    # H = 1, N = 64, T = 4, B = 256: the shipped configuration's plan
    "student:default": _student(plan=("chain_split", "chain_split", 9), rows=256),
    # a ragged second slab; rows % 32 != 0: fp32 weight gradients behind the chained bf16 backward
    "student:ragged_250": _student(over=_shape(50, 5), plan=("chain_split", "chain_split", 0), rows=250),
    # two slabs and 32 rows: 9-product weight gradients at a row count that is not whole slabs
    "student:288": _student(over=_shape(96, 3), plan=("chain_split", "chain_split", 9), rows=288),
    "student:odd_slabs_384": _student(over=_shape(128, 3), plan=("chain_split", "chain_split", 9), rows=384),
    "student:per_layer": _student(frames=2, over=SMALL, plan=("layer", "layer", 0), rows=500, kin=128),
    # a student history of 3 over a teacher of 1: 141 columns pad to 256
    "student:history": _student(over={**SMALL, "distillation.student_frame_stack": 3}, plan=("layer", "layer", 0), rows=500, kin=256),
    "student:wide": _student(over={**SMALL, "distillation.student_hidden": [512, 256, 128]}, plan=("layer", "layer", 0), rows=500),
    **{f"student:switch:{k}": _student(switch=v, rows=256) for k, v in SWITCH_CASES.items()},
    # the switches that put other kernels on the stored activations, on student:ragged_250's ragged second slab (its pad rows hold NaN)
    "student:ragged_250:CHAIN_SPLIT=False": _student(over=_shape(50, 5), switch={"CHAIN_SPLIT": False}, plan=("chain", "layer", 0), rows=250),
    "student:ragged_250:CHAIN=False": _student(over=_shape(50, 5), switch={"CHAIN": False}, plan=("layer", "layer", 0), rows=250),
    "student:ragged_250:CHAIN_SPLIT_BWD=False": _student(over=_shape(50, 5), switch={"CHAIN_SPLIT_BWD": False}, plan=("chain_split", "layer", 0), rows=250),
    "student:ragged_250:SPLIT=9": _student(over=_shape(50, 5), switch={"SPLIT": 9}, plan=("layer_split", "layer_split", 0), rows=250),
    # 768 rows: the mirrored half starts on odd slab 3
    "student:symmetry_384": _student(over=_shape(128, 3), plan=("chain_split", "chain_split", 9), rows=768, symmetry=True),
    # 576 rows: the mirrored half starts at row 32 of slab 2, and the last slab is ragged
    "student:symmetry_288": _student(over=_shape(96, 3), plan=("chain_split", "chain_split", 9), rows=576, symmetry=True),
    "student:symmetry_per_layer": _student(frames=2, over=SMALL, plan=("layer", "layer", 0), rows=1000, kin=128, symmetry=True),
    # N = 40: two 16-row tiles of the recurrence and a tail of 8; T = 5; a rollout in front, so that h0 is not zero and resets fall inside the horizon
    "student:memory_128": _student(over=_shape(40, 5), plan=("layer", "layer", 0), rows=200, warm=1, memory=128),
    "student:memory_256": _student(over=_shape(40, 5), plan=("layer", "layer", 0), rows=200, warm=1, memory=256),
    # two hidden layers are not chainable: the per-layer plan
    "estimator:default": _estimator(over={"runner.horizon_length": 5}, plan=("layer", "layer", 0), rows=500),
    "estimator:chained": _estimator(over={"runner.horizon_length": 5, "estimator.hidden": [256, 128, 128]}, plan=("chain_split", "chain_split", 0), rows=500),
    "estimator:frame_stack_3": _estimator(H=3, over={"runner.horizon_length": 5}, plan=("layer", "layer", 0), rows=500, kin=256),
    "estimator:3072": _estimator(n=128, plan=("layer", "layer", 0), rows=3072),  # tests/test_gpu_estimator.test_runner_rollout_and_update's shape
}
# distillation.symmetric_coef per symmetry case: tests/test_gpu_distill_symmetry.COEF unless (d)'s share of the symmetric term needs more
SYM_COEF = {}
# the controls of (e): case -> (keyword of supervised_gradients_f64 that makes the reference wrong, the tensor that must be off)
CONTROLS = {"student:ragged_250": (dict(mean_rows=256), "net.2.weight"),
            "student:symmetry_384": (dict(detach_mirrored_original=True), "net.2.weight"),
            "student:default": (dict(hidden_bias_scale=2.0), "net.0.bias"),
            "student:memory_128": (dict(bptt=False), "memory.weight_hh")}
# (case, tensor): (a bound other than BOUND, the fp32 twin's measured error): 4 x the twin's error, and only where the twin itself is above TWIN_FLOOR
BOUNDS = {}


@pytest.fixture(scope="module")
def teachers(tmp_path_factory):
    """frames -> the path of a seeded perceptive teacher of that env.frame_stack (tests/test_gpu_distill._save_teacher), saved once."""
    from test_gpu_distill import _save_teacher

    root, made = tmp_path_factory.mktemp("teachers"), {}

    def get(frames):
        if frames not in made:
            made[frames] = _save_teacher(str(root / f"teacher_h{frames}.pth"), frames)
        return made[frames]
    return get


def _adam_stepped(rec, make_net, scale, lr=1e-5, steps=3):
    """float64 copies of the record's parameters after `steps` clipped Adam steps on the float64 gradient with the hidden bias gradients x `scale`."""
    names = list(rec["params"])
    params = [torch.nn.Parameter(rec["params"][k].double().clone()) for k in names]
    opt = torch.optim.Adam(params, lr=lr)
    for _ in range(steps):
        g = supervised_gradients_f64(dict(rec, params={k: p.detach() for k, p in zip(names, params)}), make_net, hidden_bias_scale=scale)
        for k, p in zip(names, params):
            p.grad = g[k].clone()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    return {k: p.detach() for k, p in zip(names, params)}


def _poison_pad_rows(sup, x):
    """NaN into every row behind the batch of the network's workspaces (activations and gradients are allocated in whole 128-row slabs and hold
    `rows` rows: MLPTrainer._alloc), in front of the first step.  The chained backward launch multiplies whole slabs of the stored activations into
    accumulators that are zero behind row M, so those rows must be finite by the time it reads them: the chained forward launch stores every slab in
    full.  torch.empty leaves that to chance; with NaN there, a pass that reads a pad row it did not write gives NaN gradients, which fail (a).
    x: the network's input of the steps to come ([rows][padded width]).  Returns the number of rows poisoned."""
    tr = sup.mlp
    tr.prepare(x)  # (the workspaces the first step would allocate: forward() finds them in place)
    count = 0
    for t in tr.acts + tr.gin[1:]:
        whole = t._base
        if whole is not None and whole.shape[0] > t.shape[0]:
            assert whole.data_ptr() == t.data_ptr() and whole.shape[1:] == t.shape[1:]
            whole[t.shape[0]:] = float("nan")
            count += whole.shape[0] - t.shape[0]
    return count


def _build(spec, teachers):
    """(the object whose update() runs, its SupervisedTrainer, the network's input of its steps, the optimiser steps an update takes)."""
    if spec["kind"] == "student":
        from test_gpu_distill import _Rec, _cfg

        from booster_gym_amd.utils.distill import Distiller

        over = {"distillation.learning_rate": 1.0e-3, **spec["over"]}
        if spec["symmetry"]:
            over["distillation.symmetric_coef"] = spec["coef"]
        if spec["memory"]:
            over.update({"distillation.student_memory": spec["memory"], **_short_episodes()})
        d = Distiller(cfg=_cfg(teachers(spec["frames"]), spec["frames"], **over))
        d.begin(recorder=_Rec())
        return d, d._sup, (d._sup.gru.h if spec["memory"] else d._student_in), d.dcfg.num_epochs
    from test_gpu_estimator import _runner

    r = _runner(spec["frames"], spec["n"], **spec["over"])
    return r, r._est_trainer.sup, r._est_trainer.x, r._est.num_epochs


def run_case(name, teachers):
    """The case's measurements: per step {tensor: (error / |ref|max, the twin's, |ref|max)}, the norms, the losses, the shares, the controls' errors; no
    assertions but on the plan and on what the recorder saw."""
    from booster_gym_amd.utils.model import MLPTrainer

    spec = dict(CASES[name])
    if spec["symmetry"]:
        spec["coef"] = SYM_COEF.get(name, _coef())
    saved = {k: getattr(MLPTrainer, k) for k in spec["switch"]}
    try:
        for k, v in spec["switch"].items():  # Distiller resolves its plan once, at construction: the switch goes in front of it
            assert getattr(MLPTrainer, k) != v, (k, "is the default")
            setattr(MLPTrainer, k, v)
        owner, sup, net_in, E = _build(spec, teachers)
        for _ in range(spec["warm"]):
            owner.rollout()
            owner.buffer.roll()
        owner.rollout()
        poisoned = _poison_pad_rows(sup, net_in)
        plan, terms = sup.plan, sup.wgrad_terms
        with record_supervised_steps(sup) as steps:
            owner.update()
        torch.cuda.synchronize()
        assert "step" not in vars(sup) and "step" not in vars(sup.optimizer) and (sup.plan, sup.wgrad_terms) == (plan, terms), "the recorder changed the plan"
    finally:
        for k, v in saved.items():
            setattr(MLPTrainer, k, v)
    assert len(steps) == E and all((rec["plan"], rec["wgrad_terms"]) == (plan, terms) for rec in steps)
    B = steps[0]["rows"]
    assert all(rec["rows"] == B and tuple(rec["x"].shape) == (spec["rows"], spec["kin"]) for rec in steps) and spec["rows"] == (2 * B if spec["symmetry"] else B)
    assert all((rec["symmetry"] is not None) == spec["symmetry"] and ("h0" in rec) == bool(spec["memory"]) for rec in steps)
    make_net, make_cell = net_factory(sup), cell_factory(sup)
    out = dict(name=name, plan=plan, wgrad_terms=terms, B=B, steps=[], symmetry=spec["symmetry"], memory=spec["memory"], expect=spec["plan"])
    print(f"{name}: {spec['rows']} x {spec['kin']} input rows, B = {B}, plan {plan.fwd} / {plan.bwd}, alternate {plan.alternate}, terms {plan.terms}, "
          f"weight-gradient products {terms}, {E} steps, {poisoned} pad rows of the workspaces set to NaN")
    if spec["symmetry"]:
        assert all(rec["symmetry"][0] == spec["coef"] for rec in steps)
    if spec["memory"]:
        T, n = owner.T, owner.N
        assert all(tuple(rec["h0"].shape) == (n, spec["memory"]) and tuple(rec["resets"].shape) == (T, n) for rec in steps)
        out["resets_inside"] = [int(rec["resets"][1:].sum()) for rec in steps]
        out["h0_max"] = [rec["h0"].abs().max().item() for rec in steps]
        print(f"{name}: reset flags behind step 0 per optimiser step {out['resets_inside']}, |h0|max {out['h0_max']}")
    for s, rec in enumerate(steps):
        aux = {}
        ref = supervised_gradients_f64(rec, make_net, make_cell, aux=aux)
        twin = supervised_gradients_f64(rec, make_net, make_cell, dtype=torch.float32)
        assert list(ref) == list(rec["grads"])
        rows = {}
        for k, g in ref.items():
            top = g.abs().max().item()
            assert g.shape == rec["grads"][k].shape, k
            rows[k] = ((rec["grads"][k].double() - g).abs().max().item() / max(top, 1e-300), (twin[k].double() - g).abs().max().item() / max(top, 1e-300), top)
        norm = lambda gs: math.sqrt(sum((g.double() ** 2).sum().item() for g in gs.values()))
        m = dict(rows=rows, norm_ref=norm(ref), norm_used=math.sqrt(rec["clip_sqnorm"].item()), loss=aux["loss"],
                 terms=[aux["cloning_loss"]] + ([aux["symmetric_loss"]] if spec["symmetry"] else []), stats=(rec["stats"] / float(A * B)).tolist())
        if spec["symmetry"]:
            m["share"] = norm(aux["symmetric_grads"]) / m["norm_ref"]
        if name in CONTROLS:
            kw, k = CONTROLS[name]
            wrong = supervised_gradients_f64(rec, make_net, make_cell, **kw)[k]
            m["control"] = (rec["grads"][k].double() - wrong).abs().max().item() / wrong.abs().max().item()
        out["steps"].append(m)
        for k, (e, t, top) in rows.items():
            print(f"{name} step {s} {k}: error {e:.3e} of |ref|max {top:.3e}; fp32 twin {t:.3e}")
        print(f"{name} step {s}: norm {m['norm_ref']:.6f}, the clip's off by {abs(m['norm_used'] - m['norm_ref']) / m['norm_ref']:.2e} of it; loss terms {m['terms']}, stats / (12 B) {m['stats']}"
              + (f"; the symmetric term's share of the gradient's norm {m['share']:.3f}" if spec["symmetry"] else ""))
    if name == "student:default":  # what the iteration tests' check makes of the control's wrong gradient
        right, doubled = (_adam_stepped(steps[0], make_net, scale) for scale in (1.0, 2.0))
        out["adam"] = {k: ((doubled[k] - right[k]).abs().max().item(), (right[k] - steps[0]["params"][k].double()).abs().max().item(),
                           bool(torch.allclose(doubled[k], right[k], rtol=1e-3, atol=2e-6))) for k in right}
    return out


_PLANS = {}  # (plan, wgrad_terms) the default and the switch cases have resolved so far in this session


def check_case(m):
    name, plan, terms = m["name"], m["plan"], m["wgrad_terms"]
    if name == "student:default" or name.startswith("student:switch:"):  # no switch is silently ignored at this shape
        _PLANS[name] = (plan, terms)
        same = [k for k, p in _PLANS.items() if k != name and p == (plan, terms)]
        assert not same, (name, same)
    if m["expect"] is not None:
        assert (plan.fwd, plan.bwd, terms) == m["expect"], (name, plan, terms)
    assert all(plan.grouped[:-1])
    first, last = m["steps"][0], m["steps"][-1]
    # (d): conditions on the float64 reference
    assert all(top > 0 for st in m["steps"] for (_, _, top) in st["rows"].values()), name
    assert last["loss"] < first["loss"], (name, [st["loss"] for st in m["steps"]])
    if m["symmetry"]:
        assert all(st["share"] >= SHARE for st in m["steps"]), (name, [st["share"] for st in m["steps"]])
    if m["memory"]:
        assert all(n > 0 for n in m["resets_inside"]) and all(h > 1e-3 for h in m["h0_max"]), (name, m["resets_inside"], m["h0_max"])
        for st in m["steps"]:  # the cell's four tensors and the trunk's eight are among the compared
            assert {"memory.weight_ih", "memory.weight_hh", "memory.bias_ih", "memory.bias_hh"} <= set(st["rows"]) and len(st["rows"]) == 12
    # (a), (b), (c)
    missed = []
    for s, st in enumerate(m["steps"]):
        for k, (e, t, top) in st["rows"].items():
            if not e <= BOUNDS.get((name, k), (BOUND, None))[0]:
                missed.append((s, k, e, t))
        assert abs(st["norm_used"] - st["norm_ref"]) <= NORM_BOUND * st["norm_ref"], (name, s, st["norm_used"], st["norm_ref"])
        assert len(st["stats"]) == len(st["terms"])
        for got, want in zip(st["stats"], st["terms"]):
            assert want > 0 and abs(got - want) <= LOSS_BOUND * want, (name, s, st["stats"], st["terms"])
    assert not missed, (name, missed)
    for (case, k), (bound, twin_error) in BOUNDS.items():  # a bound of its own only above the twin's floor
        assert case in CASES and twin_error > TWIN_FLOOR and bound == 4 * twin_error, (case, k)
    # (e)
    if name in CONTROLS:
        k = CONTROLS[name][1]
        for s, st in enumerate(m["steps"]):
            print(f"{name} step {s}: against the wrong reference {CONTROLS[name][0]} {k} is off by {st['control']:.3e} ({st['control'] / BOUND:.1f} x the bound)")
        assert all(st["control"] > BOUND for st in m["steps"]), (name, [st["control"] for st in m["steps"]])
    if name == "student:default":
        for k, (diff, moved, close) in m["adam"].items():
            print(f"{name} {k}: three float64 Adam steps on the doubled hidden bias gradients end {diff:.3e} from the right ones (moved {moved:.3e}); allclose {close}")
        assert all(close and moved > 1e-5 for (_, moved, close) in m["adam"].values()), m["adam"]


@pytest.mark.parametrize("name", list(CASES))
def test_every_step_of_the_supervised_update_leaves_the_float64_gradient(name, teachers):
    check_case(run_case(name, teachers))


def test_a_switch_that_leaves_the_layer_kernels_is_the_value_error_resolve_plan_documents():
    """FUSED = False (a library GEMM in the passes) and FUSED_WGRAD = False (library weight gradients): SupervisedTrainer.resolve_plan refuses both."""
    from booster_gym_amd.utils.model import MLPTrainer, WeightClock, _mlp
    from booster_gym_amd.utils.optim import FlatAdam
    from booster_gym_amd.utils.supervised import SupervisedTrainer

    net = _mlp(47, (256, 128, 128), A).to(DEV)
    sup = SupervisedTrainer("distillation", net, FlatAdam(list(net.parameters()), lr=1.0e-3), WeightClock(), 256, 64)
    plan = sup.resolve_plan()
    assert (plan.fwd, plan.bwd, sup.wgrad_terms) == CASES["student:default"]["plan"]
    for k in ("FUSED", "FUSED_WGRAD"):
        saved = getattr(MLPTrainer, k)
        try:
            setattr(MLPTrainer, k, False)
            with pytest.raises(ValueError, match="distillation: a batch of 256 rows"):
                sup.resolve_plan()
        finally:
            setattr(MLPTrainer, k, saved)
    assert sup.resolve_plan() == plan
