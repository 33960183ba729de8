"""Record the library entry points that two training iterations call, in order, for the supervised paths: a Runner with estimator.enabled and a
Distiller plain, with student_frame_stack 3, teacher_action_prob 0.5, symmetric_coef 10, student_memory 128 and student_memory 128 with
teacher_action_prob 0.5; and for the forms of PPO's optimiser step: a Runner under the default plan (bg_update_tail), with _one_launch_tail = False
(bg_reduce_group, the weight gradients' finish, bg_optimizer_step), with _fused_opt = False (bg_adam_step, bg_adapt_lr) and with
algorithm.rnn_hidden_size 128 (the GRU trainer in the grouped launch and among the mirrors).  tests/test_gpu_launch_sequences.py holds the tree against the committed record, so a refactor of the host code cannot
drop, add or reorder a launch (a clock tick lost or an order swapped passes the float64 comparisons of the other tests).

The cases run at 128 envs under the `_cfg` helpers of tests/test_gpu_estimator.py and tests/test_gpu_distill.py with the latter's seeded teacher, no BG_*
variable set, through public names only (Runner(cfg=), begin_training, train_iteration; Distiller(cfg=), begin, train_iteration; .model, .student,
.optimizer, .buffer), so the same file records any tree of the project:

  python tests/golden/make_launch_sequences.py [--tree DIR] [--out tests/golden/launch_sequences.json]

--tree: the checkout to record (default: the one this file lies in); the committed record is the parent commit's of the change that added the case.
Every case is recorded twice, in two orders, and the two must agree (nothing in a sequence depends on what ran before in the process).  Per case
it also prints a SHA-256 over the parameters, the optimisers' flat / exp_avg / exp_avg_sq and every buffer after the two iterations: equal between
two trees exactly when they computed the same bits (not committed: a later compiler may change them).  Needs a GPU.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys
import tempfile

ITERATIONS = 2
PPO = {"estimator.enabled": False}
# a Runner: (overrides of its config, attributes set on it before the first iteration)
RUNNER_CASES = {"runner_estimator": ({}, {}),
                "ppo_default_plan": (PPO, {}),
                "ppo_tail_as_three_launches": (PPO, {"_one_launch_tail": False}),
                "ppo_separate_optimizer_launches": (PPO, {"_fused_opt": False}),
                "ppo_rnn_hidden_size_128": ({**PPO, "algorithm.rnn_hidden_size": 128}, {})}
CASES = {**RUNNER_CASES,  # (every other case: the overrides of a Distiller's config)
         "distill_plain": {},
         "distill_student_frame_stack_3": {"distillation.student_frame_stack": 3},
         "distill_teacher_action_prob": {"distillation.teacher_action_prob": 0.5},
         "distill_symmetric_coef_10": {"distillation.symmetric_coef": 10.0},
         "distill_student_memory_128": {"distillation.student_memory": 128},
         "distill_student_memory_128_teacher_action_prob": {"distillation.student_memory": 128, "distillation.teacher_action_prob": 0.5}}


@contextlib.contextmanager
def spy():
    """Every entry point of the library but bg_last_error and bg_version wrapped to append its name to the list this yields."""
    from booster_gym_amd import _lib

    lib, seq = _lib.load(), []
    names = [n for n in _lib.SYMBOLS if n not in ("bg_last_error", "bg_version")]
    saved = {n: getattr(lib, n) for n in names}

    def wrap(fn, name):
        def call(*a):
            seq.append(name)
            return fn(*a)
        return call

    for n in names:
        setattr(lib, n, wrap(saved[n], n))
    try:
        yield seq
    finally:
        for n in names:
            setattr(lib, n, saved[n])


def teachers(tmp):
    """The seeded teacher checkpoints of tests/test_gpu_distill.py by env.frame_stack: its own two frames, and one frame for a recurrent student."""
    from test_gpu_distill import H, _save_teacher

    return {f: _save_teacher(os.path.join(tmp, f"teacher_h{f}.pth"), f) for f in (H, 1)}


def build(case, teacher_by_frames):
    """The trainer of a case, begun: a Runner or a Distiller."""
    over = CASES[case]
    if case in RUNNER_CASES:
        from test_gpu_estimator import _runner

        r = _runner(1, 128, **over[0])
        for k, x in over[1].items():
            assert hasattr(r, k), k
            setattr(r, k, x)
        return r
    from test_gpu_distill import H, _Rec, _cfg

    from booster_gym_amd.utils.distill import Distiller

    frames = 1 if "distillation.student_memory" in over else H
    d = Distiller(cfg=_cfg(teacher_by_frames[frames], frames, **{"env.num_envs": 128, **over}))
    d.begin(recorder=_Rec())
    return d


def digest(t):
    """SHA-256 over the model's or the student's state dict, the optimisers' flat / exp_avg / exp_avg_sq and every buffer."""
    import torch

    net = t.model if hasattr(t, "model") else t.student
    opts = [t.optimizer] + ([t._est_opt] if getattr(t, "_est", None) is not None else [])
    h = hashlib.sha256()
    for x in list(net.state_dict().values()) + [v for o in opts for v in (o.flat, o.exp_avg, o.exp_avg_sq)] + [t.buffer[k] for k in sorted(t.buffer.names())]:
        h.update(x.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def record(case, teacher_by_frames):
    """([the entry points of iteration 0, of iteration 1], digest) of a case."""
    import torch

    t = build(case, teacher_by_frames)
    its = []
    with spy() as seq:
        for it in range(ITERATIONS):
            del seq[:]
            t.train_iteration(it)
            its.append(list(seq))
    torch.cuda.synchronize()
    return its, digest(t)


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=here)
    ap.add_argument("--out", default=os.path.join(here, "tests", "golden", "launch_sequences.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    stale = sorted(k for k in os.environ if k.startswith("BG_"))
    assert not stale, f"unset {stale}: the record is the default switches'"
    import booster_gym_amd

    print("recording " + os.path.dirname(os.path.abspath(booster_gym_amd.__file__)), flush=True)
    ck = teachers(tempfile.mkdtemp(prefix="bg_launch_sequences_"))
    out = {}
    for case in list(CASES) + list(reversed(CASES)):
        seqs, sha = record(case, ck)
        assert out.setdefault(case, seqs) == seqs, f"{case}: the sequence depends on what ran before it"
        print(f"{case}: {' + '.join(str(len(s)) for s in seqs)} calls, sha256 {sha}", flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("written " + a.out)
