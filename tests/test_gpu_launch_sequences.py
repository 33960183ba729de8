"""The library entry points that two training iterations call, in order, against the record of tests/golden/make_launch_sequences.py
(tests/golden/launch_sequences.json): the estimator's Runner, the Distiller with each of its keys, and a PPO Runner with each form of its optimiser
step (bg_update_tail; bg_reduce_group + bg_optimizer_step; bg_adam_step + bg_adapt_lr; a recurrent actor's cell in the grouped launch).  The
other tests count launches and compare results with float64 restatements to rtol 1e-3; a lost clock tick or two launches swapped can pass both."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recipe():
    spec = importlib.util.spec_from_file_location("make_launch_sequences", os.path.join(GOLDEN, "make_launch_sequences.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECIPE = _recipe()
with open(os.path.join(GOLDEN, "launch_sequences.json")) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def teacher_by_frames(tmp_path_factory):
    return RECIPE.teachers(str(tmp_path_factory.mktemp("teachers")))


def test_the_record_holds_every_case():
    assert sorted(WANT) == sorted(RECIPE.CASES) and all(len(v) == RECIPE.ITERATIONS and all(v) for v in WANT.values())


@pytest.mark.parametrize("case", list(RECIPE.CASES))
def test_two_iterations_call_the_recorded_entry_points_in_order(case, teacher_by_frames):
    got, _ = RECIPE.record(case, teacher_by_frames)
    for it, (g, w) in enumerate(zip(got, WANT[case])):
        first = next((k for k, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        assert g == w, f"{case}, iteration {it}: {len(g)} calls against {len(w)} recorded; first difference at call {first}: {g[first:first + 3]} against {w[first:first + 3]}"
