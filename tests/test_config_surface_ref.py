"""The cases of parity_util.CONFIG_CASES are well-posed on the reference alone (no GPU): under each case, on flat ground, the float64 oracle
(oracle/task_ref.py + oracle/dyn_ref.c) against its own fp32 twin through the same StepParity procedure that tests/test_gpu_config_surface.py runs
the HIP env through.
  twin          the twin stays inside the tolerances the kernel is held to (explanations under StepParity's 1 % cap): the tolerances are wide
                enough for fp32 under these configs, so a kernel that misses them is wrong and not merely rounded differently
  non-vacuity   the reward terms a case activates or re-parameterises, and the total reward, are away from zero on the oracle's own outputs
  sensitivity   every key a case alters moves the output it governs by more than 10 x that output's tolerance in at least half of the envs, when
                that one key is put back to its shipped value: parity under the case then means that the kernel honours the key
The per-case figures are printed (pytest -s); profiles/config_surface_parity.txt keeps them."""
import numpy as np
import pytest

import parity_util as PU
from parity_util import CONFIG_CASES, N_CASE, REW_FLOOR, REW_TOL, SENS_FACTOR, SENS_SHARE, STATE_TOL, SWING_SHARE

_RESET_TOL = {"q": 2e-5, "root": 1e-5}  # test_reset_matches_oracle's bounds on the reset observation (joint columns) and on the root


def _differs(spec, out, ref, out_b, base):
    """Per env: does the output `spec` of the step under the case differ from the same step under the base by more than SENS_FACTOR x its tolerance?"""
    big = lambda a, b, tol: PU.rel_state(a, b) > SENS_FACTOR * tol
    kind = spec[0]
    if kind in ("obs", "priv"):
        i = 0 if kind == "obs" else 1
        return big(out[i][:, spec[1]:spec[2]], out_b[i][:, spec[1]:spec[2]], STATE_TOL[kind])
    if kind == "term":
        zero = np.zeros(ref.n)
        return PU.rel_reward(out[5].get(spec[1], zero), out_b[5].get(spec[1], zero)) > SENS_FACTOR * REW_TOL
    if kind == "total":
        return PU.rel_reward(out[2], out_b[2]) > SENS_FACTOR * REW_TOL
    if kind == "state":
        return (big(ref.root, base.root, STATE_TOL["root"]) | big(ref.q, base.q, STATE_TOL["dof_pos"]) | big(ref.qd, base.qd, STATE_TOL["dof_vel"])
                | big(out[6]["torques"], out_b[6]["torques"], STATE_TOL["torques"]))
    if kind == "root_vel":
        return big(ref.root[:, 7:13], base.root[:, 7:13], STATE_TOL["root"])
    if kind == "push":
        return big(ref.push, base.push, 1e-4)
    if kind == "swing":  # non-zero under the case's period, zero under the shipped one
        return (np.abs(out[5]["feet_swing"]) > REW_FLOOR) & (out_b[5]["feet_swing"] == 0.0)
    raise KeyError(kind)


def _base_oracle(case, key, model):
    """The oracle under the case with `key` alone back at its shipped value (same per-env parameter draws)."""
    from booster_gym_amd.utils.config import load_cfg

    ov = {"env.num_envs": N_CASE, "terrain.type": "plane"}
    ov.update({k: v for k, v in case["overrides"].items() if k != key})
    cfg = load_cfg("T1", ov)
    return PU.make_oracle(cfg, model, PU.host_params(cfg, model, N_CASE))


@pytest.mark.parametrize("name", list(CONFIG_CASES))
def test_case_is_well_posed_on_the_oracle(name):
    case = CONFIG_CASES[name]
    cfg, twin, ref = PU.make_oracle_pair(N_CASE, case["overrides"])
    model = ref.m
    step_keys = {k: v for k, v in case["keys"].items() if v[2] != "reset"}
    bases = {k: _base_oracle(case, k, model) for k in step_keys}
    hits = {k: [] for k in step_keys}
    ki, pi_, pd_ = PU.schedule(cfg, ref.dt)
    state = {}

    def before_step(s):  # (after StepParity.begin: the oracle holds the step's inputs)
        state["snap"], state["cnt"] = PU.snapshot(ref), ref.step_count + 1

    def after_step(s, sp, act, out, keep):
        cnt = state["cnt"]
        due = {"any": True, "limit": s == 0, "kick": cnt % ki == 0, "push_start": cnt % pi_ == 0, "push_end": cnt % pi_ == pd_, "pushed": bool(np.abs(ref.push).max() > 0)}
        for k, (_, outputs, when) in step_keys.items():
            if not due[when]:
                continue
            base = bases[k]
            PU.restore(base, state["snap"])
            out_b = base.step(act.astype(np.float64))
            d = np.zeros(ref.n, dtype=bool)
            for spec in outputs:
                d |= _differs(spec, out, ref, out_b, base)
            ok = keep & (out_b[3] == out[3])
            if when == "limit":
                ok[:PU.AIRBORNE.start] = False; ok[PU.AIRBORNE.stop:] = False
            hits[k].append(d[ok])

    summary, rec = PU.run_case(cfg, twin, ref, case["start_count"], arrange=PU.arrange_for(case),
                               before_step=before_step, after_step=after_step)
    sh = PU.shares(case, rec, "ref")
    sens = {k: (float(np.concatenate(v).mean()) if v else None) for k, v in hits.items()}
    # ---- reset(): the three init_* entries
    for k, (_, outputs, when) in case["keys"].items():
        if when != "reset":
            continue
        a, b = PU.make_oracle(cfg, model, ref.p), _base_oracle(case, k, model)
        a.reset(); b.reset()
        d = np.zeros(ref.n, dtype=bool)
        for _, attr in outputs:
            d |= PU.rel_state(getattr(a, attr), getattr(b, attr)) > SENS_FACTOR * _RESET_TOL[attr]
        sens[k] = float(d.mean())
    print(f"config-surface {name}: twin explained {summary['explained']} of {summary['env_steps']} {summary['by_reason']}")
    print(f"config-surface {name}: oracle active share per term {({k: round(v, 3) for k, v in sh['terms'].items()})} feet_swing {sh.get('feet_swing')}")
    print(f"config-surface {name}: oracle total positive {sh['total_positive']:.3f} zero {sh['total_zero']:.3f} non-zero {sh['total_nonzero']:.3f}")
    print(f"config-surface {name}: share of envs moved by more than {SENS_FACTOR:g} x tolerance per key {({k: (None if v is None else round(v, 3)) for k, v in sens.items()})}")
    PU.assert_not_vacuous(case, sh, f"{name} (oracle)")
    for k, v in sens.items():
        assert v is not None, f"{name}: no step of the window could show {k}"
        need = SWING_SHARE if case["keys"][k][1] == [("swing",)] else SENS_SHARE
        assert v >= need, f"{name}: putting {k} back to its shipped value moves its output in {v:.3f} of the envs only (needs {need})"


def test_every_mode_of_apply_rand_occurs_at_an_observation_site_and_at_a_state_site():
    from booster_gym_amd.utils.utils import rand_spec

    mode = lambda k: rand_spec(PU.NOISE_KEYS[k][0])[0]
    obs = {mode("noise." + k) for k in ("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel", "height")}
    st = {mode("randomization." + k) for k in ("kick_lin_vel", "kick_ang_vel", "push_force", "push_torque", "init_dof_pos", "init_base_pos_xy", "init_base_lin_vel_xy")}
    assert obs == {0, 1, 2, 3, 4} and st == {0, 1, 2, 3, 4}, (obs, st)
