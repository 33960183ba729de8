"""The fused HIP env step against the float64 oracle AWAY from the values envs/T1.yaml ships: reward scales and soft_* factors (with the three
terms that ship at -0.0), normalisation, every mode of apply_rand at the noise / kick / push / reset sites, control.decimation, sim.dt, gravity,
PD gains and the contact constants (parity_util.CONFIG_CASES).  The procedure, the tolerances and the 1 % cap on explained env-steps are those of
test_gpu_env.test_step_matches_oracle (parity_util.run_case is that test's body); tests/test_config_surface_ref.py shows on the oracle alone that
its fp32 twin stays inside them under these cases and that every altered key moves its output by more than 10 x the tolerance, so parity here
means that the kernel honours the key.  Each case also asserts on the env's OWN outputs that the compared rewards are away from zero."""
import numpy as np
import pytest
import torch

import parity_util as PU
from parity_util import CONFIG_CASES, N_CASE

pytestmark = pytest.mark.gpu

LOW = slice(28, 36)  # envs laid on their side with the trunk between rewards.terminate_height = 0.3 and contact.body_gate_height (the gated case)


def _run(name, terrain, extra=None, arrange=None, **kw):
    case = CONFIG_CASES[name]
    cfg, env, ref = PU.make_pair(terrain, N_CASE, dict(case["overrides"], **(extra or {})))
    for t in case["new_terms"]:
        assert t in env.extras["rew_terms"], f"{t} has a non-zero scale and is missing from extras['rew_terms']"
    base = PU.arrange_for(case)

    def arr(e):
        if base is not None:
            base(e)
        if arrange is not None:
            arrange(e)

    hooks = {k: (lambda s, *a, f=f: f(s, cfg, env, ref, *a)) for k, f in kw.items()}
    summary, rec = PU.run_case(cfg, env, ref, case["start_count"], arrange=arr, **hooks, fp16=cfg["sim"]["state_dtype"] == "fp16",
                               state_tol={"root": 3e-3, "dof_pos": 3e-3, "dof_vel": 1e-2} if cfg["sim"]["state_dtype"] == "fp16" else None)
    sh_env, sh_ref = PU.shares(case, rec, "env"), PU.shares(case, rec, "ref")
    print(f"config-surface gpu {name} {terrain} {extra or ''}: StepParity {summary}")
    print(f"config-surface gpu {name} {terrain} {extra or ''}: env shares {sh_env}")
    print(f"config-surface gpu {name} {terrain} {extra or ''}: oracle shares {sh_ref}")
    PU.assert_not_vacuous(case, sh_env, f"{name} (env)")
    PU.assert_not_vacuous(case, sh_ref, f"{name} (oracle)")
    return cfg, env, ref, summary


@pytest.mark.parametrize("name,terrain", [("rewards_positive", "plane"), ("rewards_signed", "plane"), ("noise", "plane"), ("physics", "plane"),
                                          ("combined", "plane"), ("combined", "trimesh")])
def test_step_matches_oracle_under_case(name, terrain):
    _run(name, terrain)


def test_fp16_state_step_matches_oracle_under_the_combined_case():
    """sim.state_dtype: fp16 with every key of the combined case: the oracle's stored state is rounded as the kernel's is (quantize_state_fp16), the
    tolerances are those of test_gpu_env.test_fp16_state_step_matches_oracle."""
    cfg, env, ref, _ = _run("combined", "trimesh", {"sim.state_dtype": "fp16"})
    assert env._cfg_c.state_fp16 == 1
    q = env.dof_pos.cpu().numpy()
    assert np.array_equal(q, q.astype(np.float16).astype(np.float32))


def test_gated_kernels_match_oracle_under_the_combined_case():
    """rewards.terminate_height: 0.3 below contact.body_gate_height: env_step_kernel<..., true> hands the envs whose trunk is low to
    env_step_body_kernel, which then evaluates the altered task logic too.  The envs of LOW are laid on their side (as the terrain-curriculum test
    lays its robots) with the trunk between the two heights; they fall through 0.3 inside the window and are reset there."""
    seen = {"low": 0, "reset": 0}

    def arrange(env):
        rng = np.random.default_rng(31)
        root = env.get_field("root_states")
        root[LOW, 2] = torch.as_tensor(rng.uniform(0.31, 0.38, LOW.stop - LOW.start), dtype=torch.float32)
        root[LOW, 3:7] = torch.tensor([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)], dtype=torch.float32)
        root[LOW, 7:13] = 0.0
        env.set_field("root_states", root)

    def before_step(s, cfg, env, ref):
        seen["low"] += int((ref.root[LOW, 2] < cfg["contact"]["body_gate_height"]).sum())

    def after_step(s, cfg, env, ref, sp, act, out, keep):
        seen["reset"] += int(out[3][LOW].sum())

    cfg, env, ref, _ = _run("combined", "plane", {"rewards.terminate_height": 0.3}, arrange=arrange, before_step=before_step, after_step=after_step)
    assert env._cfg_c.body_gate_height > env._cfg_c.terminate_height
    assert seen["low"] >= 8 and seen["reset"] >= 4, seen  # the body kernel had envs to step, and reset some of them below the altered height


def test_terrain_curriculum_step_matches_oracle_under_the_combined_case():
    """terrain.curriculum: true (the TC instantiation) on the rough terrain: the oracle has no level state, so before each step every env's origin in
    the oracle is set to the centre of the tile legged_gym's rule would move it to if it were reset in that step (test_gpu_terrain_curriculum._rule);
    after the step the reset envs' levels and origins on the device must be those."""
    L = 6
    st = {"checked": 0, "moved": 0}

    def before_step(s, cfg, env, ref):
        t = cfg["terrain"]
        lv, cols = env.terrain_levels.cpu().numpy(), env.terrain_types.cpu().numpy()
        o = env.get_field("env_origins").cpu().numpy().astype(np.float64)
        d = np.linalg.norm(ref.root[:, :2] - o[:, :2], axis=1)
        far, near = 0.5 * t["terrain_length"], np.linalg.norm(ref.cmd[:, :2], axis=1) * 0.5 * cfg["rewards"]["episode_length_s"]
        up = d > far
        down = ~up & (d < near)
        st["lv0"], st["cols"] = lv, cols
        st["want"] = np.maximum(lv + up.astype(int) - down.astype(int), 0)
        st["sure"] = (np.abs(d - far) > 0.1) & (np.abs(d - near) > 0.1) & (st["want"] < L)  # (one step moves a robot by centimetres)
        ref.p["origins"] = env.terrain.tile_centres(np.minimum(st["want"], L - 1), cols).astype(np.float32).astype(np.float64)

    def after_step(s, cfg, env, ref, sp, act, out, keep):
        r = out[3].astype(bool) & keep & st["sure"]
        lv1 = env.terrain_levels.cpu().numpy()
        assert np.array_equal(lv1[r], st["want"][r]), (s, lv1[r], st["want"][r])
        o1 = env.get_field("env_origins").cpu().numpy()
        c = env.terrain.tile_centres(lv1, st["cols"])
        assert np.allclose(o1[r, :2], c[r, :2], atol=1e-5) and np.allclose(o1[r, 2], c[r, 2], atol=1e-4)
        k = ~out[3].astype(bool) & keep
        assert np.array_equal(lv1[k], st["lv0"][k])
        st["checked"] += int(r.sum()); st["moved"] += int((lv1[r] != st["lv0"][r]).sum())

    cfg, env, ref, _ = _run("combined", "trimesh", {"terrain.curriculum": True, "terrain.num_levels": L, "terrain.max_init_level": 3},
                            before_step=before_step, after_step=after_step)
    assert env._cfg_c.terrain_curriculum == 1
    assert st["checked"] >= 6 and st["moved"] >= 1, st  # the forced time-outs were reset through the level rule, and some of them changed level
    assert int(env.terrain_level_sum().item()) == int(env.terrain_levels.sum().item())


@pytest.mark.parametrize("name,terrain", [("noise", "plane"), ("combined", "plane"), ("combined", "trimesh")])
def test_reset_matches_oracle_under_case(name, terrain):
    """test_gpu_env.test_reset_matches_oracle's checks where the three init_* entries act: a uniform scaling of the default pose, a gaussian spawn
    offset, no spawn velocity."""
    cfg, env, ref = PU.make_pair(terrain, 64, CONFIG_CASES[name]["overrides"])
    obs, extras = env.reset()
    o_ref, p_ref = ref.reset()
    PU.assert_close(obs.cpu().numpy(), o_ref, 2e-5, frac=1.0, what="reset obs")
    PU.assert_close(extras["privileged_obs"].cpu().numpy(), p_ref, 2e-5, frac=1.0, what="reset privileged obs")
    PU.assert_close(env.root_states.cpu().numpy(), ref.root, 1e-5, frac=1.0, what="reset root")
    PU.assert_close(env.dof_pos.cpu().numpy(), ref.q, 1e-5, frac=1.0, what="reset dof_pos")
    assert (env.get_field("delay_steps").cpu().numpy()[:, 0] == ref.delay).all()
    assert (env.get_field("cmd_resample_time").cpu().numpy()[:, 0] == ref.cmd_time).all()
    # the entries did act: the spawn velocity is exactly zero, the default pose is scaled (not shifted), the spawn offset is not the shipped +-1 m box's
    root, q = env.root_states.cpu().numpy(), env.dof_pos.cpu().numpy()
    assert (root[:, 7:9] == 0).all()
    assert np.abs(q[:, [1, 2, 5]]).max() == 0 and np.abs(q[:, 3] - 0.4).max() > 1e-3
    assert ref.delay.max() < cfg["control"]["decimation"]
