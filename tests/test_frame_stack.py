"""The actor's observation history (env.frame_stack) without a GPU: the size rules of check_env_sizes, the update plan of a 141-input actor, the tiled
mirror maps, the C ABI's argument check and the host-side stack of tools/play_oracle.py against a numpy deque."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 187


def _cfg(H=None, num_obs=None, scan=False, **over):
    from booster_gym_amd.utils.config import load_cfg

    ov = {}
    if H is not None:
        ov["env.frame_stack"] = H
    if num_obs is not None:
        ov["env.num_observations"] = num_obs
    if scan:
        ov.update({"terrain.measure_heights": True, "env.num_privileged_obs": 14 + P})
    ov.update(over)
    return load_cfg("T1", ov)


def test_check_env_sizes_follows_the_frame_stack():
    from booster_gym_amd.envs.t1 import check_env_sizes, frame_stack_of

    assert frame_stack_of(_cfg()) == 1 and "frame_stack" in _cfg()["env"]  # (the shipped yaml names the key, at its default)
    check_env_sizes(_cfg(), 0)
    check_env_sizes(_cfg(3, 141), 0)
    check_env_sizes(_cfg(10, 470), 0)
    with pytest.raises(ValueError, match=r"env\.num_observations to 141"):
        check_env_sizes(_cfg(3, 47), 0)
    with pytest.raises(ValueError, match="47 observations"):  # without the key the rule is today's
        check_env_sizes(_cfg(None, 141), 0)
    with pytest.raises(ValueError, match=r"env\.frame_stack = 11 .*1 to 10.*470"):
        check_env_sizes(_cfg(11, 517), 0)
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"env\.frame_stack"):
            check_env_sizes(_cfg(bad, 47), 0)
    # with the default 187-point height scan: 47 H + 14 + 187 <= 512 holds up to H = 6
    check_env_sizes(_cfg(6, 282, scan=True), P)
    with pytest.raises(ValueError, match=r"env\.frame_stack = 7.*329 \+ 14 \+ 187.*measured_points_x.* = 530 exceeds 512"):
        check_env_sizes(_cfg(7, 329, scan=True), P)
    with pytest.raises(ValueError, match=r"env\.num_privileged_obs to 201"):
        check_env_sizes(_cfg(3, 141, **{"terrain.measure_heights": True}), P)


def test_plan_of_a_stacked_actor_is_the_per_layer_plan():
    """An actor of 141 inputs pads to 256 columns: per-layer forward and backward kernels, every hidden weight gradient in the grouped launch, the
    fused heads, no forward-ahead in the rollout (the critic of the height scan runs this plan today)."""
    from booster_gym_amd.utils.runner import pad_input, plan_update

    assert [pad_input(47 * h) for h in (1, 2, 3, 5, 6, 10)] == [64, 128, 256, 256, 512, 512]
    kin = pad_input(141)
    assert kin == 256
    sw = dict(split=0, fused=True, chain=True, chain_split=True, chain_split_bwd=True, chain_alternate=True, fused_wgrad=True, wgrad_split=9, one_stream=True,
              defer_finish=True, one_launch_tail=True, fused_opt=True, fused_head=True, fused_gae=True, chain_values=True, rollout_forward=True, dp_active=False)
    plan = plan_update(((141 + 14, 256, 256, 128, 1), pad_input(155)), ((141, 256, 128, 128, 12), kin), 24 * 4096, **sw)
    assert plan.actor.fwd == "layer" and plan.actor.bwd == "layer" and all(plan.actor.grouped[:-1])
    assert plan.critic.fwd == "layer" and plan.critic.bwd == "layer" and all(plan.critic.grouped[:-1])
    assert not plan.ahead and plan.fused_head and not plan.chain_values
    default = plan_update(((61, 256, 256, 128, 1), 64), ((47, 256, 128, 128, 12), 64), 24 * 4096, **sw)
    assert default.actor.fwd == default.critic.fwd == "chain_split" and default.ahead


def test_tiled_mirror_map_is_an_involution_and_mirrors_every_frame(flat_model):
    from booster_gym_amd.envs.mirror import mirror_maps

    axes = [int(a) for a in flat_model.joint_axis if int(a) != 0]
    q0 = np.zeros(12)
    src1, sign1, act_src, act_sign = mirror_maps(flat_model.dof_names, axes, q0, 47)
    for H in (2, 5, 10):
        src, sign, a2, s2 = mirror_maps(flat_model.dof_names, axes, q0, 47 * H, H)
        assert src.shape == sign.shape == (47 * H,) and src.dtype == np.int32
        assert np.array_equal(a2, act_src) and np.array_equal(s2, act_sign)
        x = np.random.default_rng(H).normal(size=(4, 47 * H))
        m = sign * x[:, src]
        assert np.array_equal(sign * m[:, src], x)  # applying it twice is the identity
        for k in range(H):
            assert np.array_equal(m[:, 47 * k : 47 * (k + 1)], sign1 * x[:, 47 * k : 47 * (k + 1)][:, src1]), k
    with pytest.raises(ValueError, match="141 observations"):
        mirror_maps(flat_model.dof_names, axes, q0, 141)
    with pytest.raises(ValueError, match="x 2 frames"):
        mirror_maps(flat_model.dof_names, axes, q0, 141, 2)


def test_env_create_rejects_a_frame_stack_out_of_range_without_gpu(flat_model):
    """bg_env_create checks cfg.frame_stack before it touches the device: -1 and 11 are argument errors.  A frame_stack of 0 is what every caller
    older than the field passes (a zero-initialised struct: tests/test_host_logic.py builds one and expects to reach the device check), so the
    library reads it as 1; the yaml key's 0 is a ValueError of check_env_sizes (above)."""
    import torch

    from booster_gym_amd import _lib

    lib = _lib.load()
    assert _lib.EnvCfg.frame_stack.offset + 4 <= C.sizeof(_lib.EnvCfg)
    m = flat_model
    d = _lib.ModelDesc(); d.num_bodies, d.num_dofs = 13, 12
    for b in range(13):
        d.parent[b], d.joint_axis[b], d.mass[b] = int(m.parent[b]), int(m.joint_axis[b]), float(m.mass[b])
    model = C.c_void_p()
    assert lib.bg_model_create(C.byref(d), C.byref(model)) == 0
    try:
        for H in (-1, 11):
            cfg = _lib.EnvCfg(); cfg.num_envs, cfg.decimation, cfg.sim_dt, cfg.frame_stack = 4, 10, 0.002, H
            env = C.c_void_p()
            assert lib.bg_env_create(C.byref(cfg), model, C.byref(env)) == -1 and b"frame_stack" in lib.bg_last_error(), H
        if not torch.cuda.is_available():
            for H in (0, 1, 10):  # in range: the call gets as far as the device
                cfg = _lib.EnvCfg(); cfg.num_envs, cfg.decimation, cfg.sim_dt, cfg.frame_stack = 4, 10, 0.002, H
                env = C.c_void_p()
                assert lib.bg_env_create(C.byref(cfg), model, C.byref(env)) == -3 and b"no HIP device" in lib.bg_last_error(), H
    finally:
        lib.bg_model_destroy(model)


def test_play_oracle_stack_matches_a_numpy_deque():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import play_oracle
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(3)
    for H in (1, 2, 5, 10):
        stack = play_oracle.FrameStack(H)
        dq = collections.deque([np.zeros(47)] * H, maxlen=H)  # the deploy-side deque: zero-initialised, newest last
        for step in range(40):
            if step in (13, 14, 30):  # a reset: the history is forgotten, the next observation is the only frame
                stack.reset()
                dq = collections.deque([np.zeros(47)] * H, maxlen=H)
            o = rng.normal(size=47)
            dq.append(o)
            row = stack.push(o)
            assert row.shape == (47 * H,) and np.array_equal(row, np.concatenate(list(dq))), (H, step)
            assert np.array_equal(row[-47:], o)
    layers = [(np.zeros((256, 141)), np.zeros(256))]
    assert play_oracle.actor_frames(layers) == 3 and play_oracle.actor_frames([(np.zeros((256, 47)), None)]) == 1
    with pytest.raises(ValueError, match="100 inputs"):
        play_oracle.actor_frames([(np.zeros((256, 100)), None)])
