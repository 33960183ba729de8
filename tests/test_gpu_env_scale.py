"""The stages of the simulator where one env's result depends on how many other envs there are and on where it sits in the launch, PAST their first
pass: persistent grids on a second and third trip (env_step_body_kernel, sim_substep_body_kernel, forward_dynamics_body_kernel), the compaction of
the gated forward dynamics over more than one block of masks, the exact-count resampling's block offsets and chunked scan, the command curriculum's
grid under contention and the episode statistics' float atomics.  Sizes: parity_util.SCALE_N = 33,000 envs (1,032 blocks of 32, the last of 8: three
trips of a 512-workgroup grid, five compaction blocks, more than 32,768 listed envs) and parity_util.RESAMPLE_NS; tests/test_env_scale_ref.py holds
them to the constants in csrc/bg_sim.hip.

References: (1) the same kernel at 256 envs, which the float64 oracle already holds, bit for bit: env e of the large run carries the state and the
per-env parameters (every randomisation on, copied with set_field) of env src[e] of the small run, src a fixed-seed shuffled map onto the source
envs, so the same state lands beside other neighbours, in another lane pair, in a ragged block; (2) the float64 oracle on 64 envs of the large run
chosen by position (parity_util.spot_positions) at the tolerances of tests/test_gpu_dynamics.py / test_gpu_sim_calls.py, nothing excused; (3) the
oracle's own restatement of the coupling, oracle.task_ref.resample_commands, for the resampling and curriculum stages.
Every figure printed with the prefix "env-scale:" is recorded in profiles/env_scale_parity.txt."""
import math

import numpy as np
import pytest
import torch

import parity_util as PU
from parity_util import SCALE_N as N, SCALE_SRC as NS
from test_gpu_dynamics import _states

pytestmark = pytest.mark.gpu

GATE = {"rewards.terminate_height": 0.05}
K = PU.kernel_constants()  # ENVS_PER_BLOCK, BODY_GRID, RS_BLOCK as csrc/bg_sim.hip has them
EPB, BODY_GRID = K["ENVS_PER_BLOCK"], K["BODY_GRID"]


def _env(n, terrain="plane", over=None):
    from booster_gym_amd.envs import T1
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", dict({"env.num_envs": n, "terrain.type": terrain}, **(over or {})))
    return cfg, T1(cfg)


def _tdict(env, terrain):
    if terrain == "plane":
        return None
    t = env.terrain
    return dict(height_field_raw=t.height_field_raw, hscale=t.horizontal_scale, vscale=t.vertical_scale, border_px=t.border_pixels)


def _same_terrain(small, big, terrain):
    if terrain != "plane":
        assert np.array_equal(small.terrain.height_field_raw, big.terrain.height_field_raw), "the height field depends on the env count"


def _dev(env, a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(env.device)


def _bits(a, b, what):
    """Bitwise equality of two float tensors (NaN patterns included)."""
    a, b = a.contiguous(), b.contiguous()
    same = a.view(torch.int32) == b.view(torch.int32)
    if not bool(same.all()):
        rows = torch.nonzero(~same.reshape(same.shape[0], -1).all(dim=1))[:, 0]
        raise AssertionError(f"{what}: {len(rows)} of {same.shape[0]} envs differ in bits, first at env {int(rows[0])}, last at env {int(rows[-1])}")


# ================================================================== A. forward dynamics
def _fd(env, tab, src=None):
    pick = (lambda a: a) if src is None else (lambda a: a[src])
    qacc = env.forward_dynamics(*[_dev(env, pick(tab[k])) for k in ("root", "q", "qd", "tau", "w")])
    return qacc.clone(), env.get_field("feet_contact_forces").clone()


def _fd_setup(flat_model, terrain, gated):
    from oracle.dyn_ref import DynRef

    cfg, small = _env(NS, terrain, GATE if gated else None)
    _, big = _env(N, terrain, GATE if gated else None)
    _same_terrain(small, big, terrain)
    dyn = DynRef(flat_model, feet_edge_pos=cfg["asset"]["feet_edge_pos"], terrain=_tdict(small, terrain))

    def shift(root):  # as tests/test_gpu_dynamics.py places its states on the rough strips
        if terrain != "plane":
            root[:, 0] += 20.0; root[:, 1] += 5.0
            root[:, 2] += np.array([dyn.terrain_height(x, y) for x, y in root[:, :2]])

    return small, big, dyn, PU.fd_tables(dyn, flat_model, _states, shift)


@pytest.mark.parametrize("terrain", ["plane", "trimesh"])
def test_gated_forward_dynamics_past_one_pass(flat_model, terrain):
    """bg_env_forward_dynamics with the trunk-low gate at 33,000 envs: all envs listed (the walk of forward_dynamics_body_kernel wraps: 33,000 >
    32 x 1,024 list entries; five blocks of aba_compact_kernel, the last one partial, their bases from atomics in any order), then a sparse batch on
    the same env object (the ticket of the last workgroup must have emptied the list; per-block masks empty, partial and full, every compaction block
    with entries), then all listed again.  qacc and feet_contact_forces of EVERY env are the bits of the 256-env gated run through src; 64 envs by
    position against the float64 oracle.  Which states kernel A leaves to kernel B is restated on the host (parity_util.fd_listed: trunk below the
    gate, or leg clearance negative); by that rule not every "crossed_gated" / "low" state is listed, so the all-listed batch draws from the source
    envs that have such a state (parity_util.fd_tables: pool)."""
    small, big, dyn, tabs = _fd_setup(flat_model, terrain, True)
    placement = PU.sparse_listed(N, EPB)
    pool = tabs["pool"]
    src = PU.shuffled_src((~placement).astype(int), [pool[pool % 2 == 0], pool[pool % 2 == 1]])
    assert set(src.tolist()) == set(pool.tolist()) and tabs["all"]["listed"][src].all() and np.array_equal(tabs["sparse"]["listed"][src], placement)
    params = PU.copy_params(small, big, src)
    tsrc = torch.as_tensor(src, device=big.device)
    want = {k: _fd(small, tabs[k]) for k in ("all", "sparse")}
    must = np.nonzero(placement)[0][:: max(1, int(placement.sum()) // 24)]
    spots = PU.spot_positions(N, must=must)
    for launch, k in enumerate(("all", "sparse", "all")):
        qacc, cf = _fd(big, tabs[k], src)
        _bits(qacc, want[k][0][tsrc], f"{terrain} launch {launch} ({k}): qacc")
        _bits(cf, want[k][1][tsrc], f"{terrain} launch {launch} ({k}): feet_contact_forces")
        assert torch.isfinite(qacc).all()
        if launch < 2:
            worst, ncontact = PU.fd_spot_check(dyn, tabs[k], src, spots, qacc.cpu().numpy(), cf.cpu().numpy().reshape(N, 2, 3), params)
            print(f"env-scale: A gated forward dynamics {terrain} {k}: listed {tabs[k]['listed'][src].mean():.4f} of {N} envs, {len(pool)} source envs, "
                  f"oracle spot check on {len(spots)} envs: worst error / tolerance {worst:.3f}, {ncontact} with a contact")


def test_one_kernel_forward_dynamics_at_the_same_size(flat_model):
    """The all-listed batch's size through an env created WITHOUT the gate, at the shipped heights: forward_dynamics_kernel<false> alone, the crossed-leg
    states of tests/test_gpu_dynamics.py (narrow phase through LDS), bitwise against its own 256-env run, 64 envs against the oracle at 5e-4."""
    small, big, dyn, tabs = _fd_setup(flat_model, "plane", False)
    src = PU.shuffled_src(np.zeros(N, dtype=int), [np.arange(NS)])
    params = PU.copy_params(small, big, src)
    tsrc = torch.as_tensor(src, device=big.device)
    want = _fd(small, tabs["crossed"])
    qacc, cf = _fd(big, tabs["crossed"], src)
    _bits(qacc, want[0][tsrc], "ungated: qacc")
    _bits(cf, want[1][tsrc], "ungated: feet_contact_forces")
    spots = PU.spot_positions(N)
    worst, ncontact = PU.fd_spot_check(dyn, tabs["crossed"], src, spots, qacc.cpu().numpy(), cf.cpu().numpy().reshape(N, 2, 3), params)
    print(f"env-scale: A one-kernel forward dynamics plane crossed: oracle spot check on {len(spots)} envs: worst error / tolerance {worst:.3f}, "
          f"{ncontact} with a contact")


# ================================================================== B. gated bg_sim_simulate
def test_gated_simulate_past_one_pass(flat_model):
    """Ten gym.simulate calls with the gate on at 33,000 envs, a body wrench pending on calls 0 and 5 and none on the others: sim_substep_kernel
    leaves the low envs to sim_substep_body_kernel, whose 512 workgroups take up to three trips (parity_util.low_placement: blocks b, b + 512,
    b + 1,024 for b in 0, 3, 7; one block low whole, one with a single low env, the ragged last block).  Root, dof, contact and body tensors of every
    env are the bits of the 256-env run through src after every call; after the last one 64 envs by position against the oracle's step from the
    state before it: the velocity part of tests/test_gpu_sim_calls.simulate_parity only (accelerations implied by the velocities, that file's
    tolerance for the source's family; its seed and families) -- positions, contact forces and body rows are held by the bitwise comparison with the
    256-env run, which that file compares with the oracle.  Source envs: every fourth one a "low" state (trunk more than 5 cm under the gate, so that it stays low through
    the ten calls), the others standing states."""
    from booster_gym_amd.envs.gym_calls import GymCalls, gymapi, gymtorch
    from oracle.dyn_ref import DynRef

    cfg, small = _env(NS, "plane", GATE)
    _, big = _env(N, "plane", GATE)
    dyn = DynRef(flat_model, feet_edge_pos=cfg["asset"]["feet_edge_pos"])
    gate = float(cfg["contact"]["body_gate_height"])
    root, q, qd, tau, bf, bt, is_low = PU.sim_sources(flat_model, _states, gate)
    placement = PU.low_placement(N, EPB, BODY_GRID)
    src = PU.shuffled_src((~placement).astype(int), [np.nonzero(is_low)[0], np.nonzero(~is_low)[0]])
    params = PU.copy_params(small, big, src)
    tsrc = torch.as_tensor(src, device=big.device)

    def bind(env, pick):
        n = env.num_envs
        gym = GymCalls(env)
        sim = gym.sim
        t = dict(root=gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim)), dof=gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim)).view(n, 12, 2),
                 contact=gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim)).view(n, 13, 3),
                 body=gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim)).view(n, 13, 13))
        t["root"].copy_(_dev(env, pick(root))); t["dof"][..., 0] = _dev(env, pick(q)); t["dof"][..., 1] = _dev(env, pick(qd))
        gym.set_dof_actuation_force_tensor(sim, gymtorch.unwrap_tensor(_dev(env, pick(tau))))
        wrench = (_dev(env, pick(bf)), _dev(env, pick(bt)))
        return gym, sim, t, wrench

    gs, ss, ts, ws = bind(small, lambda a: a)
    gb, sb, tb, wb = bind(big, lambda a: a[src])
    spots = PU.spot_positions(N, must=np.nonzero(placement)[0][::3])
    counts, _ = PU.block_masks(placement, EPB)
    for call in range(10):
        if call in (0, 5):
            gs.apply_rigid_body_force_tensors(ss, gymtorch.unwrap_tensor(ws[0]), gymtorch.unwrap_tensor(ws[1]), gymapi.LOCAL_SPACE)
            gb.apply_rigid_body_force_tensors(sb, gymtorch.unwrap_tensor(wb[0]), gymtorch.unwrap_tensor(wb[1]), gymapi.LOCAL_SPACE)
        low_now = (tb["root"][:, 2] < gate).cpu().numpy()  # (the plane: the terrain height is zero)
        per_trip = [int(PU.block_masks(low_now, EPB)[0][t * BODY_GRID:(t + 1) * BODY_GRID].sum()) for t in range(3)]
        assert min(per_trip) >= 1, f"call {call}: low envs per trip of the body kernel {per_trip}"
        if call == 0:
            assert np.array_equal(low_now, placement)
        before = (tb["root"][spots].cpu().numpy().astype(np.float64), tb["dof"][spots].cpu().numpy().astype(np.float64))
        gs.simulate(ss); gb.simulate(sb)
        for k in ("root", "dof", "contact", "body"):
            _bits(tb[k], ts[k][tsrc], f"call {call}: {k} tensor")
    assert torch.isfinite(tb["root"]).all() and torch.isfinite(tb["body"]).all()
    # the oracle's step from the state before the last call (no wrench pending there)
    after = (tb["root"][spots].cpu().numpy().astype(np.float64), tb["dof"][spots].cpu().numpy().astype(np.float64))
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    worst = 0.0
    for j, e in enumerate(spots):
        i = int(src[e])
        par = dict(mass_scale=f32(params["mass_scale"][e]), com_off=f32(params["com_offset"][e]).reshape(13, 3), foot_mat=f32(params["foot_material"][e]).reshape(6))
        vel_g = np.concatenate([after[0][j, 7:13], after[1][j][:, 1]])
        tol = PU.FAMILY_TOL["low" if is_low[i] else True]
        err = PU.sim_implied_error(dyn, before[0][j], before[1][j][:, 0], before[1][j][:, 1], f32(tau[i]), None, None, par, vel_g)
        assert err < tol, f"env {e} (source {i}, {'low' if is_low[i] else 'standing'}): implied acceleration error {err:.2e}, tolerance {tol:g}"
        worst = max(worst, err / tol)
    print(f"env-scale: B gated simulate plane: low {placement.mean():.5f} of {N} envs ({int(placement.sum())}; blocks with low envs {int((counts > 0).sum())}), "
          f"low envs per trip at the last call {per_trip}, oracle spot check on {len(spots)} envs after call 10: worst error / tolerance {worst:.3f}")


# ================================================================== D. exact-count resampling
NO_END = {"rewards.terminate_height": -10.0, "rewards.terminate_vel": 1.0e9, "rewards.episode_length_s": 1000.0}  # nobody is reset inside the window


def _oracle_seed(cfg):
    return (int(cfg["basic"]["seed"]) & 0xFFFFFFFF) | (1 << 32)  # oracle.task_ref.T1Ref.seed at rank 0


def _check_resampled(cfg, env, obs, flags, r, what):
    """Still set, its size, and the consistency of commands, gait frequency and observation entries 6..10 of the envs `flags` against the oracle's
    resample_commands output `r`."""
    nz, cm = cfg["normalization"], cfg["commands"]
    K = int(flags.sum())
    cmd, gf, o = env.commands.cpu().numpy(), env.get_field("gait_frequency").cpu().numpy()[:, 0], obs.cpu().numpy()
    still = flags & (gf == 0.0)
    assert np.array_equal(np.nonzero(still)[0], np.nonzero(r["still"] & flags)[0]), f"{what}: the still set differs from the oracle's"
    assert int(still.sum()) == int(float(np.float32(cm["still_proportion"])) * K), f"{what}: {int(still.sum())} still envs of K = {K}"
    assert (cmd[still] == 0.0).all() and (o[still][:, 9:11] == 0.0).all() if K else True
    if K:
        assert PU.rel_state(cmd[flags], r["commands"][flags]).max() < 1e-5, f"{what}: commands"
        assert PU.rel_state(gf[flags, None], r["gait_frequency"][flags, None]).max() < 1e-5, f"{what}: gait frequency"
        scale = np.array([nz["lin_vel"], nz["lin_vel"], nz["ang_vel"]])
        assert PU.rel_state(o[flags][:, 6:9], cmd[flags].astype(np.float64) * scale).max() < 1e-5, f"{what}: observation entries 6..8"
        moving = flags & ~still
        assert (np.abs(np.hypot(o[moving][:, 9], o[moving][:, 10]) - 1.0) < 1e-5).all(), f"{what}: gait clock entries of a moving env"
    return K, int(still.sum())


@pytest.mark.parametrize("n", PU.RESAMPLE_NS)
def test_exact_count_resampling_past_one_block(n):
    """parallel.exact_still_count at 70,000 envs (274 resample blocks: two per thread of resample_offsets_kernel, threads 137.. with an empty chunk)
    and 600 (three blocks, ragged tail): reset() (every env, stream offset 64), then single steps whose resampling envs are none / the last env
    alone / one per block / blocks 1 and 3 whole / a random 30 % / all.  Flags from the device's own cmd_resample_time change; the still set equals
    oracle.task_ref.resample_commands' as a set and has int(float32(still_proportion) K) members; commands, gait frequency and the observation's
    entries 6..10 agree with one another.  Nothing else of the step is compared."""
    from oracle.task_ref import resample_commands

    cfg, env = _env(n, "plane", dict(NO_END, **{"parallel.exact_still_count": True}))
    seed, rb = _oracle_seed(cfg), K["RS_BLOCK"]
    obs, _ = env.reset()
    r = resample_commands(np.ones(n, dtype=bool), 0, 64, None, cfg, seed)
    sizes = [_check_resampled(cfg, env, obs, np.ones(n, dtype=bool), r, "reset")]
    rng = np.random.default_rng(12)
    nb = (n + rb - 1) // rb
    one_per_block = np.zeros(n, dtype=bool)
    one_per_block[[b * rb + int(rng.integers(0, min(rb, n - b * rb))) for b in range(nb)]] = True
    two_blocks = np.zeros(n, dtype=bool); two_blocks[rb:2 * rb] = True; two_blocks[3 * rb:4 * rb] = True
    last = np.zeros(n, dtype=bool); last[-1] = True
    patterns = {"none": np.zeros(n, dtype=bool), "last": last, "one_per_block": one_per_block, "blocks_1_and_3": two_blocks[:n], "random_30": rng.random(n) < 0.3,
                "all": np.ones(n, dtype=bool)}
    act = torch.zeros(n, 12, device=env.device)
    for name, want in patterns.items():
        ep = env.get_field("episode_length_buf")
        ct = ep + 5000
        ct[torch.as_tensor(want, device=ct.device)] -= 4999  # == episode_length_buf after this step's increment
        env.set_field("cmd_resample_time", ct)
        step = env.common_step_counter
        obs, _, done, _ = env.step(act)
        assert not bool(done.any())
        flags = env.get_field("cmd_resample_time").cpu().numpy()[:, 0] != ct.cpu().numpy()[:, 0]
        assert np.array_equal(flags, want), f"{name}: {int(flags.sum())} envs resampled, {int(want.sum())} arranged"
        r = resample_commands(flags, step, 0, None, cfg, seed)
        sizes.append(_check_resampled(cfg, env, obs, flags, r, name))
    print(f"env-scale: D exact-count resampling at {n} envs: (K, still) per pattern reset, {', '.join(patterns)}: {sizes}")


# ================================================================== E. same-step curriculum under contention
def _curriculum_setup(n, same_step, update_rate=None):
    over = {"commands.curriculum": True, "parallel.exact_still_count": True, "parallel.same_step_curriculum": same_step, "rewards.terminate_height": -10.0,
            "rewards.terminate_vel": 1.0e9, "commands.lin_vel_x_toler": 1.0e9, "commands.lin_vel_y_toler": 1.0e9, "commands.ang_vel_yaw_toler": 1.0e9}
    if update_rate is not None:
        over["commands.update_rate"] = update_rate
    cfg, env = _env(n, "plane", over)
    env.reset()
    rng = np.random.default_rng(3)
    prob0 = rng.uniform(0.0, 0.8, (21, 21)).astype(np.float32); prob0[10, 10] = 1.0   # as test_gpu_env.test_command_curriculum_matches_oracle
    env.curriculum_prob = torch.tensor(prob0)
    # 6,000 envs end a long episode in the next step: 4,500 on one interior cell, 500 on each of two corner cells (clipped stencils), 500 at random
    ending = np.sort(rng.choice(n, size=6000, replace=False))
    lin, ang = rng.integers(-10, 11, n), rng.integers(-10, 11, n)
    grp = rng.permutation(6000)
    cx, cy = np.unravel_index(np.argmin(prob0[1:20, 1:20]), (19, 19))  # the interior cell with the smallest start value: room for 4,500 adds below 1
    lin[ending[grp[:4500]]], ang[ending[grp[:4500]]] = int(cx) + 1 - 10, int(cy) + 1 - 10
    lin[ending[grp[4500:5000]]], ang[ending[grp[4500:5000]]] = 10, 10
    lin[ending[grp[5000:5500]]], ang[ending[grp[5000:5500]]] = -10, 10
    env.set_field("env_curriculum_level_lin", torch.tensor(lin, dtype=torch.int32)); env.set_field("env_curriculum_level_ang", torch.tensor(ang, dtype=torch.int32))
    max_ep = int(math.ceil(cfg["rewards"]["episode_length_s"] / env.dt))
    ep = env.get_field("episode_length_buf")
    ep[torch.as_tensor(ending, device=ep.device), 0] = max_ep  # one increment past the limit: timed out in the next step
    env.set_field("episode_length_buf", ep)
    env.set_field("cmd_resample_time", torch.full_like(ep, 9000))
    return cfg, env, prob0, ending, lin, ang


def _host_grid(prob0, lin, ang, who, rate):
    """min(prob0, 1) plus the five-cell stencils of the envs `who` (t1.py:391-413), float64, and the number of adds into every cell."""
    g, adds = np.minimum(prob0.astype(np.float64), 1.0), np.zeros(prob0.shape, dtype=np.int64)
    x, y = lin[who] + 10, ang[who] + 10
    for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        xx, yy = x + dx, y + dy
        ok = (xx >= 0) & (xx < g.shape[0]) & (yy >= 0) & (yy < g.shape[1])
        np.add.at(adds, (xx[ok], yy[ok]), 1)
    return g + adds * float(np.float32(rate)), adds


@pytest.mark.parametrize("n,update_rate", [(33000, None), (70000, 1.0e-4)])
def test_same_step_curriculum_under_contention(n, update_rate):
    """commands.curriculum with both exact modes: 6,000 episodes end in ONE step by time-out, successful by construction (the four tracking
    tolerances at 1e9: success = time-out in a finite state, asserted on the outputs), 4,500 of them on one grid cell.  The grid after the step is
    min(prob0, 1) plus the host's sum of update_rate over the five-cell stencils, per cell within (adds into the cell) x 2^-24 x (value) x 2: the
    rounding of sequential fp32 adds of one constant, doubled; the getter clamps at 1 like curriculum_prob.clamp_, so both sides are clamped.  At the
    shipped update_rate (0.1) the contended cells all pass 1; the 70,000-env case lowers it to 1e-4, where the busiest cell stays below 1 and a lost
    add shows.  The episode ends at episode_length_buf = ceil(episode_length_s / dt): the time-out tests `>` after the increment.  Commands and levels
    of the envs that resampled in the step: resample_commands fed the grid read back after the step (levels exact, commands 1e-5).  episode_stats
    against the host's sums over the same step: counts exact, length and reward sums within (flushed envs) x 2^-24 relative, doubled."""
    from oracle.task_ref import resample_commands

    cfg, env, prob0, ending, lin, ang = _curriculum_setup(n, True, update_rate)
    rate = cfg["commands"]["update_rate"]
    env.episode_stats(reset=True)
    steps0, sums0 = env.get_field("episode_steps").cpu().numpy()[:, 0].astype(np.float64), env.get_field("episode_sums").cpu().numpy()[:, 0].astype(np.float64)
    step = env.common_step_counter
    obs, rew, done, extras = env.step(torch.zeros(n, 12, device=env.device))
    d, tout = done.cpu().numpy().astype(bool), extras["time_outs"].cpu().numpy().astype(bool)
    stats = env.episode_stats(reset=False).cpu().numpy().astype(np.float64)
    assert stats[-1] == 0 and np.array_equal(np.nonzero(d)[0], ending) and np.array_equal(d, tout), "successes = time-outs in a finite state = the arranged envs"
    want, adds = _host_grid(prob0, lin, ang, ending, rate)
    got = env.curriculum_prob.cpu().numpy().astype(np.float64)
    bound = adds * 2.0 ** -24 * want * 2.0 + 1e-30
    ratio = np.abs(got - np.minimum(want, 1.0)) / bound
    ratio[(adds == 0) & (got == np.minimum(want, 1.0))] = 0.0
    assert ratio.max() <= 1.0, f"grid cell {np.unravel_index(ratio.argmax(), ratio.shape)}: error {ratio.max():.2f} x its bound"
    assert adds.max() >= 4500 and (update_rate is None or want[adds.argmax() // 21, adds.argmax() % 21] < 1.0)
    # the draws of this step's resamplers read the grid AFTER this step's updates
    flags = env.get_field("cmd_resample_time").cpu().numpy()[:, 0] != 9000
    assert np.array_equal(flags, d)
    r = resample_commands(flags, step, 0, got, cfg, _oracle_seed(cfg))
    lv = np.stack([env.get_field("env_curriculum_level_lin").cpu().numpy()[:, 0], env.get_field("env_curriculum_level_ang").cpu().numpy()[:, 0]], axis=1)
    assert np.array_equal(lv[flags, 0], r["lin"][flags]) and np.array_equal(lv[flags, 1], r["ang"][flags]), "curriculum levels of the resampled envs"
    assert PU.rel_state(env.commands.cpu().numpy()[flags], r["commands"][flags]).max() < 1e-5
    stale = resample_commands(flags, step, 0, prob0, cfg, _oracle_seed(cfg))
    moved = float(((stale["lin"] != r["lin"]) | (stale["ang"] != r["ang"]))[flags].mean())
    _check_resampled(cfg, env, obs, flags, r, "curriculum step")
    # episode statistics: float atomics of 6,000 flushes
    k = len(ending)
    rw = rew.cpu().numpy().astype(np.float64)
    len_sum, rew_sum = float((steps0[d] + 1).sum()), float((sums0[d] + rw[d]).sum())
    rel = 2.0 * k * 2.0 ** -24
    assert stats[0] == k
    assert abs(stats[1] - len_sum) <= rel * len_sum and abs(stats[2] - rew_sum) <= rel * max(abs(rew_sum), float(np.abs(sums0[d] + rw[d]).sum()))
    print(f"env-scale: E same-step curriculum at {n} envs, update_rate {rate}: {k} successes, busiest cell {int(adds.max())} adds, grid error / derived bound "
          f"{ratio.max():.3f}, levels that the pre-step grid would have drawn differently {moved:.3f}, episode length sum error {abs(stats[1] - len_sum):.3g} "
          f"of {len_sum:.6g}, reward sum error {abs(stats[2] - rew_sum):.3g} of {rew_sum:.6g}")
    assert moved > 0.05, "the grid before and after the step draw the same levels: the step's update is not seen by this comparison"


def test_next_step_curriculum_draws_come_from_the_snapshot():
    """same_step_curriculum off at 33,000 envs: the 6,000 envs that resample in the step of their time-out draw from the grid as it was BEFORE the step
    (curr_read), and the envs that resample in the NEXT step from the grid after it: the copy of curr into curr_read at the end of a step."""
    from oracle.task_ref import resample_commands

    n = 33000
    cfg, env, prob0, ending, lin, ang = _curriculum_setup(n, False)
    seed = _oracle_seed(cfg)
    levels = lambda: np.stack([env.get_field("env_curriculum_level_lin").cpu().numpy()[:, 0], env.get_field("env_curriculum_level_ang").cpu().numpy()[:, 0]], axis=1)
    act = torch.zeros(n, 12, device=env.device)
    step = env.common_step_counter
    env.step(act)
    flags = env.get_field("cmd_resample_time").cpu().numpy()[:, 0] != 9000
    assert int(flags.sum()) == 6000
    grid1 = env.curriculum_prob.cpu().numpy()
    old, new = resample_commands(flags, step, 0, prob0, cfg, seed), resample_commands(flags, step, 0, grid1, cfg, seed)
    lv = levels()
    assert np.array_equal(lv[flags, 0], old["lin"][flags]) and np.array_equal(lv[flags, 1], old["ang"][flags]), "the step's own draws did not read the snapshot"
    assert float(((old["lin"] != new["lin"]) | (old["ang"] != new["ang"]))[flags].mean()) > 0.05
    # next step: another 5,000 envs resample (no episode ends), from the grid the first step left
    rng = np.random.default_rng(4)
    nxt = np.zeros(n, dtype=bool); nxt[rng.choice(np.nonzero(~flags)[0], size=5000, replace=False)] = True
    ep = env.get_field("episode_length_buf")
    ct = env.get_field("cmd_resample_time")
    ct[torch.as_tensor(nxt, device=ct.device)] = ep[torch.as_tensor(nxt, device=ct.device)] + 1
    env.set_field("cmd_resample_time", ct)
    step = env.common_step_counter
    _, _, done, _ = env.step(act)
    assert not bool(done.any())
    flags2 = env.get_field("cmd_resample_time").cpu().numpy()[:, 0] != ct.cpu().numpy()[:, 0]
    assert np.array_equal(flags2, nxt)
    new, old = resample_commands(flags2, step, 0, grid1, cfg, seed), resample_commands(flags2, step, 0, prob0, cfg, seed)
    lv = levels()
    assert np.array_equal(lv[flags2, 0], new["lin"][flags2]) and np.array_equal(lv[flags2, 1], new["ang"][flags2]), "the next step's draws did not read the grid the step left"
    assert PU.rel_state(env.commands.cpu().numpy()[flags2], new["commands"][flags2]).max() < 1e-5
    moved = float(((old["lin"] != new["lin"]) | (old["ang"] != new["ang"]))[flags2].mean())
    print(f"env-scale: E snapshot hand-over at {n} envs: next-step levels that the stale grid would have drawn differently {moved:.3f}")
    assert moved > 0.05


# ================================================================== C. gated env step
QUIET = {f"noise.{k}": None for k in ("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel", "height")}  # observation noise is keyed by the env index
STEP_FIELDS = PU.FIELDS + ["episode_sums", "episode_steps"]
LOW_EVERY = 32  # every 32nd source env is laid on its side under the gate


def _heights(env, xy):
    return env.terrain.terrain_heights(np.c_[xy, np.zeros(len(xy))]).cpu().numpy().astype(np.float64)


def _gated_step_case(terrain, extra, tc=False):
    """Four env steps with the gate on (rewards.terminate_height 0.3 under contact.body_gate_height 0.45, as tests/test_gpu_config_surface.py's gated
    case) at 33,000 envs against the 256-env run through src.  The small run is reset and settled for 15 steps; every 32nd source env is then laid on
    its side between the two heights (test_gpu_config_surface.LOW); six source envs, one of them low, time out in the first step; no command
    is resampled inside the window (resampling draws are keyed by the env index); observation noise is off, kicks and pushes fall outside the window.
    The whole state (parity_util.FIELDS) and the per-env parameters go to the large env with set_field through src, actions are tiled through src.
    Low envs sit as parity_util.low_placement puts them: env_step_body_kernel's workgroups 0, 3 and 7 have work on three trips.
    Per step, for the envs whose source env has not been reset before it: done, time_outs, reward and every reward term are the small run's bits
    (pre-reset quantities); for those not reset in it either, root / dof state, torques, foot forces, observation and privileged rows as well.  An env
    is left out from the step after its source env's reset on: the reset draws are keyed by the env index."""
    over = dict(QUIET, **{"rewards.terminate_height": 0.3}, **extra)
    cfg, small = _env(NS, terrain, over)
    _, big = _env(N, terrain, over)
    _same_terrain(small, big, terrain)
    gate = float(cfg["contact"]["body_gate_height"])
    assert small._cfg_c.body_gate_height > small._cfg_c.terminate_height and big._cfg_c.terrain_curriculum == int(tc)
    small.reset(); big.reset()
    g = torch.Generator(device="cpu").manual_seed(5)
    for _ in range(15):
        small.step((0.2 * torch.rand(NS, 12, generator=g) - 0.1).to(small.device))  # (larger random targets topple the robots inside the window)
    rng = np.random.default_rng(31)
    low_src = np.arange(NS) % LOW_EVERY == 0
    root = small.get_field("root_states").cpu().numpy()
    root[low_src, 2] = _heights(small, root[low_src, :2]) + rng.uniform(0.32, 0.42, int(low_src.sum()))
    root[low_src, 3:7] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
    root[low_src, 7:13] = 0.0
    small.set_field("root_states", torch.from_numpy(root).float())
    max_ep = int(math.ceil(cfg["rewards"]["episode_length_s"] / small.dt))
    ep = small.get_field("episode_length_buf")
    ep[:6, 0] = max_ep  # timed out in the window's first step; source env 0 is a low one
    small.set_field("episode_length_buf", ep)
    small.set_field("cmd_resample_time", torch.full_like(ep, 20000))
    placement = PU.low_placement(N, EPB, BODY_GRID)
    src = PU.shuffled_src((~placement).astype(int), [np.nonzero(low_src)[0], np.nonzero(~low_src)[0]])
    tsrc = torch.as_tensor(src, device=big.device)
    PU.copy_params(small, big, src)
    if tc:
        big.terrain_levels = small.terrain_levels[tsrc]
    for k in STEP_FIELDS:
        big.set_field(k, small.get_field(k)[tsrc])
    big.common_step_counter = small.common_step_counter
    alive = np.ones(NS, dtype=bool)
    seen = {"reset": np.zeros(NS, dtype=bool), "low_reset": 0, "tout": 0, "levels_checked": 0, "levels_moved": 0}
    for s in range(4):
        r0 = big.get_field("root_states").cpu().numpy().astype(np.float64)
        low_now = r0[:, 2] - _heights(big, r0[:, :2]) < gate
        per_trip = [int(PU.block_masks(low_now, EPB)[0][t * BODY_GRID:(t + 1) * BODY_GRID].sum()) for t in range(3)]
        assert min(per_trip) >= 1, f"step {s}: low envs per trip of the body kernel {per_trip}"
        if s == 0:
            assert np.array_equal(low_now, placement)
        rs0 = small.get_field("root_states").cpu().numpy().astype(np.float64)
        low_small = rs0[:, 2] - _heights(small, rs0[:, :2]) < gate
        if tc:
            lv0, cols, o0 = big.terrain_levels.cpu().numpy(), big.terrain_types.cpu().numpy(), big.get_field("env_origins").cpu().numpy().astype(np.float64)
            cmd0 = big.commands.cpu().numpy().astype(np.float64)
        act = 0.6 * torch.rand(NS, 12, generator=g) - 0.3
        os_, rs_, ds_, es_ = small.step(act.to(small.device))
        ob, rb, db, eb = big.step(act[torch.as_tensor(src)].to(big.device))
        d_small = ds_.cpu().numpy().astype(bool)
        a_big = torch.as_tensor(alive[src], device=big.device)
        k_big = torch.as_tensor((alive & ~d_small)[src], device=big.device)
        pre = {"done": (db, ds_), "time_outs": (eb["time_outs"], es_["time_outs"]), "reward": (rb, rs_)}
        pre.update({f"reward term {k}": (eb["rew_terms"][k], es_["rew_terms"][k]) for k in es_["rew_terms"]})
        for what, (b, sm) in pre.items():
            if b.dtype == torch.float32:
                _bits(b[a_big], sm[tsrc][a_big], f"step {s}: {what}")
            else:
                assert torch.equal(b[a_big], sm[tsrc][a_big]), f"step {s}: {what}"
        post = {"observation": (ob, os_), "privileged observation": (eb["privileged_obs"], es_["privileged_obs"])}
        post.update({k: (big.get_field(k), small.get_field(k)) for k in ("root_states", "dof_pos", "dof_vel", "torques", "feet_contact_forces")})
        for what, (b, sm) in post.items():
            _bits(b[k_big], sm[tsrc][k_big], f"step {s}: {what}")
        assert torch.isfinite(ob).all()
        seen["reset"] |= d_small & alive
        seen["low_reset"] += int((d_small & alive & low_small).sum())
        seen["tout"] += int((es_["time_outs"].cpu().numpy().astype(bool) & alive).sum())
        if tc:
            lv1 = big.terrain_levels.cpu().numpy()
            assert int(big.terrain_level_sum().item()) == int(lv1.sum()), f"step {s}: terrain level sum"
            t = cfg["terrain"]
            d = np.linalg.norm(r0[:, :2] - o0[:, :2], axis=1)
            far, near = 0.5 * t["terrain_length"], np.linalg.norm(cmd0[:, :2], axis=1) * 0.5 * cfg["rewards"]["episode_length_s"]
            up = d > far
            want = np.maximum(lv0 + up.astype(int) - (~up & (d < near)).astype(int), 0)
            sure = (np.abs(d - far) > 0.1) & (np.abs(d - near) > 0.1) & (want < t["num_levels"])  # (one step moves a robot by centimetres)
            rr = db.cpu().numpy().astype(bool) & sure
            assert np.array_equal(lv1[rr], want[rr]), f"step {s}: terrain levels of the reset envs"
            assert np.array_equal(lv1[~db.cpu().numpy().astype(bool)], lv0[~db.cpu().numpy().astype(bool)])
            seen["levels_checked"] += int(rr.sum()); seen["levels_moved"] += int((lv1[rr] != lv0[rr]).sum())
        alive &= ~d_small
    share = float(seen["reset"].mean())
    print(f"env-scale: C gated env step {terrain} {extra}: low {placement.mean():.5f} of {N} envs, source envs reset inside the window {share:.4f} "
          f"({int(seen['reset'].sum())} of {NS}; {seen['low_reset']} of them low, {seen['tout']} time-outs), compared to the end {float(alive[src].mean()):.4f} of {N} envs, "
          f"low envs per trip at the last step {per_trip}" + (f", terrain levels checked {seen['levels_checked']}, moved {seen['levels_moved']}" if tc else ""))
    assert 0.01 <= share <= 0.10, f"{share:.3f} of the source envs were reset inside the window"
    assert seen["tout"] >= 6 and seen["low_reset"] >= 1, seen
    if tc:
        assert seen["levels_checked"] >= 100 and seen["levels_moved"] >= 1, seen


@pytest.mark.parametrize("state_dtype", ["fp32", "fp16"])
def test_gated_env_step_past_one_pass(state_dtype):
    """env_step_kernel<., true> + env_step_body_kernel on the plane, state stored in fp32 and in fp16: _gated_step_case."""
    _gated_step_case("plane", {"sim.state_dtype": state_dtype})


def test_gated_env_step_with_the_terrain_curriculum_past_one_pass():
    """The terrain-curriculum instantiation on the rough terrain: additionally terrain_level_sum() equals the sum of the levels after every step, and
    the levels of the reset envs are legged_gym's rule (bg_env.h) applied on the host to the pre-step root position, origin and command (as
    tests/test_gpu_config_surface.py states it; envs within 0.1 m of one of the rule's two distances, or wrapping past the top level, left to
    tests/test_gpu_terrain_curriculum.py).  A large env's origin is the centre of the tile of ITS column at its source env's level, so the robots
    stand far from their origins and most resets move a level."""
    _gated_step_case("trimesh", {"terrain.curriculum": True, "terrain.num_levels": 6, "terrain.max_init_level": 3}, tc=True)
