"""CPU companion of tests/test_gpu_env_scale.py: what keeps the GPU cases honest without a GPU.
  * the sizes of the cases exceed the thresholds of the stages they are aimed at, with the constants READ from csrc/bg_sim.hip: a later change of
    BODY_GRID, RS_BLOCK, ENVS_PER_BLOCK, the 1,024 of bg_env_forward_dynamics or the 256 of aba_compact_kernel fails here instead of silently turning
    the GPU cases back into first-pass tests;
  * the placement tables hit what they claim (which workgroup takes which trip, which masks are empty / partial / full);
  * oracle.task_ref.resample_commands equals the in-line code it replaced, and its vectorised keyed permutation is a permutation;
  * the oracle's fp32 twin satisfies, on the spot-check states of the forward-dynamics and simulate cases, the tolerances the GPU test imposes."""
import numpy as np
import pytest

import parity_util as PU
from oracle import task_ref as TR
from parity_util import SCALE_N as N, SCALE_SRC as NS
from test_gpu_dynamics import _states

K = PU.kernel_constants()
EPB = K["ENVS_PER_BLOCK"]


def test_constants_are_found_and_sizes_cross_their_thresholds():
    assert K["COMPACT_BLOCK"] == K["COMPACT_GRID_DIV"]  # one mask per thread of aba_compact_kernel
    nb = -(-N // EPB)
    assert N % EPB not in (0,) and N - (nb - 1) * EPB < EPB, "no ragged last block"
    # env_step_body_kernel / sim_substep_body_kernel: grid min(nb, BODY_GRID), block b served on trip b // BODY_GRID
    assert -(-nb // K["BODY_GRID"]) >= 3, "kernel B's workgroups take fewer than three trips"
    # aba_compact_kernel: one block per COMPACT_BLOCK masks
    ncb = -(-nb // K["COMPACT_BLOCK"])
    assert ncb >= 2 and nb % K["COMPACT_BLOCK"] != 0, "one compaction block, or no partial one"
    # forward_dynamics_body_kernel: grid min(nb, FD_GRID) workgroups of EPB list entries
    assert N > EPB * K["FD_GRID"] and nb > K["FD_GRID"], "the list walk does not wrap"
    # spot positions sit on both sides of the boundaries that matter
    assert EPB * K["BODY_GRID"] == 16384 and EPB * K["FD_GRID"] == 32768
    spots = PU.spot_positions(N)
    assert {0, N - 1, 16383, 16384, 32767, 32768} <= set(spots.tolist()) and set(range((nb - 1) * EPB, N)) <= set(spots.tolist()) and len(spots) == 64
    assert len({int(e) // EPB // K["BODY_GRID"] for e in spots}) == 3
    # resampling: per = ceil(nblocks / RS_BLOCK) blocks per thread of resample_offsets_kernel
    big, small = PU.RESAMPLE_NS
    rb = K["RS_BLOCK"]
    nrb = -(-big // rb)
    per = -(-nrb // rb)
    assert per >= 2 and -(-nrb // per) < rb, "no thread of the offsets scan has two blocks, or none has an empty chunk"
    assert (nrb, per, -(-nrb // per)) == (274, 2, 137)
    nrs = -(-small // rb)
    assert nrs >= 3 and -(-nrs // rb) == 1 and small % rb != 0


def test_sparse_listed_placement_hits_what_it_claims():
    listed = PU.sparse_listed(N, EPB)
    counts, rows = PU.block_masks(listed, EPB)
    for b in PU.SPARSE_ONE:
        assert counts[b] == (rows[b] if b in PU.SPARSE_FULL else 1), b
    for b in PU.SPARSE_FULL:
        assert counts[b] == rows[b], b
    assert rows[-1] == N - (len(rows) - 1) * EPB < EPB and counts[-1] == rows[-1]
    assert (counts == 0).sum() > 100 and ((counts > 0) & (counts < rows)).sum() > 100 and (counts == rows).sum() == len(PU.SPARSE_FULL)
    # every block of aba_compact_kernel has entries (its base atomic fires), and none of them is full
    cb = K["COMPACT_BLOCK"]
    per_cb = [int(counts[i:i + cb].sum()) for i in range(0, len(counts), cb)]
    assert len(per_cb) == 5 and min(per_cb) >= 1 and len(counts) % cb == 8
    assert 0.02 < listed.mean() < 0.05
    # the masks next to the boundaries of the compaction blocks and of kernel B's grid carry one entry each
    assert {0, cb - 1, cb, 2 * cb - 1, 2 * cb, K["FD_GRID"] - 1, K["FD_GRID"]} <= set(PU.SPARSE_ONE)


def test_low_placement_hits_what_it_claims():
    g = K["BODY_GRID"]
    low = PU.low_placement(N, EPB, g)
    counts, rows = PU.block_masks(low, EPB)
    holding = set(np.nonzero(counts)[0].tolist())
    assert holding == {b + t * g for b in PU.LOW_BASES for t in range(3)}
    # workgroup b of the persistent grid serves blocks b, b + g, b + 2 g: three trips with work for workgroups 0, 3 and 7
    for b in PU.LOW_BASES:
        assert [int(counts[b + t * g] > 0) for t in range(3)] == [1, 1, 1]
    assert counts[3 + g] == rows[3 + g] == EPB and counts[7] == 1
    last = len(counts) - 1
    assert last == 7 + 2 * g and rows[last] < EPB and 0 < counts[last] <= rows[last]
    # a class of source envs must fit into the low positions
    assert low.sum() >= 16


def test_shuffled_src_covers_every_source_env_and_is_no_tiling_in_order():
    listed = PU.sparse_listed(N, EPB)
    pool = np.arange(NS)
    src = PU.shuffled_src((~listed).astype(int), [pool[pool % 2 == 0], pool[pool % 2 == 1]])
    assert set(src.tolist()) == set(pool.tolist())
    assert (src[listed] % 2 == 0).all() and (src[~listed] % 2 == 1).all()
    assert (np.diff(src) == 1).mean() < 0.05 and np.array_equal(src, PU.shuffled_src((~listed).astype(int), [pool[pool % 2 == 0], pool[pool % 2 == 1]]))
    # neighbours: the same source env sits in even and odd lane pairs and in many different blocks
    where = np.nonzero(src == 1)[0]
    assert len(set((where % EPB).tolist())) > 8 and len(set((where // EPB).tolist())) > 8


# ------------------------------------------------------------------ the refactored resample block against the in-line code it replaced
def _old_inline(rs, step, so, grid, cfg, seed, exact):
    """The resample block of T1Ref._reset_and_observe as it stood before resample_commands (Python loops per env and per position)."""
    cm, n = cfg["commands"], len(rs)
    dt = cfg["control"]["decimation"] * cfg["sim"]["dt"]
    env = np.arange(n, dtype=np.uint32)
    c0u, _ = TR.rand4(seed, env, step, so + TR.RS_CMD0)
    c1u, _ = TR.rand4(seed, env, step, so + TR.RS_CMD1)
    new = np.stack([cm["lin_vel_x"][0] + (cm["lin_vel_x"][1] - cm["lin_vel_x"][0]) * c0u[:, 0],
                    cm["lin_vel_y"][0] + (cm["lin_vel_y"][1] - cm["lin_vel_y"][0]) * c0u[:, 1],
                    cm["ang_vel_yaw"][0] + (cm["ang_vel_yaw"][1] - cm["ang_vel_yaw"][0]) * c0u[:, 2]], axis=1).astype(np.float64)
    lin = ang = None
    if cm.get("curriculum", False):
        cru, _ = TR.rand4(seed, env, step, so + TR.RS_CURR)
        p = np.minimum(grid, 1.0).astype(np.float32).reshape(-1)
        total = np.float32(0.0)
        for v in p:
            total = np.float32(total + v)
        cum = np.cumsum(p, dtype=np.float32)
        target = cru[:, 0] * total
        idx = np.minimum(np.array([int(np.searchsorted(cum, t, side="right")) for t in target]), p.size - 1)
        lin, ang, new = TR.curriculum_commands(idx, cru[:, 1].astype(np.float64) - 0.5, 2.0 * cru[:, 2].astype(np.float64) - 1.0,
                                               cru[:, 3].astype(np.float64) - 0.5, cm, grid.shape[1])
    gf = (cm["gait_frequency"][0] + (cm["gait_frequency"][1] - cm["gait_frequency"][0]) * c0u[:, 3]).astype(np.float64)
    if exact:
        ids = np.nonzero(rs)[0]
        Kn = len(ids)
        m = int(float(np.float32(cm["still_proportion"])) * Kn)
        key = TR._mix32(np.uint32(seed & 0xFFFFFFFF) ^ TR._mix32(np.uint32((step + 0x632BE5AB * (so + 1)) & 0xFFFFFFFF)))
        still = np.zeros(n, dtype=bool)
        for pos, e in enumerate(ids):
            still[e] = TR.keyed_perm(pos, Kn, key) < m
    else:
        still = c1u[:, 0] < np.float32(cm["still_proportion"])
    new[still] = 0.0; gf[still] = 0.0
    lo, hi = int(cm["resampling_time_s"][0] / dt), int(cm["resampling_time_s"][1] / dt)
    add = lo + np.minimum((c1u[:, 1] * np.float32(hi - lo)).astype(np.int64), hi - lo - 1) if hi > lo else np.full(n, lo)
    return dict(commands=new, gait_frequency=gf, still=still, add=add, lin=lin, ang=ang)


@pytest.mark.parametrize("n", [96, 1000])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("curriculum", [False, True])
def test_resample_commands_equals_the_inline_code_it_replaced(n, exact, curriculum):
    from booster_gym_amd.utils.config import load_cfg

    cfg = load_cfg("T1", {"env.num_envs": n, "terrain.type": "plane", "commands.curriculum": curriculum, "parallel.exact_still_count": exact})
    rng = np.random.default_rng(n)
    grid = rng.uniform(0.0, 1.3, (21, 21))
    seed = 42 | (1 << 32)
    for rs, step, so in ((np.ones(n, dtype=bool), 0, 64), (rng.random(n) < 0.3, 17, 0), (np.arange(n) == n - 1, 250, 0), (np.zeros(n, dtype=bool), 3, 0)):
        old, new = _old_inline(rs, step, so, grid, cfg, seed, exact), TR.resample_commands(rs, step, so, grid, cfg, seed)
        for k in ("commands", "gait_frequency", "still", "add") + (("lin", "ang") if curriculum else ()):
            assert np.array_equal(old[k], new[k]), (k, step)
        if exact:
            assert int((new["still"] & rs).sum()) == int(float(np.float32(cfg["commands"]["still_proportion"])) * int(rs.sum())) and not (new["still"] & ~rs).any()


@pytest.mark.parametrize("Kn", [1, 2, 3, 255, 256, 257, 65536, 70000])
def test_vectorised_keyed_perm_is_a_permutation(Kn):
    for key in (0, 0x9E3779B9, 0xFFFFFFFF):
        out = TR.keyed_perm_vec(np.arange(Kn), Kn, key)
        assert np.array_equal(np.sort(out), np.arange(Kn))
        for p in ([0, Kn - 1, Kn // 2] if Kn > 300 else range(Kn)):
            assert int(out[p]) == TR.keyed_perm(p, Kn, key)


# ------------------------------------------------------------------ the fp32 twin on the spot-check states
def _dyn_pair(flat_model, terrain):
    from booster_gym_amd.utils.config import load_cfg
    from booster_gym_amd.utils.terrain import Terrain
    from oracle.dyn_ref import DynRef

    cfg = load_cfg("T1", {"env.num_envs": NS, "terrain.type": terrain, "rewards.terminate_height": 0.05})
    tdict = None
    if terrain != "plane":
        t = Terrain("cpu", cfg["terrain"], seed=int(cfg["basic"]["seed"]))
        tdict = dict(height_field_raw=t.height_field_raw, hscale=t.horizontal_scale, vscale=t.vertical_scale, border_px=t.border_pixels)
    mk = lambda real: DynRef(flat_model, feet_edge_pos=cfg["asset"]["feet_edge_pos"], terrain=tdict, real=real)
    return cfg, mk("f64"), mk("f32")


@pytest.mark.parametrize("terrain", ["plane", "trimesh"])
def test_fp32_twin_meets_the_forward_dynamics_spot_checks(flat_model, terrain):
    cfg, dyn, twin = _dyn_pair(flat_model, terrain)

    def shift(root):
        if terrain != "plane":
            root[:, 0] += 20.0; root[:, 1] += 5.0
            root[:, 2] += np.array([dyn.terrain_height(x, y) for x, y in root[:, :2]])

    tabs = PU.fd_tables(dyn, flat_model, _states, shift)
    pool = tabs["pool"]
    assert len(pool) >= 200 and (pool % 2 == 0).sum() >= 64 and (pool % 2 == 1).sum() >= 64
    assert tabs["all"]["listed"][pool].all() and np.array_equal(tabs["sparse"]["listed"][pool], pool % 2 == 0)
    listed = PU.sparse_listed(N, EPB)
    src = PU.shuffled_src((~listed).astype(int), [pool[pool % 2 == 0], pool[pool % 2 == 1]])
    hp = PU.host_params(cfg, flat_model, NS)
    params = {"mass_scale": hp["mass_scale"][src], "com_offset": hp["com_off"].reshape(NS, 39)[src], "foot_material": hp["foot_mat"].reshape(NS, 6)[src]}
    spots = PU.spot_positions(N, must=np.nonzero(listed)[0][:: max(1, int(listed.sum()) // 24)])
    for k in ("all", "sparse") + (("crossed",) if terrain == "plane" else ()):
        worst, ncontact = PU.fd_spot_check(dyn, tabs[k], src if k != "crossed" else PU.shuffled_src(np.zeros(N, dtype=int), [np.arange(NS)]), spots, None, None,
                                           params, twin=twin)
        print(f"fp32 twin on the spot-check states, {terrain} {k}: worst error / tolerance {worst:.3f}, {ncontact} with a contact")
        assert ncontact >= 8


def test_fp32_twin_meets_the_simulate_spot_check(flat_model):
    """Case B: one step of the twin from the source states at the spot positions through src, with the body wrench pending and without it, held to the
    float64 oracle's step by the comparison the GPU test makes (parity_util.sim_implied_error) at that test's tolerances."""
    cfg, dyn, twin = _dyn_pair(flat_model, "plane")
    root, q, qd, tau, bf, bt, is_low = PU.sim_sources(flat_model, _states, float(cfg["contact"]["body_gate_height"]))
    low = PU.low_placement(N, EPB, K["BODY_GRID"])
    src = PU.shuffled_src((~low).astype(int), [np.nonzero(is_low)[0], np.nonzero(~is_low)[0]])
    assert set(src.tolist()) == set(range(NS)) and np.array_equal(is_low[src], low)
    spots = PU.spot_positions(N, must=np.nonzero(low)[0][::3])
    assert is_low[src[spots]].sum() >= 16 and (~is_low[src[spots]]).sum() >= 16
    hp = PU.host_params(cfg, flat_model, NS)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    worst = {"wrench": 0.0, "none": 0.0}
    for e in spots:
        i = int(src[e])
        par = dict(mass_scale=hp["mass_scale"][i], com_off=hp["com_off"][i], foot_mat=hp["foot_mat"][i].reshape(6))
        tol = PU.FAMILY_TOL["low" if is_low[i] else True]
        for name, (f, t) in {"wrench": (f32(bf[i]), f32(bt[i])), "none": (None, None)}.items():
            r, qq, qv = f32(root[i]), f32(q[i]), f32(qd[i])
            twin.step_bw(r, qq, qv, f32(tau[i]), f, t, **par)
            err = PU.sim_implied_error(dyn, f32(root[i]), f32(q[i]), f32(qd[i]), f32(tau[i]), f, t, par, np.concatenate([r[7:13], qv]))
            assert err < tol, f"env {e} (source {i}, {'low' if is_low[i] else 'standing'}, {name}): implied acceleration error {err:.2e}, tolerance {tol:g}"
            worst[name] = max(worst[name], err / tol)
    print(f"fp32 twin on the simulate spot-check states: worst error / tolerance {worst}")
