"""The dynamics away from the T1's model, without a GPU: the product's lane code compiled for the host (tests/host_harness/harness.cpp) against the
float64 oracle on the models of tests/model_variants.py, and the conditions under which that comparison means something:
  parity             hh_forward / hh_forward_pk hold the tolerances of test_product_dynamics_header_matches_oracle on every variant
  mask independence  the sweeps specialised by the variant's true Phys::zmask, by no bit and (all_axis, swapped) by each single bit give the same
  the oracle itself  ABA (DynRef.forward) against RNEA (DynRef.inverse), two independent algorithms, on every variant
  visibility         each altered group of numbers, put back to the T1's values alone, moves the oracle's accelerations by more than 10 x the
                     tolerance in at least half of the states of the family that exercises it
  twin               DynRef(real="f32") holds every tolerance with no excused state in the airborne, standing and crossed families
and the forecast for tests/test_gpu_model_surface.py: the states that file draws (same seed), through the host-compiled lane code.
The figures are printed (pytest -s); profiles/model_surface_parity.txt keeps them."""
import ctypes as C
import copy
import os
import subprocess

import numpy as np
import pytest

import dyn_header_util as DH
import model_variants as MV

HERE = os.path.dirname(os.path.abspath(__file__))
SENS_FACTOR, SENS_SHARE = 10.0, 0.5  # the rule of the config-surface work (parity_util.SENS_FACTOR / SENS_SHARE)


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hh_model") / "libharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-O2", "-o", so, os.path.join(HERE, "host_harness", "harness.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def variants(flat_model, tmp_path_factory):
    """Every variant after a save / FlatModel.load round trip."""
    d = tmp_path_factory.mktemp("variants")
    return {name: MV.saved(flat_model, name, d)[0] for name in MV.NAMES}


def _desc(model, v):
    """bg_model_desc as T1._model_struct fills it."""
    from booster_gym_amd import _lib

    d = _lib.ModelDesc()
    d.num_bodies, d.num_dofs = model.num_bodies, model.num_dofs
    for b in range(13):
        d.parent[b], d.joint_axis[b], d.mass[b] = int(model.parent[b]), int(model.joint_axis[b]), float(model.mass[b])
        for a in range(3):
            d.body_pos[b][a], d.com[b][a] = float(model.body_pos[b, a]), float(model.com[b, a])
        for a in range(6):
            d.inertia[b][a] = float(model.inertia[b, a])
    for k in range(4):
        for a in range(3):
            d.feet_edge_pos[k][a] = float(v.feet_edge_pos[k][a])
    sph = model.contact_spheres(exclude_bodies=[6, 12])
    d.num_body_spheres = len(sph)
    for k, (b, c, r) in enumerate(sph):
        d.sphere_body[k], d.sphere_radius[k] = b, r
        for a in range(3):
            d.sphere_pos[k][a] = c[a]
    for leg, caps in enumerate(model.self_collision_capsules([6, 12])):
        for k, (_, a, b, r) in enumerate(caps):
            d.self_capsule_r[leg][k] = r
            for ax in range(3):
                d.self_capsule_a[leg][k][ax], d.self_capsule_b[leg][k][ax] = a[ax], b[ax]
    return d


@pytest.mark.parametrize("name", MV.NAMES)
def test_variant_is_a_valid_physical_model(flat_model, variants, name):
    """The variant survives the file round trip unchanged, passes bg_model_validate, has the zero structure its table row states, and is physical:
    positive principal moments that satisfy the triangle inequalities on every body."""
    from booster_gym_amd import _lib

    v, raw = variants[name], MV.variant(flat_model, name)
    for f in ("body_pos", "mass", "com", "inertia", "dof_lower", "dof_upper"):
        assert np.array_equal(getattr(v.model, f), getattr(raw.model, f)), f
    assert v.model.shapes == raw.model.shapes and MV.zmask_of(v.model) == v.zmask
    lib, mh = _lib.load(), C.c_void_p()
    d = _desc(v.model, v)
    _lib.check(lib.bg_model_create(C.byref(d), C.byref(mh)), "bg_model_create")
    lib.bg_model_destroy(mh)
    for b in range(13):
        lam = MV.principal_moments(v.model.inertia[b])
        assert lam[0] > 0 and lam[0] + lam[1] >= lam[2] * (1 - 1e-12), (b, lam)
    m, t1 = v.model, flat_model
    legs = m.body_pos[1:, :2]
    if name in ("off_axis", "mirror"):
        assert np.abs(legs).min() >= 0.005 and np.abs(m.com[:, 1]).min() >= (0.0 if name == "mirror" else 0.005)
        prod = np.abs(m.inertia[1:, 3:]).max(axis=1) / m.inertia[1:, :3].max(axis=1)
        assert prod.min() > 0.05 and np.median(prod) > 0.2, prod  # the largest product against the largest diagonal entry, every leg link (the hip pitch links are nearly isotropic)
        if name == "off_axis":
            f = m.mass / t1.mass
            assert f[1:].min() >= 0.6 and f[1:].max() <= 1.6 and len(set(np.round(f, 6))) == 13
            assert np.abs(m.body_pos[1:7, 1] + m.body_pos[7:13, 1]).min() > 1e-3  # left and right differ by more than the mirror image
        else:
            assert np.array_equal(m.body_pos[7:13], m.body_pos[1:7] * [1, -1, 1]) and np.abs(m.body_pos[1:7, 1]).min() >= 0.005
    if name == "one_leg":
        assert np.array_equal(m.body_pos[1:7], t1.body_pos[1:7]) and np.abs(m.body_pos[[8, 9, 11], :2]).min() >= 0.005
        assert MV.zmask_of(m) == 0 and all(np.all(m.body_pos[1 + i, :2] == 0) for i in (1, 2, 4))  # the left leg alone says 0b010110
    if name == "geometry":
        for f in ("body_pos", "mass", "com", "inertia"):
            assert np.array_equal(getattr(m, f), getattr(t1, f))
        c = np.array(v.feet_edge_pos)
        assert len(set(np.round(np.abs(c[:, 0]), 6))) == 4 and len(set(np.round(np.abs(c[:, 1]), 6))) == 4
        assert np.all(m.dof_lower > t1.dof_lower) and np.all(m.dof_upper < t1.dof_upper) and np.all(m.dof_lower < m.dof_upper)
        # the default pose stays inside the narrowed range
        q0 = np.array([-0.2, 0, 0, 0.4, -0.25, 0] * 2)
        assert np.all(q0 > m.dof_lower) and np.all(q0 < m.dof_upper)


@pytest.mark.parametrize("name", MV.NAMES)
def test_the_products_derivations_agree_with_the_oracles_own(variants, name):
    """utils/urdf.py's contact spheres and self-collision capsules (what bg_model_desc gets) against oracle/dyn_ref.py's own derivations from the
    same shapes, on shapes that are not centred (geometry) as on the T1's."""
    from oracle.dyn_ref import contact_spheres, self_capsules

    m = variants[name].model
    mine, ref = m.contact_spheres(exclude_bodies=[6, 12]), contact_spheres(m, [6, 12])
    key = lambda t: (t[0], tuple(np.round(t[1], 12)), t[2])
    assert sorted(map(key, mine)) == sorted(map(key, ref)) and [t[0] for t in mine] == sorted(t[0] for t in mine)
    caps = [c for leg in m.self_collision_capsules([6, 12]) for c in leg]
    want = self_capsules(m, [6, 12])
    assert len(caps) == len(want) == 4
    for (b, a0, b0, r), (wb, wa, wbb, wr) in zip(caps, want):
        assert b == wb and r == wr and np.allclose(a0, wa, atol=0, rtol=0) and np.allclose(b0, wbb, atol=0, rtol=0)
    if name == "geometry":  # the end points lie off the link axis, in the components bg_model_validate allows
        assert all(abs(a0[1]) > 1e-3 for _, a0, _, _ in caps) and all(abs(caps[k][1][0]) > 1e-3 for k in (0, 2))


@pytest.mark.parametrize("name", MV.NAMES)
def test_lane_code_matches_the_oracle_on_the_variant(hh, variants, name):
    """Parity and twin: the six state families of test_product_dynamics_header_matches_oracle at its tolerances and contact-count floors, the lane
    code with the sweeps specialised by the variant's true mask (hh_forward_zspec, hh_forward_pk) and without (hh_forward)."""
    v = variants[name]
    for entry in ("hh_forward_zspec", "hh_forward"):
        recs = DH.header_parity(hh, v.model, v.zmask, v.feet_edge_pos, v.phys, entry=entry, twin=entry == "hh_forward_zspec")
        for r in recs:
            print(f"model-surface {name} {entry} {r['family']}: qacc err / tol {r['worst']:.3f}, packed {r['worst_pk']:.3f}, twin {r['worst_twin']:.3f}; "
                  f"{r['ncontact']} states in contact, {r['nbody']} with a body contact")
        DH.assert_parity(recs, f"{name} {entry}", v.self_collisions)
        if entry == "hh_forward_zspec":
            for r in recs:  # (no state of any family is excused here, `low` included)
                assert r["worst_twin"] < 1.0, (name, "twin", r["family"], r["worst_twin"])


@pytest.mark.parametrize("name", MV.NAMES)
def test_the_specialised_sweeps_do_not_depend_on_the_mask(hh, variants, name):
    """Mask independence: a bit of Phys::zmask may only be set for a link on the parent's z axis, and then the specialised branch computes what the
    general one does.  The true mask (test_lane_code_matches_the_oracle_on_the_variant), no bit at all and (all_axis, swapped) each single bit of
    the true mask hold the tolerance on all six families."""
    v = variants[name]
    fams = DH.FAMILIES
    masks = [0] + ([1 << i for i in range(6) if (v.zmask >> i) & 1] if name in ("all_axis", "swapped") else [])
    for mask in masks:
        recs = DH.header_parity(hh, v.model, mask, v.feet_edge_pos, v.phys, entry="hh_forward_zspec", families=fams)
        print(f"model-surface {name} mask {mask:#08b}: " + ", ".join(f"{r['family']} {r['worst']:.3f} packed {r['worst_pk']:.3f}" for r in recs))
        assert len(recs) == 6
        DH.assert_parity(recs, f"{name} mask {mask:#08b}", v.self_collisions)


def _airborne(m, rng, n):
    for _ in range(n):
        root = np.zeros(13); root[2] = 5.0
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0, 1.0)
        root[3:6], root[6] = ax * np.sin(ang / 2), np.cos(ang / 2)
        root[7:13] = rng.normal(size=6)
        yield root, rng.uniform(m.dof_lower, m.dof_upper), rng.normal(size=12), rng.uniform(-m.dof_effort, m.dof_effort), rng.normal(size=6) * 10


@pytest.mark.parametrize("name", MV.NAMES)
def test_oracle_aba_equals_its_inverse_dynamics_on_the_variant(variants, name):
    """The oracle on models it has never seen: airborne, contact-free, in-limit states; RNEA of ABA's accelerations returns the applied torques and
    base wrench to test_oracle_golden.py::test_aba_equals_inverse_dynamics' bound (1e-9 absolute, float64), randomised inertials included."""
    from oracle.dyn_ref import DynRef

    m = variants[name].model
    dyn, rng, worst = DynRef(m, phys={"self_collisions": 0}), np.random.default_rng(0), 0.0
    for root, q, qd, tau, w in _airborne(m, rng, 300):
        ms, co = rng.uniform(0.8, 1.2, 13), rng.uniform(-0.05, 0.05, (13, 3))
        qacc, cf = dyn.forward(root, q, qd, tau, base_wrench=w, mass_scale=ms, com_off=co)
        assert np.abs(cf).max() == 0.0
        res = dyn.inverse(root, q, qd, qacc, mass_scale=ms, com_off=co)
        worst = max(worst, np.abs(res - np.concatenate([w[3:], w[:3], tau])).max())
    print(f"model-surface {name}: inverse(forward) residual {worst:.2e}")
    assert worst < 1e-9


_FAMILY_TOL = {False: 1e-4, True: 5e-4, "crossed": 5e-4, "low": 1e-3}  # tests/test_gpu_dynamics.py's tolerances, per _states family


@pytest.mark.parametrize("name", MV.NAMES)
def test_every_altered_group_is_visible_in_the_oracles_accelerations(flat_model, variants, name):
    """Visibility: per altered group, that group alone back at the T1's values moves DynRef's qacc by more than SENS_FACTOR x the family's tolerance
    in at least SENS_SHARE of the states of the family that exercises it (test_gpu_dynamics._states, the draw the GPU file uses)."""
    from oracle.dyn_ref import DynRef
    from test_gpu_dynamics import _states

    v, n = variants[name], 100
    for group in v.groups:
        fam = MV.GROUP_FAMILY[group]
        if fam == "crossed" and not v.self_collisions:
            continue
        base, corners = copy.deepcopy(v.model), v.feet_edge_pos
        if group == "corners":
            corners = MV.T1_CORNERS
        else:
            MV.set_group(base, flat_model, group)
        a, b = DynRef(v.model, feet_edge_pos=v.feet_edge_pos, phys=v.phys), DynRef(base, feet_edge_pos=corners, phys=v.phys)
        root, q, qd, tau, w = _states(np.random.default_rng(3), v.model, n, fam)
        moved = 0
        for e in range(n):
            qa, _ = a.forward(root[e], q[e], qd[e], tau[e], base_wrench=w[e])
            qb, _ = b.forward(root[e], q[e], qd[e], tau[e], base_wrench=w[e])
            moved += int(np.abs(qa - qb).max() / max(1.0, np.abs(qa).max()) > SENS_FACTOR * _FAMILY_TOL[fam])
        print(f"model-surface {name}: {group} back at the T1's values moves qacc by more than {SENS_FACTOR:g} x {_FAMILY_TOL[fam]:g} in {moved} of {n} "
              f"states of family {fam!r}")
        assert moved >= SENS_SHARE * n, (name, group, moved)


GPU_FAMILIES = (("plane", False, 1e-4), ("plane", True, 5e-4), ("trimesh", True, 5e-4), ("plane", "crossed", 5e-4), ("plane", "low", 1e-3))


@pytest.mark.parametrize("name", [n for n in MV.NAMES if n != "mirror"])
def test_forecast_of_the_gpu_cases_needs_no_excused_state(hh, variants, name):
    """The states tests/test_gpu_model_surface.py draws (same seed, same n; nominal per-env parameters here, a seeded rough field standing for the
    trimesh), through the host-compiled lane code with the sweeps specialised by the variant's mask: how many states the lane code itself needs the
    twin's excuse for, and whether the twin itself holds the tolerance on them.  None outside `low`; in `low` at most 1 % of the case."""
    from oracle.dyn_ref import DynRef
    from test_gpu_dynamics import _states

    v, n = variants[name], 100
    lane = DH.Lane(hh, v.model, v.zmask, v.feet_edge_pos, v.phys)
    hf = np.random.default_rng(1).integers(-10, 10, size=(60, 60)).astype(np.int16)
    for terrain, contact, tol in GPU_FAMILIES:
        if contact == "crossed" and not v.self_collisions:
            continue
        tdict = dict(height_field_raw=hf, hscale=0.1, vscale=0.005, border_px=30) if terrain != "plane" else None
        t = DH.Terr()
        if tdict:
            t.type, t.rows, t.cols, t.border_px, t.inv_hscale, t.vscale, t.hf = 1, 60, 60, 30, 10.0, 0.005, hf.ctypes.data
        ref = DynRef(v.model, feet_edge_pos=v.feet_edge_pos, terrain=tdict, phys=v.phys)
        twin = DynRef(v.model, feet_edge_pos=v.feet_edge_pos, terrain=tdict, phys=v.phys, real="f32")
        root, q, qd, tau, w = _states(np.random.default_rng(3), v.model, n, contact)
        if tdict:
            root[:, 2] += np.array([ref.terrain_height(x, y) for x, y in root[:, :2]])
        worst, worst_twin, excused, ncontact = 0.0, 0.0, [], 0
        for e in range(n):
            qa, _, _ = lane.forward("hh_forward_zspec", t, root[e], q[e], qd[e], tau[e], w[e], np.ones(13), np.zeros(39), np.array([1.0, 1.0, 0.0] * 2))
            a = lane.arrs
            kw = dict(base_wrench=a[7], mass_scale=a[0], com_off=a[1].reshape(13, 3), foot_mat=a[2])
            qr, cf = ref.forward(a[3], a[4], a[5], a[6], **kw)
            qt, _ = twin.forward(a[3], a[4], a[5], a[6], **kw)
            touching = np.abs(cf).max() > 0
            ncontact += int(touching)
            scale = max(1.0, np.abs(qr).max())
            raw, terr = np.abs(qa - qr).max() / scale, np.abs(qt - qr).max() / scale
            tol_s = max(tol, 5e-4) if touching else tol
            worst_twin = max(worst_twin, terr / tol_s)
            if raw >= tol_s and touching:
                assert raw <= terr and raw <= 3e-3, (name, terrain, contact, e, raw, terr)
                excused.append(e)
                continue
            worst = max(worst, raw / tol_s)
        print(f"model-surface forecast {name} {terrain} {contact!r}: qacc err / tol {worst:.3f}, twin {worst_twin:.3f}, {ncontact} of {n} in contact, excused {excused}")
        assert worst < 1.0, (name, terrain, contact, worst)
        assert worst_twin < 1.0, (name, terrain, contact, worst_twin)  # the twin itself holds the tolerance on these states: nothing to excuse
        assert len(excused) <= (n // 100 if contact == "low" else 0), (name, terrain, contact, excused)


@pytest.mark.parametrize("name", ["off_axis", "geometry"])
def test_env_step_twin_stays_inside_the_caps_on_the_variant(flat_model, tmp_path, name):
    """The env-step cases of tests/test_gpu_model_surface.py are well-posed on the reference alone: the shipped config with asset.file = the variant,
    flat ground, the float64 oracle against its own fp32 twin through parity_util.run_case (flags_bad <= 2, the 1 % cap on explained env-steps)."""
    import parity_util as PU

    v, path = MV.saved(flat_model, name, tmp_path)
    cfg, twin, ref = PU.make_oracle_pair(64, v.overrides(path))
    assert np.array_equal(ref.m.body_pos, v.model.body_pos) and np.array_equal(ref.m.mass, v.model.mass)
    summary, _ = PU.run_case(cfg, twin, ref, 96)
    print(f"model-surface env step {name} (twin): explained {summary['explained']} of {summary['env_steps']} {summary['by_reason']}")
