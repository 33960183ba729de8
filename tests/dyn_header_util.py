"""The product's per-lane dynamics headers compiled for the host (tests/host_harness/harness.cpp) against the float64 oracle, on any flat model:
the body of tests/test_host_logic.py::test_product_dynamics_header_matches_oracle as a function, for tests/test_model_surface_ref.py to run on the
models of tests/model_variants.py as well."""
import ctypes as C

import numpy as np


class ModelDev(C.Structure):
    _fields_ = [("pos", C.c_float * 3 * 13), ("mass", C.c_float * 13), ("com", C.c_float * 3 * 13), ("inertia", C.c_float * 6 * 13), ("q_lo", C.c_float * 12),
                ("q_hi", C.c_float * 12), ("qd_max", C.c_float * 12), ("tau_lim", C.c_float * 12), ("corner", C.c_float * 3 * 4),
                ("sph_n", C.c_int), ("sph_first", C.c_int * 13), ("sph_cnt", C.c_int * 13), ("sph_pos", C.c_float * 3 * 16), ("sph_r", C.c_float * 16),
                ("cap_c", C.c_float * 3 * 2 * 2), ("cap_h", C.c_float * 2 * 2), ("cap_r", C.c_float * 2 * 2)]


class Cfg(C.Structure):
    _fields_ = [("dt", C.c_float), ("g", C.c_float * 3)] + [(k, C.c_float) for k in ("contact_k", "contact_d", "contact_ramp", "friction_visc", "limit_k", "limit_d",
                                                                                  "terrain_mu", "terrain_restitution")] + [("clamp_qd", C.c_int), ("body_gate", C.c_float), ("self_on", C.c_int)] + \
               [(k, C.c_float) for k in ("self_k", "self_d", "self_mu", "self_visc")] + [("zmask", C.c_int)]


class Terr(C.Structure):
    _fields_ = [("type", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("border_px", C.c_int), ("inv_hscale", C.c_float), ("vscale", C.c_float), ("hf", C.c_void_p)]


T1_CORNERS = [[0.1215, 0.05, -0.03], [0.1215, -0.05, -0.03], [-0.1015, 0.05, -0.03], [-0.1015, -0.05, -0.03]]
# (terrain?, contact, tolerance): contact False = airborne, True = standing height (sole contacts), "low" = trunk 0.15-0.5 m above the ground in any
# orientation, so that the trunk box and the hip-yaw / shank cylinders touch (explicit sphere contacts) as well, "crossed" = airborne with the hip
# rolls drawn inwards, so that shanks / feet of the two legs overlap (leg-against-leg contacts)
FAMILIES = ((False, False, 2e-5), (False, True, 5e-4), (True, True, 5e-4), (False, "low", 1e-3), (True, "low", 1e-3), (False, "crossed", 5e-4))


def model_dev(m, feet_edge_pos=None):
    """ModelDev as bg_env_create fills it, from the product's own derivations of the contact spheres and self-collision capsules (utils/urdf.py)."""
    md = ModelDev()
    for b in range(13):
        md.mass[b] = m.mass[b]
        for a in range(3):
            md.pos[b][a], md.com[b][a] = m.body_pos[b, a], m.com[b, a]
        for a in range(6):
            md.inertia[b][a] = m.inertia[b, a]
    for j in range(12):
        md.q_lo[j], md.q_hi[j], md.qd_max[j], md.tau_lim[j] = m.dof_lower[j], m.dof_upper[j], m.dof_velocity[j], m.dof_effort[j]
    corners = T1_CORNERS if feet_edge_pos is None else feet_edge_pos
    for k in range(4):
        for a in range(3):
            md.corner[k][a] = corners[k][a]
    sph = m.contact_spheres(exclude_bodies=[6, 12])  # the product's own derivation of the contact spheres (utils/urdf.py)
    md.sph_n = len(sph)
    for k, (b, c, r) in enumerate(sph):
        if md.sph_cnt[b] == 0:
            md.sph_first[b] = k
        md.sph_cnt[b] += 1
        md.sph_r[k] = r
        for a in range(3):
            md.sph_pos[k][a] = c[a]
    assert len(sph) == 16 and [md.sph_cnt[b] for b in (0, 3, 4, 9, 10)] == [8, 2, 2, 2, 2]
    for leg, caps in enumerate(m.self_collision_capsules([6, 12])):  # the product's own derivation of the self-collision capsules
        for k, (body, a, b, r) in enumerate(caps):
            assert body == (4, 6)[k] + 6 * leg
            ax = (2, 0)[k]
            md.cap_h[leg][k], md.cap_r[leg][k] = 0.5 * (b[ax] - a[ax]), r
            for i in range(3):
                md.cap_c[leg][k][i] = 0.5 * (a[i] + b[i])
    return md


def cfg_of(zmask, phys=None):
    from oracle.dyn_ref import DEFAULT_PHYS

    ph = dict(DEFAULT_PHYS); ph.update(phys or {})
    cfg = Cfg(); cfg.dt = ph["dt"]; cfg.clamp_qd = 1; cfg.body_gate = ph["body_gate_height"]
    cfg.self_on = int(ph["self_collisions"])
    for k in ("self_k", "self_d", "self_mu", "self_visc"):
        setattr(cfg, k, ph[k])
    cfg.zmask = zmask
    for a in range(3):
        cfg.g[a] = ph["g"][a]
    for k in ("contact_k", "contact_d", "contact_ramp", "friction_visc", "limit_k", "limit_d", "terrain_mu", "terrain_restitution"):
        setattr(cfg, k, ph[k])
    return cfg


class Lane:
    """One env through the host-compiled lane code.  entry: "hh_forward" (the fused env step's store: the mask is ignored), "hh_forward_zspec" (the
    same lane code with the sweeps specialised by the mask, as in the ABA kernel) or "hh_forward_pk" (the packed kernel's code: specialised)."""

    def __init__(self, hh, model, zmask, feet_edge_pos=None, phys=None):
        self.hh, self.md, self.cfg = hh, model_dev(model, feet_edge_pos), cfg_of(zmask, phys)

    def forward(self, entry, terr, root, q, qd, tau, w, ms, co, fm):
        """qacc[18], foot forces [2,3], body contact forces [13,3] (None for the packed code).  Inputs are rounded to fp32 here; `arrs` keeps them."""
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self.arrs = arrs = [f32(ms), f32(np.reshape(co, 39)), f32(fm), f32(root), f32(q), f32(qd), f32(tau), f32(w)]
        qa, cf = np.zeros(18, np.float32), np.zeros(6, np.float32)
        if entry == "hh_forward_pk":
            self.hh.hh_forward_pk(C.byref(self.md), C.byref(self.cfg), C.byref(terr), *[p(a) for a in arrs], p(qa), p(cf))
            return qa, cf.reshape(2, 3), None
        bcf = np.zeros((13, 3), np.float32)
        getattr(self.hh, entry)(C.byref(self.md), C.byref(self.cfg), C.byref(terr), *[p(a) for a in arrs], p(qa), p(cf), 0, p(bcf))
        return qa, cf.reshape(2, 3), bcf


def header_parity(hh, model, zmask, feet_edge_pos=None, phys=None, entry="hh_forward", pk_zmask=None, twin=False, families=FAMILIES):
    """150 seeded states per family through `entry` (and, at pk_zmask or `zmask`, the packed lane code) against DynRef float64 on `model`.
    Returns one record per family: worst / worst_pk (relative qacc error over the tolerance of the state: < 1 passes), ncontact, nbody, and with
    `twin` worst_twin (DynRef real="f32" held to the same tolerances, no state excused).  The foot and body contact forces are asserted here."""
    from oracle.dyn_ref import DynRef

    m = model
    lane = Lane(hh, m, zmask, feet_edge_pos, phys)
    lane_pk = lane if pk_zmask is None else Lane(hh, m, pk_zmask, feet_edge_pos, phys)
    rng = np.random.default_rng(1)
    hf = rng.integers(-10, 10, size=(60, 60)).astype(np.int16)
    out = []
    for rough, contact, tol in FAMILIES:
        terrain = dict(height_field_raw=hf, hscale=0.1, vscale=0.005, border_px=30) if rough else None
        d = DynRef(m, feet_edge_pos=feet_edge_pos, terrain=terrain, phys=phys)
        d32 = DynRef(m, feet_edge_pos=feet_edge_pos, terrain=terrain, phys=phys, real="f32") if twin else None
        t = Terr()
        if terrain is not None:
            t.type, t.rows, t.cols, t.border_px, t.inv_hscale, t.vscale, t.hf = 1, 60, 60, 30, 10.0, 0.005, hf.ctypes.data
        name = ("rough " if rough else "plane ") + {False: "airborne", True: "standing", "low": "low", "crossed": "crossed"}[contact]
        rec = dict(family=name, tol=tol, worst=0.0, worst_pk=0.0, worst_twin=0.0, ncontact=0, nbody=0, contact=contact)
        crossed = contact == "crossed"
        if crossed:
            contact = False
        for _ in range(150):  # (every family draws its states whether it is asked for or not: one stream, the same states as ever)
            root = np.zeros(13); root[2] = (rng.uniform(0.15, 0.5) if contact == "low" else rng.uniform(0.55, 0.72)) if contact else 5.0
            root[:2] = rng.uniform(-1, 1, 2)
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(0, 3.0 if contact == "low" else 0.3)
            root[3:6], root[6] = ax * np.sin(ang / 2), np.cos(ang / 2)
            root[7:13] = rng.normal(size=6) * (0.3 if contact else 1.0)
            q = (np.array([-0.2, 0, 0, 0.4, -0.25, 0] * 2) + rng.normal(size=12) * 0.1) if contact else rng.uniform(m.dof_lower - 0.05, m.dof_upper + 0.05)
            if crossed:
                q[[1, 7]], q[[0, 6]], q[[3, 9]] = (rng.uniform(-0.3, 0.0), rng.uniform(0.0, 0.3)), rng.uniform(-0.6, 0.2, 2), rng.uniform(0.0, 0.8, 2)
            elif not contact:  # plain airborne case: smooth dynamics only, legs apart
                q[[1, 7]] = rng.uniform(0.2, 1.0), rng.uniform(-1.0, -0.2)
            qd, tau, w = rng.normal(size=12), rng.uniform(-m.dof_effort, m.dof_effort), rng.normal(size=6) * 10
            ms, co = rng.uniform(0.8, 1.2, 13), rng.uniform(-0.05, 0.05, (13, 3))
            fm = np.array([rng.uniform(0.1, 2), rng.uniform(0.5, 1.5), rng.uniform(0.1, 0.9)] * 2)
            if (rough, rec["contact"], tol) not in families:
                continue
            qa, cf32, bcf = lane.forward(entry, t, root, q, qd, tau, w, ms, co, fm)
            arrs = lane.arrs
            kw = dict(base_wrench=arrs[7], mass_scale=arrs[0], com_off=arrs[1].reshape(13, 3), foot_mat=arrs[2])
            qacc, cf = d.forward(arrs[3], arrs[4], arrs[5], arrs[6], **kw)
            tol_s = tol if np.abs(cf).max() == 0 else max(tol, 5e-4)  # any contact (also a chance leg-against-leg one in the airborne case) is stiff
            rec["worst"] = max(rec["worst"], np.abs(qa - qacc).max() / max(1.0, np.abs(qacc).max()) / tol_s)
            if contact != "low":  # the packed lane code (one env per lane, bg_dyn_pk.h) carries no non-foot body contacts: every other case
                qp, cfp, _ = lane_pk.forward("hh_forward_pk", t, root, q, qd, tau, w, ms, co, fm)
                rec["worst_pk"] = max(rec["worst_pk"], np.abs(qp - qacc).max() / max(1.0, np.abs(qacc).max()) / tol_s)
                assert np.abs(cfp - cf[[6, 12]]).max() <= 2e-3 * max(1.0, np.abs(cf).max())
            if twin:
                qt, _ = d32.forward(arrs[3], arrs[4], arrs[5], arrs[6], **kw)
                rec["worst_twin"] = max(rec["worst_twin"], np.abs(qt - qacc).max() / max(1.0, np.abs(qacc).max()) / tol_s)
            rec["ncontact"] += int(np.abs(cf).max() > 0)
            body_rows = [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11]
            rec["nbody"] += int(np.abs(cf[body_rows]).max() > 0)
            assert np.abs(bcf[body_rows] - cf[body_rows]).max() <= 2e-3 * max(1.0, np.abs(cf).max())
        if (rough, rec["contact"], tol) in families:
            out.append(rec)
    return out


def assert_parity(recs, what="", self_collisions=True):
    """The assertions of test_product_dynamics_header_matches_oracle on header_parity's records: tolerances and contact-count floors."""
    for r in recs:
        contact = r["contact"]
        crossed = contact == "crossed"
        assert r["worst"] < 1.0, (what, r["family"], r["worst"])
        assert r["worst_pk"] < 1.0, (what, "packed", r["family"], r["worst_pk"])
        touching = (contact in (True, "low")) or (crossed and self_collisions)
        assert (r["ncontact"] > 50) == bool(touching), (what, r["family"], r["ncontact"])
        assert (r["nbody"] > 30) == (contact == "low" or (crossed and self_collisions)), (what, r["family"], r["nbody"])  # crossed: the shank rows carry leg-against-leg forces
