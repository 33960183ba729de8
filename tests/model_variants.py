"""Models away from the shipped T1 for the dynamics parity tests (tests/test_model_surface_ref.py on the host, tests/test_gpu_model_surface.py on
the GPU).  bg_model_validate fixes the topology only (13 bodies, two 6-link chains with axes y x z y y x); every NUMBER of bg_model_desc is free,
and the T1's numbers share a zero structure (leg links 1, 2, 4 on the parent's z axis, com y and the xy / yz inertia products next to nothing,
symmetric sole corners, centred collision shapes) under which a wrong sign or index in a term that multiplies one of them goes unseen.

variant(flat_model, name) -> Variant: a deep copy of the T1 FlatModel with

  name       what changes                                                                                     Phys::zmask expected
  off_axis   origins, com, inertia products and masses of every leg link, different left and right           0
  one_leg    T1 origins except the RIGHT leg's links 1, 2, 4 (x, y offsets); com / inertia / mass as off_axis  0  (the left leg alone would give 0b010110)
  swapped    links 3 and 5 on the parent's z axis in both legs, links 0, 1, 2, 4 off it; rest as off_axis      0b101000
  all_axis   every leg link at (0, 0, z) in both legs (the chains coincide: leg-against-leg contacts off)      0b111111
  geometry   T1 inertials; sole corners, collision shapes and joint limits changed                            0b010110
  mirror     conftest.symmetrised(off_axis): exactly mirror-symmetric with non-zero y everywhere              0

Magnitudes (chosen on the host so that tests/test_model_surface_ref.py's visibility, twin and contact-count conditions all hold; what moved on the way:
  hip and shank y offsets of ORIGIN_XY outwards -> inwards (the crossed family touched in 49 / 50 / 25 of 150 states, floors 50 / 30); geometry shank
  cylinders r 0.05 -> 0.075 / 0.07, foot boxes 0.10 -> 0.14 / 0.13 wide (capsules visible in 49 % -> 61 % of the crossed states); two mass factors twice
  -> thirteen different ones; swapped: x offsets of links 1, 2, 4 as off_axis -> negated (SWAPPED_SIGN): with off_axis' signs one crossed state of
  the GPU file's draw, env 79, is ill-conditioned in single precision, the twin at 1.38 x the 5e-4 tolerance; negated 0.14 x, 0.11 x with random
  per-env parameters):
  origins    x, y of 0.8 - 2.4 cm on every leg link (ORIGIN_XY; the hip pitch link gets them on top of the T1's 6 / 10 cm)
  com        y offsets of 1.0 - 2.5 cm on every body, the trunk included (COM_DY)
  inertia    I = R diag(principal moments of the T1's tensor) R^T with R a turn of 0.5 - 0.75 rad about a skew axis (INERTIA_TURN): the products
             reach a sizeable fraction of the diagonals, the principal moments stay the T1's own (triangle inequalities hold), and the tensor is
             about the centre of mass, so it stays physical under any per-env mass_scale / com_off
  masses     per-link factors in [0.65, 1.5], the trunk 0.95 (MASS_FACTOR); the inertia is scaled with the mass
  limits     narrowed by 0.05 - 0.30 rad per joint, per side and per leg (LIMIT_IN)
"""
import copy
from dataclasses import dataclass

import numpy as np

NAMES = ("off_axis", "one_leg", "swapped", "all_axis", "geometry", "mirror")
T1_ZMASK = 0b010110
T1_CORNERS = [[0.1215, 0.05, -0.03], [0.1215, -0.05, -0.03], [-0.1015, 0.05, -0.03], [-0.1015, -0.05, -0.03]]

# x, y of the link origins in the parent frame, leg links 0..5, [left, right]; link 0: added to the T1's hip position
ORIGIN_XY = np.array([[[0.008, -0.009], [0.015, -0.012], [-0.012, 0.018], [-0.024, -0.014], [0.011, -0.016], [0.013, 0.012]],
                      [[-0.006, 0.012], [0.012, 0.016], [-0.017, -0.011], [-0.020, 0.017], [0.014, 0.010], [-0.010, -0.015]]])
# swapped: the x offsets of links 1, 2, 4 with the other sign (see the docstring)
SWAPPED_SIGN = np.array([-1.0, 1.0])
# y offset of the centre of mass, bodies 0..12
COM_DY = np.array([0.015, 0.020, -0.012, 0.025, -0.018, 0.010, 0.014, -0.016, 0.022, -0.013, 0.024, -0.011, -0.017])
# turn of the inertia tensor's principal frame: axis (not normalised) and angle, bodies 0..12
INERTIA_TURN = [((1, 1, 1), 0.50), ((1, -1, 1), 0.60), ((1, 2, -1), 0.70), ((2, 1, 1), 0.55), ((-1, 1, 2), 0.65), ((1, 1, -2), 0.75), ((1, -2, 1), 0.60),
                ((-1, 1, 1), 0.70), ((2, -1, 1), 0.55), ((1, 1, 2), 0.65), ((1, -1, -1), 0.50), ((-2, 1, 1), 0.60), ((1, 2, 1), 0.75)]
MASS_FACTOR = np.array([0.95, 1.3, 0.7, 1.2, 0.8, 1.5, 1.1, 0.85, 1.4, 0.9, 1.25, 0.65, 1.35])
# joint limits moved inwards: (lower += a, upper -= b), DoFs 0..11
LIMIT_IN = np.array([[0.20, 0.30], [0.05, 0.25], [0.15, 0.10], [0.10, 0.25], [0.12, 0.08], [0.10, 0.06],
                     [0.30, 0.15], [0.20, 0.05], [0.10, 0.20], [0.15, 0.30], [0.06, 0.10], [0.05, 0.12]])
# the sole corners of the geometry variant: a quadrilateral with no symmetry (front left, front right, rear left, rear right as in the T1's list)
GEOMETRY_CORNERS = [[0.1300, 0.060, -0.03], [0.1150, -0.040, -0.03], [-0.0900, 0.045, -0.03], [-0.1100, -0.055, -0.03]]
# the collision shapes of the geometry variant, in the order of the T1's list: trunk box moved and resized, hip-yaw cylinders moved and resized,
# shank cylinders and foot boxes moved in x / y and resized, different left and right (their capsules then lie off the link axis in the components bg_model_validate allows)
GEOMETRY_SHAPES = [dict(body=0, type="box", size=[0.17, 0.18, 0.26], pos=[0.04, 0.015, 0.10]),
                   dict(body=3, type="cylinder", size=[0.045, 0.18], pos=[0.010, -0.008, 0.010]),
                   dict(body=4, type="cylinder", size=[0.075, 0.19], pos=[0.012, -0.009, -0.12]),
                   dict(body=6, type="box", size=[0.223, 0.14, 0.03], pos=[0.02, 0.008, -0.015]),
                   dict(body=9, type="cylinder", size=[0.055, 0.14], pos=[-0.006, 0.012, -0.010]),
                   dict(body=10, type="cylinder", size=[0.07, 0.18], pos=[-0.008, 0.011, -0.12]),
                   dict(body=12, type="box", size=[0.21, 0.13, 0.03], pos=[0.005, -0.006, -0.015])]

# the groups a variant can alter and the state family (test_gpu_dynamics._states' `contact` argument) that exercises each
GROUP_FAMILY = {"origins_xy": False, "com_y": False, "inertia_products": False, "masses": False, "limits": False, "corners": True,
                "capsules": "crossed", "spheres": "low"}


@dataclass
class Variant:
    name: str
    model: object          # FlatModel
    zmask: int             # what bg_env_create must derive (Phys::zmask)
    groups: tuple          # keys of GROUP_FAMILY this variant alters
    feet_edge_pos: list    # asset.feet_edge_pos / DynRef(feet_edge_pos=...)
    self_collisions: bool  # False: asset.self_collisions = 1 (the filter mask: off) and phys={"self_collisions": 0} in DynRef

    def overrides(self, path):
        """Config overrides that make T1(cfg) run this variant from the flat-model file at `path`."""
        ov = {"asset.file": str(path), "asset.feet_edge_pos": [list(c) for c in self.feet_edge_pos]}
        if not self.self_collisions:
            ov["asset.self_collisions"] = 1
        return ov

    @property
    def phys(self):
        return None if self.self_collisions else {"self_collisions": 0}


def zmask_of(model):
    """bg_env_create's rule: the leg links whose origin lies on the parent's z axis in BOTH legs."""
    return sum(1 << i for i in range(6) if all(model.body_pos[1 + 6 * leg + i, 0] == 0 and model.body_pos[1 + 6 * leg + i, 1] == 0 for leg in range(2)))


def _turn(axis, angle):
    k = np.asarray(axis, dtype=np.float64); k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _tensor(i6):
    return np.array([[i6[0], i6[3], i6[4]], [i6[3], i6[1], i6[5]], [i6[4], i6[5], i6[2]]])


def principal_moments(i6):
    return np.linalg.eigvalsh(_tensor(i6))


def set_group(dst, src, group):
    """Copy one group of numbers from model `src` into model `dst` (both FlatModels): how a variant is put together, and how the visibility check
    puts one group alone back to the T1's values.  corners are not part of the model (Variant.feet_edge_pos)."""
    if group == "origins_xy":
        dst.body_pos[:, :2] = src.body_pos[:, :2]
    elif group == "com_y":
        dst.com[:, 1] = src.com[:, 1]
    elif group == "inertia_products":  # the tensor about the centre of mass at dst's mass: src's orientation of the principal frame
        dst.inertia[:] = src.inertia * (dst.mass / src.mass)[:, None]
    elif group == "masses":
        dst.inertia[:] = dst.inertia * (src.mass / dst.mass)[:, None]
        dst.mass[:] = src.mass
    elif group == "limits":
        dst.dof_lower[:], dst.dof_upper[:] = src.dof_lower, src.dof_upper
    elif group in ("capsules", "spheres"):  # one list of shapes feeds both derivations
        dst.shapes = copy.deepcopy(src.shapes)
    else:
        raise KeyError(group)


def _inertials(m, t1):
    m.com[:, 1] = t1.com[:, 1] + COM_DY
    for b in range(13):
        lam, vec = np.linalg.eigh(_tensor(t1.inertia[b]))
        assert lam[0] > 0 and lam[0] + lam[1] >= lam[2], f"body {b}: the T1's principal moments are not physical"
        I = _turn(*INERTIA_TURN[b]) @ vec @ np.diag(lam) @ vec.T @ _turn(*INERTIA_TURN[b]).T * MASS_FACTOR[b]
        m.inertia[b] = [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
    m.mass[:] = t1.mass * MASS_FACTOR


def variant(flat_model, name):
    t1 = flat_model
    m = copy.deepcopy(t1)
    m.name = f"{t1.name}_{name}"
    corners, selfc = [list(c) for c in T1_CORNERS], True
    inertial_groups = ("com_y", "inertia_products", "masses")
    if name in ("off_axis", "mirror"):
        for leg in range(2):
            for i in range(6):
                b = 1 + 6 * leg + i
                m.body_pos[b, :2] = ORIGIN_XY[leg, i] + (t1.body_pos[b, :2] if i == 0 else 0.0)
        _inertials(m, t1)
        groups = ("origins_xy",) + inertial_groups
        if name == "mirror":
            from conftest import symmetrised

            m = symmetrised(m)
            m.name = f"{t1.name}_{name}"
    elif name == "one_leg":
        for i in (1, 2, 4):
            m.body_pos[7 + i, :2] = ORIGIN_XY[1, i]
        _inertials(m, t1)
        groups = ("origins_xy",) + inertial_groups
    elif name == "swapped":
        for leg in range(2):
            for i in range(6):
                b = 1 + 6 * leg + i
                m.body_pos[b, :2] = 0.0 if i in (3, 5) else ORIGIN_XY[leg, i] * (1.0 if i == 0 else SWAPPED_SIGN) + (t1.body_pos[b, :2] if i == 0 else 0.0)
        _inertials(m, t1)
        groups = ("origins_xy",) + inertial_groups
    elif name == "all_axis":
        m.body_pos[1:, :2] = 0.0
        _inertials(m, t1)
        groups, selfc = ("origins_xy",) + inertial_groups, False
    elif name == "geometry":
        m.shapes = copy.deepcopy(GEOMETRY_SHAPES)
        m.dof_lower[:] = t1.dof_lower + LIMIT_IN[:, 0]
        m.dof_upper[:] = t1.dof_upper - LIMIT_IN[:, 1]
        corners = [list(c) for c in GEOMETRY_CORNERS]
        groups = ("corners", "capsules", "spheres", "limits")
    else:
        raise KeyError(name)
    expected = {"off_axis": 0, "one_leg": 0, "swapped": 0b101000, "all_axis": 0b111111, "geometry": T1_ZMASK, "mirror": 0}[name]
    assert zmask_of(m) == expected, (name, bin(zmask_of(m)))
    return Variant(name, m, expected, groups, corners, selfc)


def saved(flat_model, name, directory):
    """The variant, written to `directory` and loaded back (what asset.file hands the env): (Variant with the loaded model, path)."""
    import os

    from booster_gym_amd.utils.urdf import FlatModel

    v = variant(flat_model, name)
    path = os.path.join(str(directory), f"T1_{name}.flat.json")
    v.model.save(path)
    v.model = FlatModel.load(path)
    return v, path
