"""Left-right mirror maps of the T1 task: reflection in the sagittal plane (y -> -y), for the mirror-symmetry loss (algorithm.symmetry_loss).

Both maps are signed permutations, written as (src, sign): (M v)[i] = sign[i] * v[src[i]].  They are built from the model (joint names and axes)
and the observation layout of T1's observations (oracle/task_ref.py compute_observations), not from a table:
  * joints (actions, dof_pos - default, dof_vel, last actions): Left_* <-> Right_* by name; a joint about x or z (roll, yaw) changes sign, one about
    y (pitch) keeps it;
  * projected gravity (x, -y, z); base angular velocity, a pseudo-vector, (-x, y, -z); commands (vx, -vy, -yaw rate);
  * gait clock (cos, sin) -> (-cos, -sin): the feet-swing reward puts the left foot at phase 0.25 and the right one at 0.75, so the mirror image
    of a gait is the same gait half a period later.
"""
import numpy as np

# T1's observation layout: gravity [0, 3), angular velocity [3, 6), commands [6, 9), gait clock cos / sin 9 / 10, then dof_pos - default, dof_vel
# and the last actions, one block of num_dofs each
OBS_JOINTS = 11
_SWAP = (("Left", "Right"), ("left", "right"))


def joint_mirror(dof_names, dof_axes):
    """(src, sign) of the joints: src[j] = the joint whose name is j's with Left and Right swapped (a joint without either maps to itself), sign[j] =
    -1 for a joint about x or z, +1 about y (dof_axes: 1 / 2 / 3 = x / y / z).  ValueError if the model has no left / right pairs, a joint has no
    partner, or two partners turn about different axes."""
    names = list(dof_names)
    if len(dof_axes) != len(names):
        raise ValueError(f"joint_mirror: {len(names)} joint names but {len(dof_axes)} axes")
    src, sign, paired = [], [], False
    for j, name in enumerate(names):
        other = name
        for a, b in _SWAP:
            if a in name:
                other, paired = name.replace(a, b), True
                break
            if b in name:
                other, paired = name.replace(b, a), True
                break
        if other not in names:
            raise ValueError(f"symmetry loss: joint {name!r} has no mirror partner {other!r} in the model")
        k = names.index(other)
        if int(dof_axes[k]) != int(dof_axes[j]) or int(dof_axes[j]) not in (1, 2, 3):
            raise ValueError(f"symmetry loss: joints {name!r} and {other!r} do not turn about the same x / y / z axis")
        src.append(k)
        sign.append(1.0 if int(dof_axes[j]) == 2 else -1.0)
    if not paired:
        raise ValueError("symmetry loss: the model has no Left_* / Right_* joint pairs to mirror")
    return np.array(src, dtype=np.int32), np.array(sign, dtype=np.float32)


def scan_mirror(height_points):
    """src of the height scan's mirror map (every sign is +1, a height does not change under y -> -y): src[p] = the point at (x_p, -y_p).
    ValueError naming terrain.measured_points_y if the grid is not symmetric under y -> -y."""
    pts = np.asarray(height_points, dtype=np.float64).reshape(-1, 2)
    index = {(float(x), float(y)): p for p, (x, y) in enumerate(pts)}
    src = [index.get((float(x), float(-y)), -1) for x, y in pts]
    if min(src, default=0) < 0:
        raise ValueError("algorithm.symmetry_loss with terrain.actor_heights needs a height scan that is its own mirror image: "
                         "terrain.measured_points_y must be symmetric under negation (for every y also -y)")
    return np.array(src, dtype=np.int32)


def mirror_maps(dof_names, dof_axes, default_dof_pos, num_obs, frame_stack=1, height_points=None):
    """(obs_src, obs_sign, act_src, act_sign): the maps M_o of the observations and M_a of the actions.  ValueError if the model has no left /
    right pairing, the observation width is not T1's layout for these joints, or the default pose is not its own mirror image (dof_pos - default
    then would not mirror as a signed permutation).  frame_stack = H > 1 (env.frame_stack): num_obs is H single observations side by side and M_o
    the single observation's map tiled over them, frame k's source indices offset by k times the single width.  height_points ([P][2], terrain.actor_heights)
    : the row ends with the P values of the height scan, and M_o with their block: point (x_i, y_j) takes the value of (x_i, -y_j), sign +1."""
    act_src, act_sign = joint_mirror(dof_names, dof_axes)
    nd = len(act_src)
    scan_src = scan_mirror(height_points) if height_points is not None and len(height_points) else np.zeros(0, dtype=np.int32)
    num_obs = num_obs - len(scan_src)
    H, total = int(frame_stack), num_obs
    if H < 1 or num_obs != H * (OBS_JOINTS + 3 * nd):
        raise ValueError(f"symmetry loss: {num_obs} observations are not T1's layout for {nd} joints ({OBS_JOINTS + 3 * nd}"
                         + (f" x {H} frames)" if H > 1 else ")"))
    num_obs = total // H
    q0 = np.asarray(default_dof_pos, dtype=np.float64).reshape(-1)
    if not np.array_equal(act_sign * q0[act_src], q0):
        raise ValueError(f"symmetry loss: the default joint pose {q0.tolist()} is not its own mirror image")
    obs_src = np.arange(num_obs, dtype=np.int32)
    obs_sign = np.ones(num_obs, dtype=np.float32)
    obs_sign[[1, 3, 5, 7, 8, 9, 10]] = -1.0  # gravity y; angular velocity x, z; commands vy, yaw rate; gait clock cos, sin
    for k in range(3):
        blk = OBS_JOINTS + k * nd
        obs_src[blk : blk + nd] = blk + act_src
        obs_sign[blk : blk + nd] = act_sign
    if H > 1:
        obs_src = np.concatenate([obs_src + k * num_obs for k in range(H)]).astype(np.int32)
        obs_sign = np.tile(obs_sign, H)
    if len(scan_src):
        obs_src = np.concatenate([obs_src, total + scan_src]).astype(np.int32)
        obs_sign = np.concatenate([obs_sign, np.ones(len(scan_src), dtype=np.float32)])
    return obs_src, obs_sign, act_src, act_sign


def signed_permutation(src, sign):
    """The matrix M of (src, sign): M[i, src[i]] = sign[i] (float64)."""
    n = len(src)
    m = np.zeros((n, n))
    m[np.arange(n), np.asarray(src)] = np.asarray(sign, dtype=np.float64)
    return m
