"""CPU checker of the K8 row (numpy, float64): forward kinematics, geometric Jacobian, the damped-least-squares IK for
link 7 (gripper `base`) and the 1000-step macro plan -- the host restatement of what the reference asks pybullet for in
step_cartesian / generate_plan (real_robots/envs/env.py:372-375, 388-454, 422-427:
calculateInverseKinematics(0, 7, pos, orn, maxNumIterations=1000, residualThreshold=0.001)).

TEST INFRASTRUCTURE ONLY (like everything under oracle/): the product path plans and solves IK on the device
(k_ik, k_plan_macro in real_robots_amd/csrc/realrobot.hip) and never imports this module.  "parity unpinned" w.r.t.
PyBullet: pybullet's IK branch choice is an implementation detail of its solver; the selection rule below is the one the
device implements and the reference's tracking known answers (tests/test_actions.py:147-152) are what pins both.
"""
import numpy as np

from real_robots_amd.mathutil import quat_from_euler  # noqa: F401  (re-exported for the tests)
from real_robots_amd.model import load_model          # reader of the compiled model DATA (no arithmetic)

PARENT = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 9]
EE_LINK = 8          # URDF depth-first id of gripper `base` (pybullet link index 7), rigidly attached to body 6


def _axis_angle(a, ang):
    c, s = np.cos(ang), np.sin(ang)
    t = 1 - c
    x, y, z = a
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
                     [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]])


def quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


_chain = None


def _chain_f64():
    """The model's chain constants in float64, converted once (the values of load_model(), no arithmetic)."""
    global _chain
    if _chain is None:
        m = load_model()
        b = int(m['link_body'][EE_LINK])
        _chain = dict(robot_pos=m['robot_pos'].astype(np.float64), jrot=[m['body_jrot'][i].astype(np.float64) for i in range(11)],
                      axis=[m['body_axis'][i].astype(np.float64) for i in range(11)],
                      jpos=[m['body_jpos'][i].astype(np.float64) for i in range(11)],
                      ee_body=b, ee_rot=m['link_rot'][EE_LINK].astype(np.float64), ee_pos=m['link_pos'][EE_LINK].astype(np.float64))
    return _chain


def forward(q11, nbodies=11):
    """Returns (R[11,3,3], p[11,3], axis_world[11,3]) of the 11 moving bodies (the first `nbodies` filled in)."""
    c = _chain_f64()
    R = np.zeros((11, 3, 3))
    p = np.zeros((11, 3))
    ax = np.zeros((11, 3))
    for b in range(nbodies):
        if PARENT[b] < 0:
            Rp, pp = np.eye(3), c['robot_pos']
        else:
            Rp, pp = R[PARENT[b]], p[PARENT[b]]
        Rj = Rp @ c['jrot'][b]
        a = c['axis'][b]
        p[b] = pp + Rp @ c['jpos'][b]
        R[b] = Rj @ _axis_angle(a, q11[b])
        ax[b] = Rj @ a
    return R, p, ax


def link_pose(q11, link):
    """World (R, p) of the COM frame of robot link `link` (URDF depth-first id)."""
    m = load_model()
    b = int(m['link_body'][link])
    lr = m['link_rot'][link].astype(np.float64)
    lp = m['link_pos'][link].astype(np.float64)
    if b < 0:
        return lr, m['robot_pos'].astype(np.float64) + lp
    R, p, _ = forward(q11)
    return R[b] @ lr, p[b] + R[b] @ lp


def ee_jacobian(q11):
    """6x7 geometric Jacobian (linear; angular) of the gripper base frame w.r.t. the 7 arm joints."""
    R, p, ax = forward(q11, 7)                            # the arm: bodies 0..6 (the gripper base rides on body 6)
    c = _chain_f64()
    b = c['ee_body']                                      # (link_pose(q11, EE_LINK) without a second pass over the chain)
    Re, pe = R[b] @ c['ee_rot'], p[b] + R[b] @ c['ee_pos']
    J = np.zeros((6, 7))
    a, r = ax[:7], pe - p[:7]
    J[0] = a[:, 1] * r[:, 2] - a[:, 2] * r[:, 1]          # cross(axis, lever), all seven joints at once
    J[1] = a[:, 2] * r[:, 0] - a[:, 0] * r[:, 2]
    J[2] = a[:, 0] * r[:, 1] - a[:, 1] * r[:, 0]
    J[3:] = a.T
    return J, Re, pe


ELBOW_UP_SEED = np.array([0.0, 0.6, 0.0, -1.3, 0.0, 1.2, 0.0])


def pose_residual(Re, pe, target_pos, Rt):
    """The 6-vector the solver drives to zero (the device's definition, rr_ik.inc ik_dls): position error, then half the
    antisymmetric part of Rt Re^T (sin(angle) x axis of the orientation error)."""
    dp = np.asarray(target_pos, dtype=np.float64) - pe
    Rerr = Rt @ Re.T
    w = 0.5 * np.array([Rerr[2, 1] - Rerr[1, 2], Rerr[0, 2] - Rerr[2, 0], Rerr[1, 0] - Rerr[0, 1]])
    return np.concatenate([dp, w])


def ee_residual(q11, target_pos, target_quat):
    """Float64 residual norm of the gripper base at joints q11 against a target pose (position and orientation)."""
    Re, pe = link_pose(np.asarray(q11, dtype=np.float64), EE_LINK)
    Rt = quat_to_mat(np.asarray(target_quat, dtype=np.float64) / np.linalg.norm(target_quat))
    return float(np.linalg.norm(pose_residual(Re, pe, target_pos, Rt)))


def _dls(q, target_pos, Rt, max_iters, residual, damping, prev=None):
    """Returns (q, residual, number of updates applied: max_iters when the run never met the threshold).
    `prev` (a list): receives the iterate before the last update and its residual -- where a float32 solver whose residual
    crosses the threshold one iteration earlier stops."""
    lam2 = damping * damping
    err = np.inf
    iters = int(max_iters)
    for it in range(int(max_iters)):
        J, Re, pe = ee_jacobian(q)
        e = pose_residual(Re, pe, target_pos, Rt)
        err = np.linalg.norm(e)
        if err < residual:
            iters = it
            break
        if prev is not None:
            prev[:] = [q.copy(), float(err)]
        dq = J.T @ np.linalg.solve(J @ J.T + lam2 * np.eye(6), e)
        n = np.abs(dq).max()
        if n > 0.5:
            dq *= 0.5 / n
        q[:7] += dq
        q[:7] = (q[:7] + np.pi) % (2 * np.pi) - np.pi
    return q, err, iters


def inverse_kinematics(q11, target_pos, target_quat, max_iters=1000, residual=1e-3, damping=0.1, prefer=None, single_seed=False):
    """Damped least squares IK for link 7 (gripper base) position + orientation; returns all 11 dofs like pybullet
    does (the fingers keep their current values).  pybullet seeds DLS with the current joints and the branch it lands
    on is an implementation detail of its solver; here two seeds are tried (current joints, a canonical elbow-up
    posture) and, among the converged ones, the solution with the highest elbow (link_4 origin) is returned -- the
    collision-free branch the reference's tracking test expects (tests/test_actions.py:147-152)."""
    q0 = np.array(q11, dtype=np.float64)
    Rt = quat_to_mat(np.asarray(target_quat, dtype=np.float64) / np.linalg.norm(target_quat))
    best, best_key = None, None
    seeds = [q0[:7], ELBOW_UP_SEED] + ([np.asarray(prefer, dtype=np.float64)[:7]] if prefer is not None else [])
    if single_seed:                # the reference's literal semantics: ONE solve from the simulator's current joints (env.py:372-375, 421-427)
        seeds = seeds[:1]
    for seed in seeds:
        q = q0.copy()
        q[:7] = seed
        q, err, _ = _dls(q, target_pos, Rt, max_iters, residual, damping)
        _, p, _ = forward(q)
        if prefer is not None:     # continuity with the previous way-point of a plan
            key = (err < 10 * residual, -float(np.abs(q[:7] - np.asarray(prefer)[:7]).max()))
        else:                      # converged first, then elbow height
            key = (err < 10 * residual, p[3][2])
        if best is None or key > best_key:
            best, best_key = q, key
    return best


def ik_candidates(q11, target_pos, target_quat, prefer=None, max_iters=1000, residual=1e-3, damping=0.1, single_seed=False):
    """Every seed's DLS result [(q11, residual, key, q11 one update earlier, its residual, updates applied)] in seed order (current joints,
    elbow-up, previous way-point) -- lets a test tell a branch disagreement (another seed won on a near-tie of the keys) or a
    stop one iteration apart (residual within rounding of the threshold) from an arithmetic disagreement."""
    q0 = np.array(q11, dtype=np.float64)
    Rt = quat_to_mat(np.asarray(target_quat, dtype=np.float64) / np.linalg.norm(target_quat))
    seeds = [q0[:7], ELBOW_UP_SEED] + ([np.asarray(prefer, dtype=np.float64)[:7]] if prefer is not None else [])
    if single_seed:
        seeds = seeds[:1]
    out = []
    for seed in seeds:
        q = q0.copy()
        q[:7] = seed
        prev = []
        q, err, iters = _dls(q, target_pos, Rt, max_iters, residual, damping, prev)
        _, p, _ = forward(q)
        key = -float(np.abs(q[:7] - np.asarray(prefer)[:7]).max()) if prefer is not None else float(p[3][2])
        out.append((q, float(err), key, prev[0] if prev else q, prev[1] if prev else float(err), iters))
    return out


def segment_count(point_1, point_2, steps=500):
    """interpolate3D's number of IK segments for the p1 -> p2 rows (env.py:433), in float64 on the inputs as given."""
    dist = np.linalg.norm(np.asarray(point_2, dtype=np.float64) - np.asarray(point_1, dtype=np.float64))
    return min(int(dist / 0.05) + 1, steps)


def plan_way_points(macro_action):
    """The IK way points of a macro plan in the order they are solved, [(first plan row, target xyz)]: above p1 (row 100), at p1
    (200), the end of every p1 -> p2 segment (250 + i * chunk), above p2 (750).  Each one's rows run up to the next one's first
    row; the last segment also holds the remainder rows up to 749; above p2 holds 750-799."""
    p1, p2 = np.asarray(macro_action[0], dtype=np.float64), np.asarray(macro_action[1], dtype=np.float64)
    pieces = segment_count(p1, p2)
    chunk = 500 // pieces
    coords = np.linspace(np.hstack([p1, 0.46]), np.hstack([p2, 0.46]), pieces + 1)
    return ([(100, np.hstack([p1, 0.6])), (200, np.hstack([p1, 0.46]))] + [(250 + i * chunk, c) for i, c in enumerate(coords[1:])] +
            [(750, np.hstack([p2, 0.6]))])


def generate_plan(q_seed11, macro_action, single_seed=False):
    """The reference's 1000-step macro plan of 9-vectors (real_robots/envs/env.py:388-454): 100x home2, 100x above
    p1 (z 0.6), 50x at p1 (z 0.46), 500x p1->p2 at z 0.46 in <= 5 cm IK segments, 50x above p2, 100x home2, 100x home.
    IK orientation getQuaternionFromEuler([0, 3.14, -1.57]) (env.py:422); each IK result is cut to its first 9 dofs
    (env.py:427).  single_seed: every way point from ONE solve seeded with q_seed11 (the reference calls calculateInverseKinematics once per
    way point without stepping in between: every call starts from the same current joints) instead of the best of several seeds."""
    point_1, point_2 = np.asarray(macro_action[0], dtype=np.float64), np.asarray(macro_action[1], dtype=np.float64)
    home = np.zeros(9)
    home2 = np.zeros(9)
    home2[5] = np.pi / 2
    home2[6] = np.pi / 2
    orient = quat_from_euler(0, 3.14, -1.57)
    q_seed = np.asarray(q_seed11, dtype=np.float64)

    last = [None]

    def goToPosXY(coords):
        q = inverse_kinematics(q_seed, coords, orient, prefer=last[0], single_seed=single_seed)
        last[0] = q
        return q[:9].copy()

    def interpolate3D(p1, p2, steps):
        p1, p2 = np.array(p1), np.array(p2)
        dist = np.linalg.norm(p2 - p1)
        pieces = min(int(dist / 0.05) + 1, steps)
        coords = np.linspace(p1, p2, pieces + 1)
        joints = np.zeros((steps, 9))
        chunk = int(steps / pieces)
        for i, coord in enumerate(coords[1:]):
            joints[i * chunk:, :] = goToPosXY(coord)
        return joints

    # way-points are solved in path order so that each IK prefers the branch closest to the previous one
    point_1_h = goToPosXY(np.hstack([point_1, 0.6]))
    point_1_l = goToPosXY(np.hstack([point_1, 0.46]))
    middle = interpolate3D(np.hstack([point_1, 0.46]), np.hstack([point_2, 0.46]), 500)
    point_2_h = goToPosXY(np.hstack([point_2, 0.6]))
    parts = [np.tile(home2, (100, 1)), np.tile(point_1_h, (100, 1)), np.tile(point_1_l, (50, 1)), middle,
             np.tile(point_2_h, (50, 1)), np.tile(home2, (100, 1)), np.tile(home, (100, 1))]
    return np.vstack(parts)


