"""A float64 numpy restatement of the inverse kinematics at candidate targets (rr_posture_ik, include/realrobot.h), for the tests (a
helper module: pytest does not collect it).

The algorithm of the header, for any kinematic point (link, position in the link's COM frame), vectorised over rows:

* forward kinematics: tests/numpy_step.py `forward` (the road of tests/numpy_kinematics.py);
* the tool frame: the point's world position, the orientation of its link's COM frame;
* Jacobian column k of the seven arm joints: [a_k x (x - p_k); a_k] if joint k moves the point's link, zero otherwise;
* residual: (target - x, half the antisymmetric part of Rt Re^T) -- oracle/kinematics.py `pose_residual`; position only: target - x;
* update: dq = J^T (J J^T + lambda^2 I)^-1 e by numpy.linalg.solve, scaled to |dq|inf <= max_step, then the clamp into body_limits[:7]
  (the seed is clamped first) or the wrap to (-pi, pi];
* the residual is evaluated before each update and once more after the last; status 0: residual < tolerance and, in full-pose mode,
  (trace(Rt Re^T) - 1) / 2 > 0; status 1: the cap; status 2: a residual that is not finite.

Also the fixture of the tests: goals uniform within the limits, targets their forward kinematics, seeds the goals plus U(-0.3, 0.3).
"""
import numpy as np

from tests import numpy_step as ns

ARM = 7
EE_LINK = 8                  # gripper `base`: the point of a fresh handle
FIX_N, FIX_K, FIX_SEED = 5, 32, 20261020
FIX_MAX_ITERATIONS = 64
CLEAR_CUT = 32               # a row the restatement solves within this many updates is clear-cut


def quat_to_mat(q):
    """Rotation matrices [..., 3, 3] of xyzw quaternions [..., 4], normalised here."""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all='ignore'):
        q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = (q[..., i] for i in range(4))
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def tool_frame(q, link=EE_LINK, local=None):
    """For q [..., 11]: Re [..., 3, 3], x [..., 3] of the tool frame and its 6 x 7 Jacobian over the arm joints [..., 6, 7]."""
    m = ns.model()
    q = np.asarray(q, dtype=np.float64)
    local = np.zeros(3) if local is None else np.asarray(local, dtype=np.float64)
    R, p, ax = ns.forward(q)
    b = int(m['link_body'][link])
    off = m['link_pos'][link] + m['link_rot'][link] @ local
    if b < 0:
        Re = np.broadcast_to(m['link_rot'][link], q.shape[:-1] + (3, 3))
        x = np.broadcast_to(m['robot_pos'] + off, q.shape[:-1] + (3,))
        moves = np.zeros(ARM)
    else:
        Re = R[..., b, :, :] @ m['link_rot'][link]
        x = p[..., b, :] + np.einsum('...ij,j->...i', R[..., b, :, :], off)
        moves = m['anc'][b, :ARM]
    a = ax[..., :ARM, :] * moves[:, None]
    lin = np.cross(a, x[..., None, :] - p[..., :ARM, :])
    J = np.concatenate([np.swapaxes(lin, -1, -2), np.swapaxes(a, -1, -2)], -2)
    return Re, x, J


def errors(q, targets, link=EE_LINK, local=None):
    """What a result row reports for the posture q [..., 11] against targets [..., 7], in float64: dict(e [..., 6] the full residual
    vector, position_error, orientation_error (the true angle), full (|e|), cos ((trace(Rt Re^T) - 1) / 2))."""
    targets = np.asarray(targets, dtype=np.float64)
    with np.errstate(all='ignore'):
        Re, x, _ = tool_frame(q, link, local)
        Rerr = quat_to_mat(targets[..., 3:]) @ np.swapaxes(Re, -1, -2)
        w = 0.5 * np.stack([Rerr[..., 2, 1] - Rerr[..., 1, 2], Rerr[..., 0, 2] - Rerr[..., 2, 0], Rerr[..., 1, 0] - Rerr[..., 0, 1]], -1)
        ep = targets[..., :3] - x
        cos = 0.5 * (Rerr[..., 0, 0] + Rerr[..., 1, 1] + Rerr[..., 2, 2] - 1.0)
        e = np.concatenate([ep, w], -1)
        return dict(e=e, position_error=np.linalg.norm(ep, axis=-1), orientation_error=np.arctan2(np.linalg.norm(w, axis=-1), cos),
                    full=np.linalg.norm(e, axis=-1), cos=cos)


def solve(targets, seeds, link=EE_LINK, local=None, max_iterations=32, tolerance=1e-3, damping=0.1, max_step=0.5, position_only=False,
          clamp=True):
    """The header's algorithm on rows targets [R, 7], seeds [R, 11] in float64.  Returns dict(posture [R, 11], residual,
    position_error, orientation_error, cos [R], status, iterations [R] int)."""
    m = ns.model()
    lim = m['body_limits'][:ARM]
    t = np.asarray(targets, dtype=np.float64)
    q = np.array(seeds, dtype=np.float64)
    rows = len(q)
    if clamp:
        fin = np.isfinite(q[:, :ARM])
        q[:, :ARM] = np.where(fin, np.clip(q[:, :ARM], lim[:, 0], lim[:, 1]), q[:, :ARM])
    status = np.ones(rows, np.int64)
    iterations = np.zeros(rows, np.int64)
    active = np.ones(rows, bool)
    M = 3 if position_only else 6
    for it in range(int(max_iterations) + 1):
        with np.errstate(all='ignore'):
            err = errors(q, t, link, local)
            _, _, J = tool_frame(q, link, local)
        res = err['position_error'] if position_only else err['full']
        bad = active & ~np.isfinite(res)
        done = active & ~bad & (res < tolerance) & (position_only | (err['cos'] > 0))
        status[bad], status[done] = 2, 0
        active &= ~(bad | done)
        iterations[active] = it
        if it == max_iterations or not active.any():
            break
        idx = np.flatnonzero(active)
        Ja, ea = J[idx, :M], err['e'][idx, :M]
        x = np.linalg.solve(Ja @ np.swapaxes(Ja, -1, -2) + damping * damping * np.eye(M), ea[..., None])
        dq = (np.swapaxes(Ja, -1, -2) @ x)[..., 0]
        n = np.abs(dq).max(-1)
        dq *= np.where(n > max_step, max_step / np.where(n > 0, n, 1.0), 1.0)[:, None]
        v = q[idx, :ARM] + dq
        v = np.clip(v, lim[:, 0], lim[:, 1]) if clamp else np.pi - np.mod(np.pi - v, 2 * np.pi)
        moved = np.abs(J[idx, 3:]).max(-2) > 0           # (an axis is a unit vector: a zero column is a joint that does not move the link)
        q[idx, :ARM] = np.where(moved, v, q[idx, :ARM])
        iterations[idx] = it + 1
    return dict(posture=q, residual=res, position_error=err['position_error'], orientation_error=err['orientation_error'], cos=err['cos'],
                status=status, iterations=iterations)


def fixture(link=EE_LINK, local=None, N=FIX_N, K=FIX_K, seed=FIX_SEED):
    """(targets float32 [N, K, 7], seeds float32 [N, K, 11], goals float64 [N, K, 11]): the goal's joints uniform within body_limits,
    the seed's arm joints the goal's plus U(-0.3, 0.3) clipped to the limits (its fingers are the goal's), both rounded to float32;
    the target is the float64 tool pose of the float32 goal."""
    from tests.numpy_kinematics import mat_to_quat
    lim = ns.model()['body_limits']
    rng = np.random.default_rng(seed)
    goal = rng.uniform(lim.min(1), lim.max(1), (N, K, ns.NB)).astype(np.float32)
    seeds = goal.astype(np.float64)
    seeds[..., :ARM] = np.clip(seeds[..., :ARM] + rng.uniform(-0.3, 0.3, (N, K, ARM)), lim[:ARM, 0], lim[:ARM, 1])
    seeds = seeds.astype(np.float32)
    seeds[..., :ARM] = np.clip(seeds[..., :ARM], lim[:ARM, 0].astype(np.float32), lim[:ARM, 1].astype(np.float32))
    Re, x, _ = tool_frame(goal.astype(np.float64), link, local)
    targets = np.concatenate([x, mat_to_quat(Re)], -1).astype(np.float32)
    return targets, seeds, goal.astype(np.float64)
