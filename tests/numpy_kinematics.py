"""A float64 numpy restatement of the kinematic observations (rr_kinematic_observations), for the tests (a helper module: pytest
does not collect it).

It takes another road than the kernel: the forward kinematics of tests/numpy_step.py (its dtype follows q) evaluated at
q + i h e_k, so that

* the linear Jacobian of a point held fixed in its link's COM frame is Im(x(q + i h e_k)) / h, and
* the angular one comes from the skew matrix dR/dq_k R^T of the link's rotation

-- not the axis x lever expression the device uses.  Velocities are J @ qd.  Quaternions come from the link's rotation matrix by
the "largest of four squares" rule, not by the trace branches of the device's m3_to_quat (the sign of a quaternion is free:
compare after aligning it).
"""
import numpy as np

from tests import numpy_step as ns

NL = 17


def _link_frames(q):
    """COM frames of the 17 URDF links for q [..., 11] (real or complex): R [..., 17, 3, 3], p [..., 17, 3]."""
    m = ns.model()
    Rb, pb, _ = ns.forward(q)
    sh = Rb.shape[:-3]
    R = np.zeros(sh + (NL, 3, 3), Rb.dtype)
    p = np.zeros(sh + (NL, 3), Rb.dtype)
    for l in range(NL):
        b = int(m['link_body'][l])
        if b < 0:
            R[..., l, :, :] = m['link_rot'][l]
            p[..., l, :] = m['robot_pos'] + m['link_pos'][l]
        else:
            R[..., l, :, :] = Rb[..., b, :, :] @ m['link_rot'][l]
            p[..., l, :] = pb[..., b, :] + Rb[..., b, :, :] @ m['link_pos'][l]
    return R, p


def mat_to_quat(R):
    """xyzw quaternions of rotation matrices [..., 3, 3]: the largest of the four squared components is rooted, the other three
    follow from the off-diagonal sums and differences."""
    R = np.asarray(R, dtype=np.float64)
    r = lambda i, j: R[..., i, j]
    sq = np.stack([1 + r(0, 0) - r(1, 1) - r(2, 2), 1 - r(0, 0) + r(1, 1) - r(2, 2), 1 - r(0, 0) - r(1, 1) + r(2, 2),
                   1 + r(0, 0) + r(1, 1) + r(2, 2)], -1) / 4                                    # x^2, y^2, z^2, w^2
    # 4 * (component a) * (component b) for every pair
    prod = {(0, 1): r(0, 1) + r(1, 0), (0, 2): r(0, 2) + r(2, 0), (1, 2): r(1, 2) + r(2, 1),
            (0, 3): r(2, 1) - r(1, 2), (1, 3): r(0, 2) - r(2, 0), (2, 3): r(1, 0) - r(0, 1)}
    big = sq.argmax(-1)
    out = np.zeros(R.shape[:-2] + (4,))
    for a in range(4):
        root = np.sqrt(np.maximum(sq[..., a], 0.0))
        cand = np.zeros_like(out)
        for b in range(4):
            cand[..., b] = root if a == b else prod[(min(a, b), max(a, b))] / (4 * np.where(root > 0, root, 1.0))
        out = np.where((big == a)[..., None], cand, out)
    return out


def ancestors(links):
    """anc [len(links), 11]: 1.0 where joint k moves the link (its body and that body's ancestors), all zero for a link that is
    rigid with the world."""
    m = ns.model()
    out = np.zeros((len(links), ns.NB))
    for i, l in enumerate(links):
        b = int(m['link_body'][int(l)])
        if b >= 0:
            out[i] = m['anc'][b]
    return out


def observations(state, links=(8,), local_pos=None):
    """The seven fields for state [N, 61] (any float dtype; taken as float64) and the points (links [P], local_pos [P, 3] or None):
    a dict with link_pos [N, 17, 3], link_quat [N, 17, 4], link_jac [N, 17, 6, 11], link_vel [N, 17, 6], point_pos [N, P, 3],
    point_jac [N, P, 6, 11], point_vel [N, P, 6], joint_vel [N, 11], obj_vel [N, 3, 6]."""
    st = np.asarray(state, dtype=np.float64)
    q, qd = st[:, :11], st[:, 11:22]
    links = np.asarray(links, dtype=np.int64)
    local = np.zeros((len(links), 3)) if local_pos is None else np.asarray(local_pos, dtype=np.float64)
    h = ns.CS_H

    def positions(R, p):          # the 17 frame origins, then the points: [..., 17 + P, 3]
        x = p[..., links, :] + np.einsum('...pij,pj->...pi', R[..., links, :, :], local)
        return np.concatenate([p, x], -2)

    R, p = _link_frames(q)
    X = positions(R, p)
    n_items = NL + len(links)
    J = np.zeros((len(st), n_items, 6, ns.NB))
    item_link = np.concatenate([np.arange(NL), links])
    qc = ns._cs_points(q)
    for k in range(ns.NB):
        Rk, pk = _link_frames(qc[k])
        J[:, :, :3, k] = positions(Rk, pk).imag / h
        W = np.einsum('...ij,...kj->...ik', Rk.imag / h, R)          # dR/dq_k R^T: the skew matrix of the angular column
        w = np.stack([W[..., 2, 1], W[..., 0, 2], W[..., 1, 0]], -1)
        J[:, :, 3:, k] = w[:, item_link, :]
    V = np.einsum('nirk,nk->nir', J, qd)
    ov = np.stack([st[:, 22 + 13 * o + 7:22 + 13 * o + 13] for o in range(3)], 1)
    return dict(link_pos=X[:, :NL], link_quat=mat_to_quat(R), link_jac=J[:, :NL], link_vel=V[:, :NL], point_pos=X[:, NL:],
                point_jac=J[:, NL:], point_vel=V[:, NL:], joint_vel=qd.copy(), obj_vel=ov)
