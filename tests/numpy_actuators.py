"""A float64 step with PER-JOINT actuators (kp, kd, max_force, joint damping arrays of 11), for the per-env actuator tests.

tests/numpy_step.py takes the motor constants as scalars; this helper is built from its public pieces -- `prep` (M^-1, bias, the
objects' terms), `motor_targets`, the link Jacobians, `contact_material`, `warm_start`, `plane_space` -- and restates only the row
assembly and the Gauss-Seidel loop of `numpy_step.step`, in the same order with the same arithmetic, with
    qd* = qd + dt M^-1 (-bias - damping * qd)
recomputed from prep's Minv and bias under the per-joint damping.  With arrays that are constant over the joints it reproduces
`numpy_step.step(..., solver={...})` exactly (tests/test_numpy_actuators.py).  Not collected by pytest.
"""
import numpy as np

from tests import numpy_step as ns
from tests.numpy_step import DT, NB


def per_joint(v, default):
    """A scalar, an array of 11 or None (-> default) as a float64 array of 11."""
    return np.broadcast_to(np.asarray(default if v is None else v, dtype=np.float64), (NB,)).copy()


def unconstrained_velocities(pr, qd, damping):
    """qd* under a per-joint damping, from prep's M^-1 and bias (numpy_step.prep's expression with the array in the blob's place)."""
    return qd + DT * np.einsum('...ij,...j->...i', pr['Minv'], -pr['bias'] - damping * qd)


def step(state, action, contacts, kp=None, kd=None, max_force=None, damping=None, dyn=None, prev=None, solver=None, solver_iters=50,
         nobj=3, home=None):
    """numpy_step.step with per-joint kp / kd / max_force / damping (scalars or arrays of 11 in the order of q[11]; None: the
    value of `solver` / the model's body_damping).  Returns dict(state (61), lambda_n [n], rows, lam (every row's impulse; the
    first 11 are the motors'), mat, prep, qds (the unconstrained joint velocities), vt (the motors' target velocities))."""
    P = dict(ns.SOLVER_DEFAULTS, **(solver or {}))
    m = ns.model()
    kp, kd = per_joint(kp, P['motor_kp']), per_joint(kd, P['motor_kd'])
    max_force, damping = per_joint(max_force, P['motor_max_force']), per_joint(damping, m['body_damping'])
    dyn = ns.default_dynamics(nobj) if dyn is None else np.asarray(dyn, dtype=np.float64)
    s = np.array(state, dtype=np.float64)
    contacts = np.asarray(contacts, dtype=np.float64).reshape(-1, 12)
    q, qd = s[:NB].copy(), s[NB:2 * NB]
    pr = ns.prep(s, dyn, P, nobj, home=home)
    tgt = ns.motor_targets(q, action, P['rate_limit'])
    R, p, Minv = pr['R'], pr['p'], pr['Minv']
    qds = unconstrained_velocities(pr, qd, damping)
    nd = NB + 6 * nobj
    W = np.zeros((nd, nd))
    W[:NB, :NB] = Minv
    ustar = np.concatenate([qds] + [np.concatenate([pr['ovs'][i], pr['ows'][i]]) for i in range(nobj)])
    for i in range(nobj):
        o = NB + 6 * i
        W[o:o + 3, o:o + 3] = np.eye(3) / dyn[i][0]
        W[o + 3:o + 6, o + 3:o + 6] = pr['oIinv'][i]
    jac = ns._link_jacobians(q, R, p)
    rows = []                      # (kind, ref, J, rhs, lo, hi, normal row index or -1, coefficient, W J, 1 / diag)

    def add(kind, ref, J, rhs_of, lo, hi, nrow=-1, coef=0.0):
        WJ = W @ J
        diag = J @ WJ
        dinv = 1.0 / diag if diag > 0 else 0.0
        rows.append([kind, ref, J, rhs_of(J @ ustar) * dinv, lo, hi, nrow, coef, WJ, dinv])

    vts = np.zeros(NB)
    for j in range(NB):
        hi_m = max_force[j] * DT
        vt = kp[j] * (tgt[j] - q[j]) / DT + qds[j] + kd[j] * (0 - qds[j])
        vts[j] = vt
        add('motor', (j,), np.eye(nd)[j], lambda rel, vt=vt: vt - rel, -hi_m, hi_m)
    for j in range(NB):
        lo_, hi_ = m['body_limits'][j]
        if not lo_ < hi_:
            continue
        for side, (dist, sg) in enumerate(((q[j] - lo_, 1.0), (hi_ - q[j], -1.0))):
            if dist >= ns.LIMIT_WINDOW:
                continue

            def rhs_lim(rel, dist=dist):
                return (-rel - dist / DT) if dist > 0 else (-dist * P['erp'] / DT - rel)
            add('limit', (j, side), sg * np.eye(nd)[j], rhs_lim, 0.0, ns.LIMIT_MAX_IMPULSE)

    def contact_J(c, d, angular):
        J = np.zeros(nd)
        x = c[3:6]
        for body, sg in ((int(c[0]), 1.0), (int(c[1]), -1.0)):
            if body < 0:
                continue
            if body < 16:
                Jv, Jw = jac(body, x)
                J[:NB] += sg * (d @ (Jw if angular else Jv))
            else:
                o = NB + 6 * (body - 16)
                if not angular:
                    J[o:o + 3] += sg * d
                    J[o + 3:o + 6] += sg * np.cross(x - pr['opos'][body - 16], d)
                else:
                    J[o + 3:o + 6] += sg * d
        return J

    mats = np.array([ns.contact_material(c, dyn) for c in contacts]).reshape(-1, 4)
    normal_rows = []
    for ci, c in enumerate(contacts):
        dist, rest = c[9], mats[ci][1]

        def rhs_n(rel, dist=dist, rest=rest):
            r = max(rest * -rel, 0.0) if abs(rel) >= ns.REST_THRESHOLD else 0.0
            return (r - rel - dist / DT) if dist > 0 else (-dist * P['erp'] / DT + r - rel)
        normal_rows.append(len(rows))
        add('normal', (ci,), contact_J(c, c[6:9], False), rhs_n, 0.0, ns.NORMAL_MAX_IMPULSE)
    for ci, c in enumerate(contacts):
        for k, t in enumerate(ns.plane_space(c[6:9])):
            add('friction', (ci, k), contact_J(c, t, False), lambda rel: -rel, 0.0, 0.0, normal_rows[ci], mats[ci][0])
    for ci, c in enumerate(contacts):
        t1, t2 = ns.plane_space(c[6:9])
        for k, (axis, coef) in enumerate(((c[6:9], mats[ci][3]), (t1, mats[ci][2]), (t2, mats[ci][2]))):
            if coef > 0:
                add('torsional', (ci, k), contact_J(c, axis, True), lambda rel: -rel, 0.0, 0.0, normal_rows[ci], coef)
    lam = np.zeros(len(rows))
    du = np.zeros(nd)
    lam0 = ns.warm_start(contacts, prev, P['warmstart'])
    for ci, r in enumerate(normal_rows):
        if lam0[ci] > 0:
            lam[r] = lam0[ci]
            du += rows[r][8] * lam0[ci]
    for _ in range(int(solver_iters)):
        for k in range(len(rows)):
            kind, ref, J, rhs, lo, hi, nrow, coef, WJ, dinv = rows[k]
            if nrow >= 0:
                hi = coef * lam[nrow]
                lo = -hi
            new = min(max(lam[k] + rhs - (J @ du) * dinv, lo), hi)
            dl = new - lam[k]
            lam[k] = new
            du += WJ * dl
    u = ustar + du
    out = s.copy()
    out[NB:2 * NB] = u[:NB]
    out[:NB] = q + DT * u[:NB]
    for i in range(nobj):
        v, w = u[NB + 6 * i:NB + 6 * i + 3], u[NB + 6 * i + 3:NB + 6 * i + 6]
        pos = pr['opos'][i] + DT * v
        wn = np.linalg.norm(w)
        h = np.concatenate([w / wn * np.sin(wn * DT / 2), [np.cos(wn * DT / 2)]]) if wn > 0 else np.array([0, 0, 0, 1.0])
        qo = pr['oquat'][i]
        qn = np.array([h[3] * qo[0] + h[0] * qo[3] + h[1] * qo[2] - h[2] * qo[1],
                       h[3] * qo[1] - h[0] * qo[2] + h[1] * qo[3] + h[2] * qo[0],
                       h[3] * qo[2] + h[0] * qo[1] - h[1] * qo[0] + h[2] * qo[3],
                       h[3] * qo[3] - h[0] * qo[0] - h[1] * qo[1] - h[2] * qo[2]])
        out[2 * NB + 13 * i:2 * NB + 13 * (i + 1)] = np.concatenate([pos, qn / np.linalg.norm(qn), v, w])
    return dict(state=out, lambda_n=lam[normal_rows] if normal_rows else np.zeros(0), rows=[(r[0],) + r[1] for r in rows],
                lam=lam, mat=mats, prep=pr, qds=qds, vt=vts)
