"""A float64 numpy restatement of one REALRobot step, for the tests (a helper module: pytest does not collect it).

Built from the compiled model's data (real_robots_amd.model.load_model) and the documented Bullet semantics only -- it calls
nothing of the oracle (oracle/rr_oracle.c) or of the HIP kernels, and where it can it takes another road than they do:

* forward kinematics whose dtype follows q, so that a complex q gives complex-step derivatives;
* M(q) = sum_b m_b Jv_b^T Jv_b + Jw_b^T I_b Jw_b, and the bias forces from the Lagrangian,
  b(q, qd) = Mdot qd - 1/2 d(qd^T M qd)/dq + dV/dq, with dM/dq and dV/dq by complex step (exact to rounding) -- the oracle and
  the device run a recursive Newton-Euler pass instead;
* the contact Jacobian of a robot link as the complex-step derivative of the forward kinematics of the contact point held fixed
  in the link frame (linear) and of the link's rotation (angular) -- not the axis x (x - p_joint) expression;
* every row a dense Jacobian over the generalised velocities (11 joints, then 6 per object) against a block-diagonal inverse
  mass, solved by projected Gauss-Seidel in Bullet's order: motors, joint limits, normals, lateral frictions, torsional frictions.

The narrow phase is restated in tests/numpy_collide.py; here the contact points, normals and distances of the step come in as
input (records in the layout of the contact lists: bodyA, bodyB, linkA, x (3), n (3), dist, normal force, mu).  Every function of
the preparation broadcasts over leading batch dimensions (prep() checks whole batches of the device's preparation record).  With
fewer than three objects the state keeps its 61 entries: the slots of the absent objects pass through a step unchanged.
"""
import numpy as np

from real_robots_amd.model import load_model

NB = 11
DT = 0.005
GRAVITY = 9.81
REST_THRESHOLD = 0.2          # m_restitutionVelocityThreshold
WARM_DIST = 0.02              # contact breaking threshold: a new contact inherits from a cached one closer than this
LIMIT_WINDOW = 0.5            # joint-limit rows exist within this distance (rad) of a limit
LIMIT_MAX_IMPULSE = 100.0     # btMultiBodyConstraint m_maxAppliedImpulse
NORMAL_MAX_IMPULSE = 1e10
ROLL_SPIN_MAX = 10.0          # btManifoldResult clamps the combined rolling / spinning friction to 10
CS_H = 1e-20                  # complex step
SOLVER_DEFAULTS = dict(motor_kp=0.1, motor_kd=1.0, motor_max_force=100000.0, warmstart=0.85, lin_damping=0.04,
                       ang_damping=0.04, erp=0.2, rate_limit=True)

_M = None


def model():
    """The model's arrays in float64, plus the ancestor table anc[b, k] (joint k moves body b)."""
    global _M
    if _M is None:
        m = load_model()
        f = lambda k: np.array(m[k], dtype=np.float64)
        d = {k: f(k) for k in ('robot_pos', 'body_jpos', 'body_jrot', 'body_axis', 'body_mass', 'body_com', 'body_damping',
                               'body_limits', 'obj_mass', 'obj_inertia', 'obj_pose0', 'table_pos', 'act_min', 'act_max',
                               'act_maxdiff', 'link_pos', 'link_rot', 'shape_mat', 'shape_roll', 'shape_planes')}
        d['parent'] = [int(x) for x in m['body_parent']]
        d['link_body'] = np.array(m['link_body'], dtype=np.int64)
        d['shape_owner'] = np.array(m['shape_owner'], dtype=np.int64)
        d['shape_nf'] = np.array(m['shape_nf'], dtype=np.int64)
        I6 = f('body_inertia')
        d['body_I'] = np.stack([np.array([[a[0], a[3], a[4]], [a[3], a[1], a[5]], [a[4], a[5], a[2]]]) for a in I6])
        anc = np.zeros((NB, NB))
        for b in range(NB):
            k = b
            while k >= 0:
                anc[b, k] = 1.0
                k = d['parent'][k]
        d['anc'] = anc
        _M = d
    return _M


def _axis_angle(a, ang):
    c, s = np.cos(ang), np.sin(ang)
    t = 1 - c
    x, y, z = a
    rows = [[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
            [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
            [t * x * z - s * y, t * y * z + s * x, t * z * z + c]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def forward(q):
    """Body frames of the 11 moving bodies for q [..., 11]: R [..., 11, 3, 3], joint position p [..., 11, 3], world joint axis
    [..., 11, 3].  The dtype follows q (complex q: complex-step derivatives)."""
    m = model()
    q = np.asarray(q)
    dt = np.result_type(q.dtype, np.float64)
    sh = q.shape[:-1]
    R = np.zeros(sh + (NB, 3, 3), dt)
    p = np.zeros(sh + (NB, 3), dt)
    ax = np.zeros(sh + (NB, 3), dt)
    for b in range(NB):
        pb = m['parent'][b]
        Rp = np.eye(3) if pb < 0 else R[..., pb, :, :]
        pp = m['robot_pos'] if pb < 0 else p[..., pb, :]
        Rj = Rp @ m['body_jrot'][b]
        p[..., b, :] = pp + Rp @ m['body_jpos'][b]
        R[..., b, :, :] = Rj @ _axis_angle(m['body_axis'][b], q[..., b])
        ax[..., b, :] = Rj @ m['body_axis'][b]
    return R, p, ax


def link_pose(q, link):
    """World (R, p) of the COM frame of robot link `link` (URDF depth-first id)."""
    m = model()
    b = int(m['link_body'][link])
    if b < 0:
        return m['link_rot'][link], m['robot_pos'] + m['link_pos'][link]
    R, p, _ = forward(q)
    return R[..., b, :, :] @ m['link_rot'][link], p[..., b, :] + R[..., b, :, :] @ m['link_pos'][link]


def mass_matrix_and_potential(q, g=GRAVITY, frames=None):
    """M(q) = sum_b m_b Jv_b^T Jv_b + Jw_b^T I_b Jw_b (Jv, Jw of each body's centre of mass) and V(q) = sum_b m_b g z_b."""
    m = model()
    R, p, ax = forward(q) if frames is None else frames
    c = p + np.einsum('...bij,bj->...bi', R, m['body_com'])
    Iw = np.einsum('...bij,bjk,...blk->...bil', R, m['body_I'], R)
    d = c[..., :, None, :] - p[..., None, :, :]                                  # [..., body, joint, 3]
    Jv = np.cross(np.broadcast_to(ax[..., None, :, :], d.shape), d) * m['anc'][:, :, None]
    Jw = ax[..., None, :, :] * m['anc'][:, :, None]
    M = np.einsum('b,...bki,...bli->...kl', m['body_mass'], Jv, Jv) + np.einsum('...bki,...bij,...blj->...kl', Jw, Iw, Jw)
    V = g * np.einsum('b,...b->...', m['body_mass'], c[..., 2])
    return M, V


def _cs_points(q):
    """q + i h e_k for k = 0..10: [11, ..., 11] complex."""
    q = np.asarray(q, dtype=np.float64)
    E = np.eye(NB).reshape((NB,) + (1,) * (q.ndim - 1) + (NB,))
    return q[None] + 1j * CS_H * E


def bias(q, qd, g=GRAVITY, coriolis=True):
    """b(q, qd) = Mdot qd - 1/2 d(qd^T M qd)/dq + dV/dq from the Lagrangian, the derivatives of M and V by complex step.
    coriolis=False keeps dV/dq only (a negative control)."""
    q = np.asarray(q, dtype=np.float64)
    qd = np.asarray(qd, dtype=np.float64)
    qc = _cs_points(q)
    dM = np.empty((NB,) + q.shape[:-1] + (NB, NB))
    dV = np.empty((NB,) + q.shape[:-1])
    for k in range(NB):                 # one direction at a time (a 4096-env batch stays small)
        Mc, Vc = mass_matrix_and_potential(qc[k], g)
        dM[k], dV[k] = Mc.imag / CS_H, Vc.imag / CS_H
    b = np.moveaxis(dV, 0, -1)
    if coriolis:
        Mdot = np.einsum('k...ij,...k->...ij', dM, qd)
        b = b + np.einsum('...ij,...j->...i', Mdot, qd) - 0.5 * np.moveaxis(np.einsum('...i,k...ij,...j->k...', qd, dM, qd), 0, -1)
    return b


def quat_to_mat(qt):
    x, y, z, w = (qt[..., i] for i in range(4))
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def default_dynamics(nobj=3):
    """The model's per-object dynamics rows {mass, ixx, iyy, izz, friction, restitution, rolling, spinning} [nobj, 8]."""
    m = model()
    rows = np.zeros((nobj, 8))
    for o in range(nobj):
        s = [s for s in range(len(m['shape_owner'])) if m['shape_owner'][s][0] == 2 and m['shape_owner'][s][1] == o][0]
        rows[o] = np.concatenate([[m['obj_mass'][o]], m['obj_inertia'][o], m['shape_mat'][s], m['shape_roll'][s]])
    return rows


def out_of_bounds(pos):
    """control_objects_limits (env.py:257-264): below the table top, or beyond the table's edge x > 0.11 under z 0.29."""
    m = model()
    x, z = pos[..., 0], pos[..., 2]
    return (z < m['table_pos'][2]) | ((x > 0.11) & (z < 0.29))


def prep(state, dyn, solver=None, nobj=3, coriolis=True, gyroscopic=True, home=None):
    """The preparation of a step from a state [..., 61] and per-env dynamics rows [..., nobj, 8]: body frames, M, M^-1, the
    unconstrained joint velocities qd* = qd + dt M^-1 (-b - damping qd), and per object (after the out-of-bounds re-pose to
    `home` [..., nobj, 7], default the model's start poses) position, quaternion, R, R diag(1/I) R^T, the unconstrained
    velocities (linear and angular damping v (k + k |v|), gravity, the gyroscopic term I^-1 (w x I w))."""
    P = dict(SOLVER_DEFAULTS, **(solver or {}))
    m = model()
    s = np.asarray(state, dtype=np.float64)
    dyn = np.asarray(dyn, dtype=np.float64)
    q, qd = s[..., :NB], s[..., NB:2 * NB]
    R, p, ax = forward(q)
    M, _ = mass_matrix_and_potential(q, frames=(R, p, ax))
    b = bias(q, qd, coriolis=coriolis)
    Minv = np.linalg.inv(M)
    qds = qd + DT * np.einsum('...ij,...j->...i', Minv, -b - m['body_damping'] * qd)
    ob = s[..., 2 * NB:2 * NB + 13 * nobj].reshape(s.shape[:-1] + (nobj, 13))
    pos, quat, v, w = ob[..., :3].copy(), ob[..., 3:7].copy(), ob[..., 7:10].copy(), ob[..., 10:13].copy()
    if home is None:
        home = np.broadcast_to(m['obj_pose0'][:nobj], pos.shape[:-1] + (7,))
    oob = out_of_bounds(pos)
    pos = np.where(oob[..., None], home[..., :3], pos)
    quat = np.where(oob[..., None], home[..., 3:7], quat)
    v = np.where(oob[..., None], 0.0, v)
    w = np.where(oob[..., None], 0.0, w)
    Ro = quat_to_mat(quat)
    Idiag = dyn[..., 1:4]
    Iw = np.einsum('...ij,...j,...kj->...ik', Ro, Idiag, Ro)
    Iinv = np.einsum('...ij,...j,...kj->...ik', Ro, 1.0 / Idiag, Ro)
    kl, ka = P['lin_damping'], P['ang_damping']
    vn = np.linalg.norm(v, axis=-1, keepdims=True)
    wn = np.linalg.norm(w, axis=-1, keepdims=True)
    vs = v + DT * (-v * (kl + kl * vn))
    vs[..., 2] -= DT * GRAVITY
    gyro = np.einsum('...ij,...j->...i', Iinv, np.cross(w, np.einsum('...ij,...j->...i', Iw, w)))
    ws = w + DT * ((-gyro if gyroscopic else 0.0) - w * (ka + ka * wn))
    return dict(R=R, p=p, axis=ax, M=M, bias=b, Minv=Minv, qds=qds, opos=pos, oquat=quat, oR=Ro, oIinv=Iinv, ovs=vs, ows=ws,
                oob=oob)


def motor_targets(q, action, rate_limit=True):
    """The action protocol: limitActionByJoint (env.py:314-321: at most act_maxdiff from the present joints), clipping to the
    joint range (robot.py:192), the gripper coupling 0 <= a[8] <= 2 a[7] (robot.py:193) -> the 11 motor targets."""
    m = model()
    a = np.array(action, dtype=np.float64)
    cur = np.concatenate([q[:7], [q[7], -q[8]]])
    if rate_limit:
        a = cur + np.clip(a - cur, -m['act_maxdiff'], m['act_maxdiff'])
    a = np.minimum(np.maximum(a, m['act_min']), m['act_max'])
    a[8] = max(min(a[8], 2 * a[7]), 0.0)
    return np.concatenate([a[:7], [a[7], -a[8], a[7], -a[8]]])


def pair_material(ma, mb):
    """Bullet's combiners (btManifoldResult): friction and restitution are products; rolling and spinning r_a mu_b + r_b mu_a,
    clamped to 10.  ma, mb: {friction, restitution, rolling, spinning}."""
    return np.array([ma[0] * mb[0], ma[1] * mb[1], min(ma[2] * mb[0] + mb[2] * ma[0], ROLL_SPIN_MAX),
                     min(ma[3] * mb[0] + mb[3] * ma[0], ROLL_SPIN_MAX)])


def _static_shape(x, robot):
    """The static shape a contact point belongs to (the records say only `static`): the one whose facet planes the point is
    least outside of.  A robot link meets the table and the shelf only (shapes 0, 1)."""
    m = model()
    cands = [s for s in range(len(m['shape_owner'])) if m['shape_owner'][s][0] == 0][:2 if robot else None]
    out = [np.max(m['shape_planes'][s][:m['shape_nf'][s], :3] @ x - m['shape_planes'][s][:m['shape_nf'][s], 3]) for s in cands]
    return cands[int(np.argmin(out))]


def contact_material(rec, dyn):
    """{mu, restitution, rolling, spinning} of a contact record's shape pair: an object's row of `dyn`, the model's materials for
    the robot's links and the statics."""
    m = model()
    own = m['shape_owner']

    def mat(body, link, x, robot_other):
        if body >= 16:
            return dyn[body - 16][4:8]
        if body >= 0:
            s = [s for s in range(len(own)) if own[s][0] == 1 and own[s][2] == link][0]
        else:
            s = _static_shape(x, robot_other)
        return np.concatenate([m['shape_mat'][s], m['shape_roll'][s]])
    bA, bB, lA = int(rec[0]), int(rec[1]), int(rec[2])
    x = np.asarray(rec[3:6], dtype=np.float64)
    return pair_material(mat(bA, lA, x, False), mat(bB, -1, x, 0 <= bA < 16))


def warm_start(contacts, prev, factor):
    """Bullet's persistent manifold restated on contact lists: a new contact inherits factor x the normal impulse of the previous
    step's contact of the same (bodyA, bodyB, linkA) nearest to it within WARM_DIST, if it is itself the nearest new contact of
    those bodies to that one (mutual nearest neighbours; ties to the lower index)."""
    n = len(contacts)
    lam0 = np.zeros(n)
    if prev is None or not len(prev) or not factor > 0:
        return lam0
    key = lambda r: (int(r[0]), int(r[1]), int(r[2]))
    d2 = lambda a, b: float(np.sum((np.asarray(a[3:6], np.float64) - np.asarray(b[3:6], np.float64)) ** 2))
    for i, c in enumerate(contacts):
        cand = [(d2(c, pc), j) for j, pc in enumerate(prev) if key(pc) == key(c)]
        cand = [t for t in cand if t[0] < WARM_DIST ** 2]
        if not cand:
            continue
        dj, j = min(cand)
        mine = [(d2(ck, prev[j]), k) for k, ck in enumerate(contacts) if key(ck) == key(c)]
        if min(mine)[1] == i:
            lam0[i] = factor * float(prev[j][10]) * DT
    return lam0


SKINS = ('skin_00', 'skin_01', 'skin_10', 'skin_11')      # Kuka.get_touch_sensors' order (robot.py:156)
CONTACT_THRESHOLD = 0.1                                    # Kuka.contact_threshold (robot.py:66, 136)


def touch_sensors(contacts, forces, order=SKINS, threshold=CONTACT_THRESHOLD, statics=True):
    """get_touch_sensors (robot.py:131-163) from contact records [n, 12] and their normal forces [n]: sensor k is the largest
    force of the contacts whose body A is the robot, whose link A is skin `order[k]` and whose |distance| is below `threshold`
    (None: no threshold); 0 if there is none.  The reference's object_names holds the table: static contacts count
    (statics=False leaves them out, a negative control)."""
    from real_robots_amd._native import LINK_NAMES
    c = np.asarray(contacts, dtype=np.float64).reshape(-1, 12)
    f = np.asarray(forces, dtype=np.float64).reshape(-1)
    ok = (c[:, 0] >= 0) & (c[:, 0] < 16)
    if threshold is not None:
        ok &= np.abs(c[:, 9]) < threshold
    if not statics:
        ok &= c[:, 1] >= 0
    out = np.zeros(len(order))
    for k, name in enumerate(order):
        sel = ok & (c[:, 2] == LINK_NAMES.index(name))
        if sel.any():
            out[k] = f[sel].max()
    return out


def plane_space(n):
    """btPlaneSpace1: the two tangents of a unit normal."""
    if abs(n[2]) > 0.7071067811865475244:
        a = n[1] * n[1] + n[2] * n[2]
        k = 1 / np.sqrt(a)
        p = np.array([0.0, -n[2] * k, n[1] * k])
        return p, np.array([a * k, -n[0] * p[2], n[0] * p[1]])
    a = n[0] * n[0] + n[1] * n[1]
    k = 1 / np.sqrt(a)
    p = np.array([-n[1] * k, n[0] * k, 0.0])
    return p, np.array([-n[2] * p[1], n[2] * p[0], a * k])


def _link_jacobians(q, R, p):
    """For every body b: a function x -> (Jv [3, 11], Jw [3, 11]) of a point x fixed in body b's frame, by complex step."""
    Rc, pc, _ = forward(_cs_points(q))                       # [k, body, ...]

    def jac(b, x):
        xl = R[b].T @ (x - p[b])
        Jv = ((Rc[:, b] @ xl) + pc[:, b]).imag.T / CS_H
        S = (Rc[:, b].imag / CS_H) @ R[b].T                    # dR/dq_k R^T = [w_k]x
        Jw = np.stack([S[:, 2, 1], S[:, 0, 2], S[:, 1, 0]])
        return Jv, Jw
    return jac


def step(state, action, contacts, dyn=None, prev=None, solver=None, solver_iters=50, nobj=3, home=None, drop=()):
    """One step from `state` (61) under `action` (9) with the step's contact records `contacts` [n, 12] (x, n, dist are used) and
    the previous step's records `prev` (warm start; None: cold).  dyn: per-object rows [nobj, 8] (None: the model's).  drop: the
    negative controls -- 'coriolis' (the velocity terms of the joint-space bias), 'gyroscopic', 'torsional' (the torsional
    friction rows), 'reverse_normals' (the normal rows swept in reverse order).  Returns dict(state (61), lambda_n [n],
    rows [(kind, contact or joint, ...)], lam (every row's impulse), mat [n, 4] (the combined materials), prep)."""
    P = dict(SOLVER_DEFAULTS, **(solver or {}))
    m = model()
    dyn = default_dynamics(nobj) if dyn is None else np.asarray(dyn, dtype=np.float64)
    s = np.array(state, dtype=np.float64)
    contacts = np.asarray(contacts, dtype=np.float64).reshape(-1, 12)
    q, qd = s[:NB].copy(), s[NB:2 * NB]
    pr = prep(s, dyn, P, nobj, coriolis='coriolis' not in drop, gyroscopic='gyroscopic' not in drop, home=home)
    tgt = motor_targets(q, action, P['rate_limit'])
    R, p, Minv, qds = pr['R'], pr['p'], pr['Minv'], pr['qds']
    nd = NB + 6 * nobj
    W = np.zeros((nd, nd))
    W[:NB, :NB] = Minv
    ustar = np.concatenate([qds] + [np.concatenate([pr['ovs'][i], pr['ows'][i]]) for i in range(nobj)])
    for i in range(nobj):
        o = NB + 6 * i
        W[o:o + 3, o:o + 3] = np.eye(3) / dyn[i][0]
        W[o + 3:o + 6, o + 3:o + 6] = pr['oIinv'][i]
    jac = _link_jacobians(q, R, p)
    rows = []                      # (kind, ref, J, rhs, lo, hi, normal row index or -1, coefficient)

    def add(kind, ref, J, rhs_of, lo, hi, nrow=-1, coef=0.0):
        WJ = W @ J
        diag = J @ WJ
        dinv = 1.0 / diag if diag > 0 else 0.0
        rows.append([kind, ref, J, rhs_of(J @ ustar) * dinv, lo, hi, nrow, coef, WJ, dinv])

    hi_m = P['motor_max_force'] * DT
    for j in range(NB):
        vt = P['motor_kp'] * (tgt[j] - q[j]) / DT + qds[j] + P['motor_kd'] * (0 - qds[j])
        add('motor', (j,), np.eye(nd)[j], lambda rel, vt=vt: vt - rel, -hi_m, hi_m)
    for j in range(NB):
        lo_, hi_ = m['body_limits'][j]
        if not lo_ < hi_:
            continue
        for side, (dist, sg) in enumerate(((q[j] - lo_, 1.0), (hi_ - q[j], -1.0))):
            if dist >= LIMIT_WINDOW:
                continue

            def rhs_lim(rel, dist=dist):
                return (-rel - dist / DT) if dist > 0 else (-dist * P['erp'] / DT - rel)
            add('limit', (j, side), sg * np.eye(nd)[j], rhs_lim, 0.0, LIMIT_MAX_IMPULSE)

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

    mats = np.array([contact_material(c, dyn) for c in contacts]).reshape(-1, 4)
    normal_rows = []
    for ci, c in enumerate(contacts):
        dist, rest = c[9], mats[ci][1]

        def rhs_n(rel, dist=dist, rest=rest):
            r = max(rest * -rel, 0.0) if abs(rel) >= REST_THRESHOLD else 0.0
            return (r - rel - dist / DT) if dist > 0 else (-dist * P['erp'] / DT + r - rel)
        normal_rows.append(len(rows))
        add('normal', (ci,), contact_J(c, c[6:9], False), rhs_n, 0.0, NORMAL_MAX_IMPULSE)
    for ci, c in enumerate(contacts):
        for k, t in enumerate(plane_space(c[6:9])):
            add('friction', (ci, k), contact_J(c, t, False), lambda rel: -rel, 0.0, 0.0, normal_rows[ci], mats[ci][0])
    if 'torsional' not in drop:
        for ci, c in enumerate(contacts):
            t1, t2 = plane_space(c[6:9])
            for k, (axis, coef) in enumerate(((c[6:9], mats[ci][3]), (t1, mats[ci][2]), (t2, mats[ci][2]))):
                if coef > 0:
                    add('torsional', (ci, k), contact_J(c, axis, True), lambda rel: -rel, 0.0, 0.0, normal_rows[ci], coef)
    order = list(range(len(rows)))
    if 'reverse_normals' in drop and normal_rows:
        a, b = normal_rows[0], normal_rows[-1] + 1
        order = order[:a] + order[a:b][::-1] + order[b:]
    lam = np.zeros(len(rows))
    du = np.zeros(nd)
    lam0 = warm_start(contacts, prev, P['warmstart'])
    for ci, r in enumerate(normal_rows):
        if lam0[ci] > 0:
            lam[r] = lam0[ci]
            du += rows[r][8] * lam0[ci]
    for _ in range(int(solver_iters)):
        for k in order:
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
                lam=lam, mat=mats, prep=pr)
