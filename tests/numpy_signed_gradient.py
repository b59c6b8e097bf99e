"""A float64 reference of the joint gradients of the signed distance (rr_signed_gradient, include/realrobot.h), for the tests (a helper
module: pytest does not collect it).

The reference takes another road than the device: CENTRAL FINITE DIFFERENCES of tests/numpy_distance.reference -- qhull on the
Minkowski difference, no GJK, no Jacobian -- over the eleven joints, with the forward and backward differences kept so that an item
whose distance has a kink inside +-H can be told from a smooth one by the reference alone.  tests/golden/make_signed_gradient.py writes
them to tests/golden/signed_gradient.npz (30 s of qhull per 7000 evaluations is too much for a test).

Beside it stands the header's formula restated in float64,
    ds/dq_k = [joint k moves A's body] n . (a_k x (a - p_k)) - [joint k moves B's body] n . (a_k x (b - p_k)),
on witness points found from the SUPPORTING VERTEX SETS of the reference's normal (no GJK either), and four deliberately wrong
evaluations of it (CONTROLS)."""
import os

import numpy as np

from tests import numpy_collide as ncol
from tests import numpy_distance as nd
from tests import numpy_step as ns

H = 1e-3                      # rad: the step of the differences (the reference's d carries about 3e-8 m of noise: 1e-4 is noise-bound)
# m/rad: an item is SMOOTH when max_k |forward - backward| is below this.  |forward - backward| = H |s''| for a smooth s, and s'' is a
# lever (at most about 1 m) times a curvature of order one: 1e-3 at H = 1e-3; a switch of witness features inside +-H jumps the
# first derivative by a lever times an angle, an order or more above that.  Fixed from the reference alone.
SMOOTH = 1e-3
NEAR_MARGIN = 1e-3            # m: a row takes part in the cost differences when no pair's distance is this near the margin
MARGIN = 0.05                 # m: the hinge margin of the cost checks
SUPPORT_EPS = 1e-7            # m: a vertex this near the supporting plane belongs to the supporting set
CONTROLS = ('ancestors_ignored', 'normal_flipped', 'jacobian_at_present_joints', 'neighbour_posture')
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'signed_gradient.npz')


def bodies(pairs):
    """[Q, 2] moving body of each shape of the pairs, -1 for a static shape or an object (no columns)."""
    S = ncol.shapes()
    return np.array([[S[s]['idx'] if S[s]['kind'] == 1 else -1 for s in p] for p in np.asarray(pairs).reshape(-1, 2).tolist()], np.int64)


def masks(pairs, anc=None):
    """(mA, mB) [Q, 11]: joint k moves the body of shape A / B of pair j."""
    anc = ns.model()['anc'] if anc is None else anc
    b = bodies(pairs)
    m = np.concatenate([anc, np.zeros((1, ns.NB))])         # (row -1: no columns)
    return m[b[:, 0]], m[b[:, 1]]


def differences(rows, pairs, h=H, items=None):
    """rows [R, 61], pairs [Q, 2] -> (d0 [R, Q], dplus [R, Q, 11], dminus [R, Q, 11]): the reference's signed distance at the rows and
    with joint k moved by +-h.  items: an optional list of (row, pair) to restrict the work to (everything else stays NaN)."""
    st = np.asarray(rows, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    R, Q = len(st), len(pairs)
    if items is not None:
        d0, dp, dm = np.full((R, Q), np.nan), np.full((R, Q, ns.NB), np.nan), np.full((R, Q, ns.NB), np.nan)
        for r in sorted(set(i[0] for i in items)):
            js = sorted(set(i[1] for i in items if i[0] == r))
            a, b, c = differences(st[r:r + 1], pairs[js], h)
            d0[r, js], dp[r, js], dm[r, js] = a[0], b[0], c[0]
        return d0, dp, dm
    d0 = nd.reference(st, pairs)['d']
    dp, dm = np.zeros((R, Q, ns.NB)), np.zeros((R, Q, ns.NB))
    for k in range(ns.NB):
        for out, sg in ((dp, 1.0), (dm, -1.0)):
            s = st.copy()
            s[:, k] += sg * h
            out[:, :, k] = nd.reference(s, pairs)['d']
    return d0, dp, dm


def derivatives(d0, dp, dm, h=H):
    """(central, forward, backward) [R, Q, 11] from the three sets of distances."""
    return (dp - dm) / (2 * h), (dp - d0[..., None]) / h, (d0[..., None] - dm) / h


def witness(A, B):
    """World extreme points A [na, 3], B [nb, 3] of two convex hulls -> (s, n, a, b, unique): the signed distance, the unit normal
    from b towards a, witness points with a - b = s n, and whether they are the only such pair.  n is the reference's (v / d apart;
    minus the outward normal of the Minkowski difference's nearest facet when overlapping); a is a convex combination of A's
    supporting vertices along -n, b of B's along +n (non-negative least squares on a - b = s n)."""
    from scipy.optimize import nnls
    from scipy.spatial import ConvexHull
    d, v = nd.signed_distance(A, B)
    if d > 0:
        n = v / d
    else:
        eq = ConvexHull((A[:, None, :] - B[None, :, :]).reshape(-1, 3)).equations
        n = -eq[int(np.argmax(eq[:, 3])), :3]
    ha, hb = A @ n, B @ n
    SA, SB = A[ha <= ha.min() + SUPPORT_EPS], B[hb >= hb.max() - SUPPORT_EPS]
    M = np.zeros((5, len(SA) + len(SB)))
    M[:3, :len(SA)], M[:3, len(SA):] = SA.T, -SB.T
    M[3, :len(SA)] = M[4, len(SA):] = 1.0
    w, _ = nnls(M, np.concatenate([d * n, [1.0, 1.0]]))
    la, mu = w[:len(SA)], w[len(SA):]
    a, b = la @ SA / la.sum(), mu @ SB / mu.sum()
    rk = lambda X: int(np.linalg.matrix_rank(X, tol=10 * SUPPORT_EPS)) if len(X) else 0
    da, db = SA[1:] - SA[0], SB[1:] - SB[0]
    unique = rk(np.concatenate([da, db])) == rk(da) + rk(db)      # the two faces' direction spaces meet in 0 only
    return d, n, a, b, unique


def formula(q, a, b, n, mA, mB):
    """The header's expression in float64: q [..., 11] joints, a, b, n [..., 3], mA, mB [..., 11] -> ds/dq [..., 11]."""
    _, p, ax = ns.forward(np.asarray(q, dtype=np.float64))
    a, b, n = (np.asarray(x, dtype=np.float64)[..., None, :] for x in (a, b, n))
    ga = (n * np.cross(ax, a - p)).sum(-1)
    gb = (n * np.cross(ax, b - p)).sum(-1)
    return mA * ga - mB * gb


def witnesses(rows, pairs, items):
    """witness() on the listed (row, pair) items of rows [R, 61] -> dict of s [I], n, a, b [I, 3], unique [I]."""
    st = np.asarray(rows, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    Rs, ps = nd.frames(st)
    W = dict(s=np.zeros(len(items)), n=np.zeros((len(items), 3)), a=np.zeros((len(items), 3)), b=np.zeros((len(items), 3)),
             unique=np.zeros(len(items), bool))
    for i, (r, j) in enumerate(items):
        sa, sb = pairs[j]
        A, B = nd.local_vertices(sa) @ Rs[r, sa].T + ps[r, sa], nd.local_vertices(sb) @ Rs[r, sb].T + ps[r, sb]
        W['s'][i], W['n'][i], W['a'][i], W['b'][i], W['unique'][i] = witness(A, B)
    return W


def formula_items(rows, pairs, items, W, control=None, present=None, neighbour=None):
    """The float64 formula on the witnesses W of the listed (row, pair) items -> g [I, 11].  control: one of CONTROLS; present /
    neighbour [R, 11]: the joints at which the two posture controls evaluate the frames."""
    st = np.asarray(rows, dtype=np.float64)
    mA, mB = masks(pairs, np.eye(ns.NB) if control == 'ancestors_ignored' else None)
    r, j = np.array([i[0] for i in items], np.int64), np.array([i[1] for i in items], np.int64)
    q = st[:, :ns.NB]
    if control == 'jacobian_at_present_joints':
        q = np.asarray(present, dtype=np.float64)
    if control == 'neighbour_posture':
        q = np.asarray(neighbour, dtype=np.float64)
    return formula(q[r], W['a'], W['b'], -W['n'] if control == 'normal_flipped' else W['n'], mA[j], mB[j])


def cost(d, margin=MARGIN):
    """C = 1/2 sum_j max(margin - d_j, 0)^2 over the last axis, in float64."""
    c = np.maximum(margin - np.asarray(d, dtype=np.float64), 0.0)
    return 0.5 * (c * c).sum(-1)


def cost_gradient(d, g, margin=MARGIN):
    """dC/dq = -sum_j c_j grad s_j: d [..., Q], g [..., Q, 11] -> [..., 11], in float64; a NaN distance contributes nothing."""
    d, g = np.asarray(d, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        c = np.where(margin - d > 0, margin - d, 0.0)
    return -(np.where(c[..., None] > 0, c[..., None] * g, 0.0)).sum(-2)


def compared(d0, fwd, bwd):
    """The items the differences may be held to: decided (numpy_distance.DECIDE) and smooth."""
    return (np.abs(d0) >= nd.DECIDE) & (np.abs(fwd - bwd).max(-1) <= SMOOTH)


_fix = None


def fixture():
    """The committed fixture as a dict of arrays, loaded once."""
    global _fix
    if _fix is None:
        with np.load(FIXTURE) as z:
            _fix = {k: z[k] for k in z.files}
    return _fix
