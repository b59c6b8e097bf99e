"""A float64 reference of the penetration depth of the signed-distance queries (rr_signed_distance, include/realrobot.h), for the
tests (a helper module: pytest does not collect it).

It extends the qhull road of tests/numpy_distance.py: two convex hulls overlap when their Minkowski difference A - B holds the origin,
the penetration depth is the distance of the origin from the nearest facet plane of that difference, and the shortest separating
translation of A runs against that facet's outward normal.  Per item it gives the exact depth, the direction n* (from b towards a, the
header's convention: moving A by depth * n* separates the hulls) and, for ANY direction n, the separating width
g(n) = max_b n . b - min_a n . a: the translation of A along n that just separates the hulls.  A device direction is not compared with
n* -- another facet more than 5 degrees away is often within 0.1 mm of the nearest one -- but by g(n_dev) <= exact + tolerance.

It also holds (expansion) a plain float64 expanding-polytope search that shares nothing with the kernel -- the qhull of the support
points gathered so far, the nearest facet, the support along its normal -- for one purpose: to show that the seeded inputs stay far
below the kernel's caps; and (face_normals_only) the tempting cheaper algorithm as a negative control: the smallest g over the face
normals of the two hulls alone, which misses the edge-edge facets of the Minkowski difference."""
import numpy as np

from tests import numpy_distance as nd
from tests import numpy_posture as npo

CONTROLS = ('object_rotation_identity', 'robot_shape_in_parent_frame', 'first_64_vertices_only', 'face_normals_only')
CASES = ('1', '5', 'R')
TRIP_CAP, FACE_CAP = 32, 64             # the kernel's caps (SD_TRIP_CAP, one face per lane)


def width(A, B, n):
    """g(n): the translation of A along n that just separates the hulls of the world vertices A and B (<= 0: already apart along n)."""
    n = np.asarray(n, dtype=np.float64)
    return float((B @ n).max() - (A @ n).min())


def nearest_facet(A, B):
    """(depth, n*) of two OVERLAPPING convex polytopes: the distance of the origin from the nearest facet plane of A - B, and minus
    that facet's outward normal (moving A by depth * n* separates the hulls)."""
    from scipy.spatial import ConvexHull
    h = ConvexHull((A[:, None, :] - B[None, :, :]).reshape(-1, 3))
    k = int(np.argmax(h.equations[:, 3]))
    assert h.equations[k, 3] <= 0, 'the hulls do not overlap'
    return float(-h.equations[k, 3]), -h.equations[k, :3]


def face_normals_only(A, B):
    """The depth a search over the face normals of the two hulls alone would report (no edge-edge facets): an upper bound of the depth."""
    Na, Nb = nd.hull_planes(A)[0], nd.hull_planes(B)[0]
    return min(width(A, B, n) for n in np.concatenate([Na, -Na, Nb, -Nb]))


def support(A, B, d):
    """The support point of A - B along d and its vertex pair (first maxima)."""
    i, j = int(np.argmax(A @ d)), int(np.argmin(B @ d))
    return A[i] - B[j], (i, j)


def expansion(A, B, eps=1e-9):
    """A float64 expanding-polytope search from the axis octahedron -> (depth, n, trips, faces): per trip the qhull of the support
    points so far, its facet nearest the origin and the support of A - B along that facet's normal; it ends when the support gains
    less than eps or is a point it already has.  faces is the largest number of triangles any trip's polytope had."""
    from scipy.spatial import ConvexHull
    pts, seen = [], set()
    for d in np.concatenate([np.eye(3), -np.eye(3)]):
        w, ij = support(A, B, d)
        if ij not in seen:
            seen.add(ij)
            pts.append(w)
    trips = faces = 0
    while True:
        trips += 1
        h = ConvexHull(np.array(pts))
        faces = max(faces, len(h.simplices))
        k = int(np.argmax(h.equations[:, 3]))
        n, d = h.equations[k, :3], -h.equations[k, 3]
        w, ij = support(A, B, n)
        if ij in seen or n @ w - d <= eps:
            return float(n @ w), -n, trips, faces
        seen.add(ij)
        pts.append(w)


def case(name, variant=None):
    """(reference, pairs) of a seeded case: '1' and '5' are numpy_distance.case(1), case(5) (the present state), 'R' is
    numpy_posture.case_r (16 rows of 80 pairs).  The reference is numpy_distance.reference's, computed once per process."""
    if name == 'R':
        return npo.case_r(variant=variant), npo.case_r_inputs()[2]
    _, pairs, ref = nd.case(int(name), variant=variant)
    return ref, pairs


def overlapping(ref):
    """The decided overlapping items of a reference: (row, pair) index arrays."""
    return np.nonzero(ref['decided'] & (ref['d'] < 0))


def hulls(ref, pairs, e, j):
    return ref['world'][int(e), int(pairs[j][0])], ref['world'][int(e), int(pairs[j][1])]


_fno = {}


def control_depths(name, control):
    """The depths [items] a control gives on the decided overlapping items of case `name` (0 where the control sees no overlap)."""
    ref, pairs = case(name)
    rows, cols = overlapping(ref)
    if control == 'face_normals_only':
        if name not in _fno:
            _fno[name] = np.array([face_normals_only(*hulls(ref, pairs, e, j)) for e, j in zip(rows, cols)])
        return _fno[name]
    var, _ = case(name, variant=control)
    return np.maximum(-var['d'][rows, cols], 0.0)


def control_error(name, control):
    """The largest |control's depth - exact depth| (m) over the decided overlapping items of case `name`."""
    ref, _ = case(name)
    rows, cols = overlapping(ref)
    return float(np.abs(control_depths(name, control) + ref['d'][rows, cols]).max()) if len(rows) else 0.0


def inside(ref, pairs, e, j, a, b):
    """How far (m) the points a, b lie outside the hulls of item (e, j): the largest plane excess, <= 0 inside."""
    worst = -np.inf
    for x, W in zip((a, b), hulls(ref, pairs, e, j)):
        Nn, Dd = nd.hull_planes(W)
        worst = max(worst, float((Nn @ np.asarray(x, dtype=np.float64) - Dd).max()))
    return worst


def compare(cols, ref, pairs, tol):
    """The device's per-item columns (host arrays [R, Q] of signed_distance: distance, bound, point_a, point_b, normal, status,
    expansions) against the reference on its decided OVERLAPPING items.  Returns (figures, failures); every figure is measured
    before anything is judged."""
    f64 = lambda k: np.asarray(cols[k], dtype=np.float64)
    sd, bound, a, b, n, status = f64('distance'), f64('bound'), f64('point_a'), f64('point_b'), f64('normal'), np.asarray(cols['status'])
    rows, cc = overlapping(ref)
    fig, fails = dict(overlapping=len(rows)), []
    if not len(rows):
        return fig, fails
    exact = -ref['d'][rows, cc]
    g = np.array([width(*hulls(ref, pairs, e, j), n[e, j]) for e, j in zip(rows, cc)])
    out = np.array([inside(ref, pairs, e, j, a[e, j], b[e, j]) for e, j in zip(rows, cc)])
    s, bo, nn, ab = sd[rows, cc], bound[rows, cc], n[rows, cc], (a - b)[rows, cc]

    def need(name, value, limit):
        fig[name] = float(value)
        if not value <= limit:
            fails.append('%s %.3g > %.3g' % (name, value, limit))
    need('status_not_1', int((status[rows, cc] != 1).sum()), 0)
    need('status_5', int((status[rows, cc] == 5).sum()), 0)
    need('depth_error', np.abs(-s - exact).max(), tol)
    need('bound_above_exact', (-bo - exact).max(), tol)
    need('width_above_exact', (g - exact).max(), tol)
    need('width_vs_signed', np.abs(g + s).max(), tol)
    need('normal_unit', np.abs(np.linalg.norm(nn, axis=-1) - 1.0).max(), 4 * 2.0 ** -23)
    need('ab_vs_signed_normal', np.linalg.norm(ab - s[:, None] * nn, axis=-1).max(), nd.R32)
    need('point_outside_hull', out.max(), tol)
    if 'expansions' in cols:
        fig['max_expansions'] = int(np.asarray(cols['expansions'])[rows, cc].max())
    return fig, fails
