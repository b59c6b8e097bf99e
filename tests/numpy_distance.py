"""A float64 reference of the whole-batch closest-point queries (rr_closest_points, include/realrobot.h), for the tests (a helper
module: pytest does not collect it).

Built from the compiled model's data (real_robots_amd.model.load_model), numpy_step's forward kinematics and
numpy_collide.shape_frames(repose=False) and the header's semantics only; it calls no kernel and it is NOT a GJK.  It takes the road
of `signed_distance` in tests/test_narrowphase_exact.py, restated here: the distance of two convex polytopes is the distance of the
origin from their Minkowski difference, whose hull scipy's qhull builds from the world vertex sets (every difference a - b of two
vertices; each set is first reduced to its extreme points, by qhull too, which leaves its hull as it is); the nearest point of
that hull comes from the facets that face the origin (Voronoi-region tests per triangle), the penetration depth from the nearest
facet plane when none does.

Per item (env, pair): the signed distance d (> 0 Euclidean distance, < 0 penetration depth), the unique closest vector
v* = a* - b* (the point of the Minkowski difference nearest the origin; zero where d <= 0), the gap of the two bounding spheres,
and DECIDED: |d| >= 1 mm (then the status must be 0 for d > 0, 1 for d < 0) and, with a cull, |sphere gap - max_distance| >= 0.1 mm.

Negative controls (VARIANTS): deliberately wrong restatements that must disagree with the device on decided items."""
import numpy as np

from real_robots_amd.model import load_model
from tests import numpy_collide as ncol
from tests import numpy_step as ns

DECIDE = 1e-3                 # m: an item nearer than this to touching is undecided
DECIDE_CULL = 1e-4            # m: ... and with a cull one whose sphere gap is nearer than this to max_distance
VARIANTS = ('normal_flipped', 'object_rotation_identity', 'robot_shape_in_parent_frame', 'first_64_vertices_only')
# float32 rounding of world points: a and b are sums of <= 3 products of weights in [0, 1] and coordinates below 2 m (an ulp of
# 1.2e-7): 8 ulps in each of a and b, 16 * 2^-23 m in a - b
R32 = 16 * 2.0 ** -23
# the bounding spheres' gap in float32: the project's frame tolerance of 2e-6 on R and p over a lever of at most 1.5 m is 5e-6 m per
# shape (tests/test_gpu_rays.py), two shapes
GAP_TOL = 1e-5
VCLASS = {8: '8', 24: '24', 43: '43/46', 46: '43/46', 68: '68/80/88', 80: '68/80/88', 88: '68/80/88', 192: '192', 117: 'coplanar', 124: 'coplanar', 141: 'coplanar'}
CLASSES = ('8', '24', '43/46', '68/80/88', '192', 'coplanar')

_extreme = {}


def names():
    """name -> shape index (BatchedREALRobotEnv.collision_shapes)."""
    from real_robots_amd.batched import BatchedREALRobotEnv
    return {r['name']: r['index'] for r in BatchedREALRobotEnv.collision_shapes()}


def vertex_class(s):
    return VCLASS[len(ncol.shapes()[s]['V'])]


def local_vertices(s, variant=None):
    """The extreme points of shape s's vertex set in its own frame (qhull; the hull of the set is the hull of these)."""
    from scipy.spatial import ConvexHull
    key = (s, variant == 'first_64_vertices_only')
    if key not in _extreme:
        V = ncol.shapes()[s]['V']
        if key[1]:
            V = V[:64]
        _extreme[key] = V[np.sort(ConvexHull(V).vertices)]
    return _extreme[key]


def frames(state, variant=None):
    """World (R [N, ns, 3, 3], p [N, ns, 3]) of every shape's frame: the header's rule (no out-of-bounds re-pose), or a variant's."""
    st = np.asarray(state, dtype=np.float64)
    R, p = ncol.shape_frames(st, repose=False)
    S = ncol.shapes()
    if variant == 'object_rotation_identity':
        for s, sh in enumerate(S):
            if sh['kind'] == 2:
                R[:, s] = np.eye(3)
    if variant == 'robot_shape_in_parent_frame':
        m = ns.model()
        Rb, pb, _ = ns.forward(st[:, :ns.NB])
        for s, sh in enumerate(S):
            if sh['kind'] == 1:
                par = m['parent'][sh['idx']]
                R[:, s], p[:, s] = (np.eye(3), m['robot_pos']) if par < 0 else (Rb[:, par], pb[:, par])
    return R, p


def tri_closest_to_origin(T):
    """closest points to the origin on the triangles T [n, 3, 3] (Voronoi-region tests, vectorised) -> [n, 3]"""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    ab, ac = b - a, c - a
    d1, d2 = -(ab * a).sum(1), -(ac * a).sum(1)
    d3, d4 = -(ab * b).sum(1), -(ac * b).sum(1)
    d5, d6 = -(ab * c).sum(1), -(ac * c).sum(1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    out = np.empty_like(a)
    done = np.zeros(len(a), bool)

    def put(m, p):
        m = m & ~done
        out[m] = p[m]
        done[m] = True
    with np.errstate(divide='ignore', invalid='ignore'):
        put((d1 <= 0) & (d2 <= 0), a)
        put((d3 >= 0) & (d4 <= d3), b)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        put((d6 >= 0) & (d5 <= d6), c)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = 1.0 / (va + vb + vc)
        put(np.ones(len(a), bool), a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None])
    return out


def signed_distance(A, B):
    """(d, v*) of two convex polytopes given by world vertices A [na, 3], B [nb, 3]: d > 0 the Euclidean distance and v* the point
    of the Minkowski difference A - B nearest the origin (= a* - b*, unique); d <= 0: minus the penetration depth and v* = 0."""
    from scipy.spatial import ConvexHull
    D = (A[:, None, :] - B[None, :, :]).reshape(-1, 3)
    h = ConvexHull(D)
    d0 = h.equations[:, 3]
    if (d0 <= 0).all():
        return float(d0.max()), np.zeros(3)
    P = tri_closest_to_origin(D[h.simplices[d0 > 0]])       # (only facets that face the origin can hold the nearest point)
    r = np.linalg.norm(P, axis=1)
    k = int(np.argmin(r))
    return float(r[k]), P[k]


def hull_planes(W):
    """(N [nf, 3], D [nf]) of the hull of the world points W: inside is N x - D <= 0."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(W).equations
    return eq[:, :3], -eq[:, 3]


def reference(state, pairs, max_distance=None, variant=None):
    """state [N, 61], pairs [Q, 2] shape indices -> dict of [N, Q] arrays: d (signed), v [N, Q, 3], gap (bounding spheres), culled,
    decided, expect (the status a decided item must have); plus `world`: {(env, shape): world extreme points}."""
    st = np.asarray(state, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    N, Q = len(st), len(pairs)
    R, p = frames(st, variant)
    sph = np.array(load_model()['shape_sphere'], dtype=np.float64)
    out = dict(d=np.zeros((N, Q)), v=np.zeros((N, Q, 3)), gap=np.zeros((N, Q)), world={})
    world = out['world']
    for e in range(N):
        for s in set(pairs.ravel().tolist()):
            world[e, s] = local_vertices(s, variant) @ R[e, s].T + p[e, s]
        for j, (a, b) in enumerate(pairs.tolist()):
            d, v = signed_distance(world[e, a], world[e, b])
            if variant == 'normal_flipped':
                v = -v
            ca, cb = R[e, a] @ sph[a, :3] + p[e, a], R[e, b] @ sph[b, :3] + p[e, b]
            out['d'][e, j], out['v'][e, j], out['gap'][e, j] = d, v, np.linalg.norm(ca - cb) - sph[a, 3] - sph[b, 3]
    cull = max_distance is not None and 0 < max_distance < np.inf
    out['culled'] = (out['gap'] > max_distance) if cull else np.zeros((N, Q), bool)
    out['decided'] = np.abs(out['d']) >= DECIDE
    if cull:
        out['decided'] = np.where(np.abs(out['gap'] - max_distance) >= DECIDE_CULL, out['decided'] | out['culled'], False)
    out['expect'] = np.where(out['culled'], 2, np.where(out['d'] > 0, 0, 1))
    return out


def compare(cols, ref, tol, pairs):
    """The device's columns (host arrays of closest_points) against a reference on its decided items.  Returns (figures, failures):
    every figure is measured before anything is judged."""
    f64 = lambda k: np.asarray(cols[k], dtype=np.float64)
    dist, lower, a, b, n, status = f64('distance'), f64('lower'), f64('point_a'), f64('point_b'), f64('normal'), np.asarray(cols['status'])
    dec = ref['decided']
    sep, pen, cul = dec & (ref['expect'] == 0), dec & (ref['expect'] == 1), dec & (ref['expect'] == 2)
    ab = a - b
    fig, fails = dict(items=int(dec.size), decided=int(dec.sum()), separated=int(sep.sum()), overlapping=int(pen.sum()), culled=int(cul.sum())), []

    def need(name, value, bound):
        fig[name] = float(value)
        if not value <= bound:
            fails.append('%s %.3g > %.3g' % (name, value, bound))
    mx = lambda x, m: float(np.abs(x[m]).max()) if m.any() else 0.0
    need('status_mismatches', int((status[dec] != ref['expect'][dec]).sum()), 0)
    need('status3_on_decided', int((status[dec] == 3).sum()), 0)
    need('distance_error', mx(dist - ref['d'], sep), tol)
    need('lower_above_exact', float((lower - ref['d'])[sep].max()) if sep.any() else 0.0, tol)
    need('lower_above_distance', float((lower - dist)[sep].max()) if sep.any() else 0.0, 0.0)
    need('norm_ab_vs_distance', mx(np.linalg.norm(ab, axis=-1) - dist, sep), R32)
    need('normal_vs_ab', float(np.linalg.norm(n * dist[..., None] - ab, axis=-1)[sep].max()) if sep.any() else 0.0, R32)
    need('normal_unit', mx(np.linalg.norm(n, axis=-1) - 1.0, sep), 4 * 2.0 ** -23)
    # the projection inequality for the min-norm point v* of a convex set: |x - v*|^2 <= |x|^2 - |v*|^2 for every x of the set
    slack = np.sqrt(np.maximum(0.0, dist ** 2 - ref['d'] ** 2)) + 2 * tol
    need('vector_excess', float((np.linalg.norm(ab - ref['v'], axis=-1) - slack)[sep].max()) if sep.any() else -1.0, 0.0)
    worst = 0.0
    for e, j in zip(*np.nonzero(sep)):
        for x, s in ((a[e, j], pairs[j][0]), (b[e, j], pairs[j][1])):
            Nn, Dd = hull_planes(ref['world'][e, s])
            worst = max(worst, float((Nn @ x - Dd).max()))
    need('point_outside_hull', worst, tol)
    if pen.any():
        ok = (dist[pen] == 0).all() and (lower[pen] == 0).all() and not np.asarray(cols['normal'])[pen].view(np.uint32).any() \
            and (a[pen] == b[pen]).all() and np.isfinite(a[pen]).all()
        need('overlap_rows_malformed', 0 if ok else 1, 0)
    if cul.any():
        need('cull_gap_error', mx(dist - ref['gap'], cul), GAP_TOL)
        need('cull_lower_is_distance', int((np.asarray(cols['lower'])[cul] != np.asarray(cols['distance'])[cul]).sum()), 0)
    return fig, fails


# ---------------------------------------------------------------------------------------------- the tests' inputs (fixed seeds)
SEED = 31


def seven_pairs():
    """Seven pairs in which every vertex-count class occurs: 8 (pads), 24, 43 / 46, 88, 192 (the cap), 117 / 124 / 141 (coplanar)."""
    n = names()
    return np.array([(n['skin_00'], n['cube']), (n['tomato'], n['table']), (n['finger_01'], n['mustard']), (n['finger_00'], n['shelf']),
                     (n['lbr_iiwa_link_7'], n['robot_base']), (n['lbr_iiwa_link_3'], n['lbr_iiwa_link_6']), (n['cube'], n['tomato'])], np.int32)


def collision_pairs(nobj=3):
    return np.array([(a, b) for _, a, b in ncol.pair_table(nobj)], np.int32)


def states(N, seed):
    """[N, 61] float32: random postures and object poses (numpy_rays.states), and in the first envs the arranged cases: env 0 the
    cube 5 mm above the table top with parallel faces, the tomato 3 cm into the cube (overlapping objects) and the mustard between
    the fingers; env 1 the cube between the fingers; env 2 the tomato overlapping the cube."""
    from tests import numpy_rays as nr
    st = nr.states(N, 3, seed).astype(np.float64)
    S, n = ncol.shapes(), names()
    table, cube = S[n['table']], S[n['cube']]
    assert np.array_equal(table['N'][2], [0, 0, 1])
    top = float(table['D'][2])

    def obj(e, o, pos, quat=None):
        c = 22 + 13 * o
        st[e, c:c + 3] = pos
        if quat is not None:
            st[e, c + 3:c + 7] = quat

    def between_fingers(e):
        q = st[e, :11]
        return 0.5 * (ns.link_pose(q, n_link('skin_00'))[1] + ns.link_pose(q, n_link('skin_10'))[1])

    def n_link(name):
        from real_robots_amd import _native as nat
        return nat.LINK_NAMES.index(name)
    cube_on = np.array([-0.1, 0.1, top + 0.005 - cube['V'][:, 2].min()])
    if N >= 1:
        obj(0, 0, cube_on, [0, 0, 0, 1])
        obj(0, 1, cube_on + [0.03, 0.0, 0.02])
        obj(0, 2, between_fingers(0))
    if N >= 3:
        obj(1, 0, between_fingers(1))
        obj(2, 1, st[2, 22:25] + [0.0, 0.03, 0.0])
    return st.astype(np.float32)


# (envs, pairs) of the parity tests: N in {1, 5, 67} -- no multiple of any workgroup's env count -- and Q in {92 ('collision'), 7, 1}
def cases():
    return ((1, 'collision', collision_pairs(3)), (5, 'seven', seven_pairs()), (67, 'one', np.array([(names()['cube'], names()['table'])], np.int32)))


_cases = {}


def case(N, variant=None, max_distance=None):
    """(state, pairs, reference) of the parity case with N envs, computed once per process and left unchanged."""
    key = (N, variant, max_distance)
    if key not in _cases:
        pairs = [p for n, _, p in cases() if n == N][0]
        st = states(N, SEED + N)
        _cases[key] = (st, pairs, reference(st, pairs, max_distance=max_distance, variant=variant))
    return _cases[key]


def control_error(ref, var):
    """The largest disagreement (m) of a variant with the reference over the reference's decided, separated items: in the distance
    or in the closest vector."""
    m = ref['decided'] & (ref['d'] > 0)
    dd = np.abs(np.maximum(var['d'], 0.0) - ref['d'])
    dv = np.linalg.norm(var['v'] - ref['v'], axis=-1)
    return float(np.maximum(dd, dv)[m].max()) if m.any() else 0.0
