"""A float64 numpy restatement of the narrow phase, for the tests (a helper module: pytest does not collect it).

Built from the compiled model's data (real_robots_amd.model.load_model) and the documented semantics only (the
comments of the collision section of oracle/rr_oracle.c) -- it imports nothing of oracle/ and calls no kernel, and
where it can it takes another road than the C and HIP code:

* shape transforms from numpy_step's forward kinematics and the model's shape_owner table;
* the pair table from the rule (objects x statics, objects x objects, moving robot shapes x {table, shelf}, moving robot shapes x
  objects), the statics that are not the robot's being "table and shelf";
* vertex candidates as dense matrix products, every vertex against every plane: NO pair cull, NO sphere-beyond-one-plane cull, NO
  plane prefilter -- a cull of the device that dropped something would show as a missing contact.  The bounding-sphere test is kept
  as a stated rule (pair(sphere=True)): it is not an exact shortcut, see pair();
* edge-edge candidates over all edge pairs at once, each condition of the rule a signed slack;
* the reduction to at most four points on arrays, with every first-maximum selection keeping its runners-up.

Besides the contact records (layout of the contact lists: bodyA, bodyB, linkA, x (3), n (3), dist, force = 0, mu) every pair
carries the identity of its candidates (kind 0 / 1: vertex of A / of B with its winning plane; kind 2: edge pair) and a DECISION
MARGIN computed from this reference alone: the smallest distance (m; the dimensionless guards of the edge rule count as they are)
of any quantity from the threshold it was compared with -- the 2 cm margin, the tier and tie limits, the edge rule's guards and
s, t in (0, 1), the 128-candidate order is exact -- and the gap between the winner and the runner-up of the best plane of every
candidate vertex, of the anchor and of the three picks.  The gaps of the squared quantities are taken as lengths (|d|, distance
from the line, signed distance on the other side).  A runner-up of the anchor or of a pick counts only if choosing it would change
the SET of points picked: a square face resting flat has its second and third corner exactly equidistant from the diagonal through
the anchor, either order gives the same four points, and that tie is no instability of the manifold.  The margin is conservative: it is a minimum
over every decision of the pair, most of which no rounding comes near, and the float32 build was seen to disagree only where it is
far below one float32 rounding of these lengths, on (almost) exact ties (tests/test_numpy_collide.py gives the measurement).
"""
import numpy as np

from real_robots_amd.model import load_model
from tests import numpy_step as ns

MARGIN = 0.02                 # contact margin: a vertex is a candidate when its largest signed plane distance is below it
CAND_MAX = 128                # candidates kept per pair, in candidate order
MAXC = 48                     # contacts kept per env, in pair order
TIER_TOL = 0.001              # tier 1: candidates within this of the deepest
TIE_TOL = 0.0005              # the anchor is chosen among the candidates within this of the deepest
SKEW = np.array([1.0, 0.618, 0.382])
EDGE_DEPTH = 0.005            # an edge pair deeper than this is no contact
EDGE_SLOP = 0.0005            # ... nor one deeper than the deepest vertex candidate by more than this
PARALLEL = 1e-4               # sin^2 of the angle below which two edges are left to their end points
BIG = 1e30

_S = None


def shapes():
    """Per shape: owner kind (0 static, 1 robot, 2 object), owner index, link, vertices, plane normals and offsets, edges
    {p0, d, facet normal 1, facet normal 2}, friction -- float64."""
    global _S
    if _S is None:
        m = load_model()
        f = lambda a: np.array(a, dtype=np.float64)
        _S = []
        for s, own in enumerate(np.array(m['shape_owner'])):
            nv, nf, ne = int(m['shape_nv'][s]), int(m['shape_nf'][s]), int(m['shape_ne'][s])
            pl = f(m['shape_planes'][s][:nf])
            _S.append(dict(kind=int(own[0]), idx=int(own[1]), link=int(own[2]), robot_base=int(own[0]) == 0 and int(own[2]) >= 0,
                           V=f(m['shape_verts'][s][:nv]), N=pl[:, :3], D=pl[:, 3], E=f(m['shape_edges'][s][:ne]),
                           mu=float(m['shape_mat'][s][0])))
    return _S


def _spheres():
    return np.array(load_model()['shape_sphere'], dtype=np.float64)


def body_id(sh):
    """The contact records' body: -1 static, the body index of a robot shape, 16 + index of an object."""
    return -1 if sh['kind'] == 0 else sh['idx'] if sh['kind'] == 1 else 16 + sh['idx']


def pair_table(nobj=3):
    """[(group, shape A, shape B)] in list order.  A: every object x every static shape; B: object x object; C: every moving robot
    shape x table and shelf (the statics that are not the robot's own base); D: every moving robot shape x every object."""
    S = shapes()
    idx = lambda pred: [s for s, sh in enumerate(S) if pred(sh)]
    statics, robot = idx(lambda sh: sh['kind'] == 0), idx(lambda sh: sh['kind'] == 1)
    objs = sorted(idx(lambda sh: sh['kind'] == 2 and sh['idx'] < nobj), key=lambda s: S[s]['idx'])
    scenery = [s for s in statics if not S[s]['robot_base']]
    out = [('A', o, s) for o in objs for s in statics]
    out += [('B', objs[i], objs[j]) for i in range(len(objs)) for j in range(i + 1, len(objs))]
    out += [('C', r, s) for r in robot for s in scenery]
    out += [('D', r, o) for r in robot for o in objs]
    return out


def shape_frames(state, repose=True):
    """World (R [..., ns, 3, 3], p [..., ns, 3]) of every shape's frame for states [..., 61]: identity for the statics, the body
    frame of numpy_step.forward for a robot shape, the pose of an object -- after the step's out-of-bounds re-pose (repose)."""
    S, m = shapes(), ns.model()
    st = np.asarray(state, dtype=np.float64)
    Rb, pb, _ = ns.forward(st[..., :ns.NB])
    ob = st[..., 2 * ns.NB:].reshape(st.shape[:-1] + (3, 13))
    pos, quat = ob[..., :3], ob[..., 3:7]
    if repose:
        oob = ns.out_of_bounds(pos)[..., None]
        pos, quat = np.where(oob, m['obj_pose0'][:, :3], pos), np.where(oob, m['obj_pose0'][:, 3:7], quat)
    Ro = ns.quat_to_mat(quat)
    R = np.zeros(st.shape[:-1] + (len(S), 3, 3))
    p = np.zeros(st.shape[:-1] + (len(S), 3))
    for s, sh in enumerate(S):
        if sh['kind'] == 0:
            R[..., s, :, :] = np.eye(3)
        elif sh['kind'] == 1:
            R[..., s, :, :], p[..., s, :] = Rb[..., sh['idx'], :, :], pb[..., sh['idx'], :]
        else:
            R[..., s, :, :], p[..., s, :] = Ro[..., sh['idx'], :, :], pos[..., sh['idx'], :]
    return R, p


def _top2(S):
    """Row-wise first maximum of S [n, k]: (index, value, gap to the runner-up)."""
    k = np.argmax(S, axis=1)
    r = np.arange(len(S))
    best = S[r, k]
    if S.shape[1] < 2:
        return k, best, np.full(len(S), BIG)
    T = S.copy()
    T[r, k] = -BIG
    return k, best, best - T.max(axis=1)


def _vertex_pass(A, Ra, pa, B, Rb, pb, sign, kind, ext):
    """Vertices of A against the planes of B.  Returns (candidates [n, 7] {x, n, s}, identities, margin, extended [m, 7]): the
    extended list holds every (vertex, plane) whose plane is within `ext` of the vertex's best and below margin + ext."""
    xw = A['V'] @ Ra.T + pa
    xl = (xw - pb) @ Rb
    S = xl @ B['N'].T - B['D']
    bf, best, gap = _top2(S)
    ok = best < MARGIN
    nw = B['N'][bf] @ Rb.T
    cand = np.concatenate([xw - 0.5 * best[:, None] * nw, sign * nw, best[:, None]], axis=1)[ok]
    ident = [(kind, int(v), int(bf[v])) for v in np.flatnonzero(ok)]
    margin = float(np.abs(best - MARGIN).min())
    if ok.any():
        margin = min(margin, float(gap[ok].min()))
    extended = np.zeros((0, 7))
    if ext > 0:
        v, f = np.nonzero((S > best[:, None] - ext) & (best[:, None] < MARGIN + ext))
        nw = B['N'][f] @ Rb.T
        extended = np.concatenate([xw[v] - 0.5 * S[v, f][:, None] * nw, sign * nw, S[v, f][:, None]], axis=1)
    return cand, ident, margin, extended


def _edge_pass(A, Ra, pa, B, Rb, pb, lo, ext):
    """Edge-edge candidates of every pair of long sharp edges: closest points strictly inside both segments, not (nearly)
    parallel, the common normal inside both facet fans, the distance along it in (-EDGE_DEPTH, MARGIN) and above `lo`.  Every
    condition is a slack that passes when positive; a pair's margin is the magnitude of its smallest slack (accepted: the
    nearest threshold; rejected: how far its worst condition is from passing), and for a pair whose closest points are inside
    both segments also the slack of the choice of the normal's sign."""
    Ea, Eb = A['E'], B['E']
    if not len(Ea) or not len(Eb):
        return np.zeros((0, 7)), [], BIG, np.zeros((0, 7))
    rot = lambda E, R, k: E[:, k:k + 3] @ R.T
    P0, D1, a1, a2 = rot(Ea, Ra, 0) + pa, rot(Ea, Ra, 3), rot(Ea, Ra, 6), rot(Ea, Ra, 9)
    Q0, D2, b1, b2 = rot(Eb, Rb, 0) + pb, rot(Eb, Rb, 3), rot(Eb, Rb, 6), rot(Eb, Rb, 9)
    na, nb = len(Ea), len(Eb)
    bc = lambda X, axis: np.broadcast_to(X[:, None] if axis == 0 else X[None], (na, nb, 3))
    D1, a1, a2, D2, b1, b2 = bc(D1, 0), bc(a1, 0), bc(a2, 0), bc(D2, 1), bc(b1, 1), bc(b2, 1)
    dot = lambda x, y: np.sum(x * y, axis=-1)
    r = P0[:, None] - Q0[None]
    a, e, b, c, f = dot(D1, D1), dot(D2, D2), dot(D1, D2), dot(D1, r), dot(D2, r)
    ae = a * e
    den = ae - b * b
    with np.errstate(divide='ignore', invalid='ignore'):
        s, t = (b * f - c * e) / den, (a * f - b * c) / den
        la, lb = np.sqrt(a), np.sqrt(e)
        geom = np.stack([den / ae - PARALLEL, s * la, (1 - s) * la, t * lb, (1 - t) * lb])
        p, q = P0[:, None] + s[..., None] * D1, Q0[None] + t[..., None] * D2
        nv = np.cross(D1, D2)
        nv = nv / np.linalg.norm(nv, axis=-1, keepdims=True)
        dm = dot(nv, a1 + a2)
        u = np.where(dm[..., None] > 0, nv, -nv)                       # unit, from A towards B
        w = -u
        pq = p - q
        dist = dot(w, pq)
        rest = np.stack([dot(np.cross(a1, u), np.cross(u, a2)) + 1e-300, dot(w, b1 + b2),
                         dot(np.cross(b1, w), np.cross(w, b2)) + 1e-300, MARGIN - dist, dist + EDGE_DEPTH, dist - lo])
    G1 = np.nan_to_num(geom, nan=-BIG, posinf=BIG, neginf=-BIG).min(axis=0)
    G2 = np.nan_to_num(rest, nan=-BIG, posinf=BIG, neginf=-BIG).min(axis=0)
    G = np.minimum(G1, G2)
    ok = G > 0
    m = np.abs(G)
    m = np.where(G1 > 0, np.minimum(m, np.abs(np.nan_to_num(dm, nan=0.0))), m)
    i, j = np.nonzero(ok)
    cand = np.concatenate([q[i, j] + 0.5 * pq[i, j], w[i, j], dist[i, j][:, None]], axis=1)
    ident = [(2, int(x), int(y)) for x, y in zip(i, j)]
    extended = np.zeros((0, 7))
    if ext > 0:
        i, j = np.nonzero(G > -ext)
        extended = np.concatenate([q[i, j] + 0.5 * pq[i, j], w[i, j], dist[i, j][:, None]], axis=1)
    return cand, ident, float(m.min()), extended


def _first_max(vals, ok):
    """The admissible entries in descending order of vals, equal values in index order: [0] is the first maximum."""
    idx = np.flatnonzero(ok)
    return idx[np.argsort(-vals[idx], kind='stable')]


def _reduce_once(x, s, forced):
    """One run of the reduction.  forced: {stage: candidate index} overrides the winner of a stage (0 anchor, 1 farthest, 2
    farthest from the line, 3 other side).  Returns (sel, stages): stages[k] = (ranking of the admissible candidates, their
    values as lengths, tier used 0 / 1) of the stage as it ran, None where it did not run; margins of the thresholds passed."""
    n = len(s)
    smin = s.min()
    tier1 = s < smin + TIER_TOL
    stages, thresholds = [None] * 4, []
    # anchor: among the candidates within TIE_TOL of the deepest, the extreme one along the skew direction
    f = x @ SKEW
    rank = _first_max(f, s < smin + TIE_TOL)
    stages[0] = (rank, f[rank], 0)
    k0 = forced.get(0, int(rank[0]))
    d = x - x[k0]
    excl = np.zeros(n, bool)
    excl[k0] = True

    def pick(stage, vals, positive):
        for tier in (0, 1):
            ok = ~excl & (tier1 if tier == 0 else True)
            rank = _first_max(vals, ok)
            if positive and len(rank):
                thresholds.append(float(abs(vals[rank[0]])))          # the winner's (or the best loser's) distance from zero
                rank = rank[vals[rank] > 0]
            if len(rank):
                stages[stage] = (rank, vals[rank], tier)
                k = forced.get(stage, int(rank[0]))
                excl[k] = True
                return k
        return -1

    k1 = pick(1, np.sqrt(np.sum(d * d, axis=1)), False)
    e = x[k1] - x[k0]
    en = np.linalg.norm(e)
    cr = np.cross(d, e)
    with np.errstate(divide='ignore', invalid='ignore'):
        k2 = pick(2, np.nan_to_num(np.sqrt(np.sum(cr * cr, axis=1)) / en), False)
        cr2 = cr[k2]
        k3 = pick(3, np.nan_to_num(-(cr @ cr2) / (np.linalg.norm(cr2) * en)), True)
    return [k0, k1, k2] + ([k3] if k3 >= 0 else []), stages, thresholds


def reduce4(x, s):
    """Manifold reduction to at most four points.  Returns (sel, margin, info): the anchor among the candidates within TIE_TOL of
    the deepest, then the farthest point, the farthest from that line, the farthest on the other side of it (three points when
    there is none); tier 1 (within TIER_TOL of the deepest) preferred at every pick."""
    n = len(s)
    if n <= 4:
        return list(range(n)), BIG, dict(speculative=False, three=False, order_gap=BIG)
    smin = s.min()
    margin = float(min(np.abs(s - smin - TIER_TOL).min(), np.abs(s - smin - TIE_TOL).min()))
    sel, stages, thresholds = _reduce_once(x, s, {})
    margin = min([margin] + thresholds)
    order_gap = BIG
    for k, st in enumerate(stages):
        if st is None:
            continue
        rank, vals, _ = st
        gap = BIG
        if len(rank) > 1:
            order_gap = min(order_gap, float(vals[0] - vals[1]))
        for j in range(1, len(rank)):
            # a runner-up counts if choosing it changes the set of points picked (the first three are tried, the fourth counts)
            if j > 3 or set(_reduce_once(x, s, {k: int(rank[j])})[0]) != set(sel):
                gap = float(vals[0] - vals[j])
                break
        margin = min(margin, gap)
    spec = any(st is not None and st[2] == 1 for st in stages[1:])
    return sel, margin, dict(speculative=spec, three=len(sel) == 3, order_gap=order_gap)


def pair(X, sa, sb, edges=True, ext=0.0, sphere=True):
    """Narrow phase of one shape pair at the shape frames X = (R [ns, 3, 3], p [ns, 3]).  Returns dict(records [k, 12], cands
    [n, 7] {x, n, s} in candidate order, ident, sel, margin, extended [m, 7], n_cand, capped, edge_picked, speculative, three)."""
    S = shapes()
    A, B = S[sa], S[sb]
    Ra, pa, Rb, pb = X[0][sa], X[1][sa], X[0][sb], X[1][sb]
    parts = {}
    # the rule's broad phase: a pair whose bounding spheres are more than the margin apart is not examined.  (It is part of the
    # rule, not an exact shortcut: near a sharp corner the margin-grown polytope reaches beyond radius + margin, and sphere=False
    # finds speculative vertex candidates there that the rule drops -- tests/test_numpy_collide.py states what they are.)
    sph = _spheres()
    gap = sph[sa, 3] + sph[sb, 3] + MARGIN - np.linalg.norm((Ra @ sph[sa, :3] + pa) - (Rb @ sph[sb, :3] + pb))
    if sphere and gap < 0:
        return dict(cands=np.zeros((0, 7)), ident=[], n_cand=0, capped=False, extended=np.zeros((0, 7)), edge_picked=False,
                    speculative=False, three=False, sel=[], margin=float(-gap), records=np.zeros((0, 12)),
                    margin_parts=dict(sphere=float(-gap)))
    c0, i0, m0, e0 = _vertex_pass(A, Ra, pa, B, Rb, pb, 1.0, 0, ext)          # A's vertices in B: normal B -> A
    c1, i1, m1, e1 = _vertex_pass(B, Rb, pb, A, Ra, pa, -1.0, 1, ext)         # B's vertices in A: normal A -> B, flipped
    cands, ident, margin, extended = [c0, c1], i0 + i1, min(m0, m1), [e0, e1]
    if sphere:
        margin = min(margin, float(gap))
    parts['vertices'] = margin
    if edges:
        sv = np.concatenate([c0[:, 6], c1[:, 6]])[:CAND_MAX]
        lo = min(0.0, sv.min() if len(sv) else 0.0) - EDGE_SLOP
        c2, i2, m2, e2 = _edge_pass(A, Ra, pa, B, Rb, pb, lo, ext)
        cands, ident, margin, extended = cands + [c2], ident + i2, min(margin, m2), extended + [e2]
        parts['edges'] = m2
    cands = np.concatenate(cands)
    n_all = len(cands)
    cands, ident = cands[:CAND_MAX], ident[:CAND_MAX]
    out = dict(cands=cands, ident=ident, n_cand=len(cands), capped=n_all > CAND_MAX, extended=np.concatenate(extended),
               edge_picked=False, speculative=False, three=False, sel=[], margin=margin, records=np.zeros((0, 12)),
               margin_parts=parts, order_gap=BIG)
    if not len(cands):
        return out
    sel, mr, info = reduce4(cands[:, :3], cands[:, 6])
    rec = np.zeros((len(sel), 12))
    rec[:, 0], rec[:, 1], rec[:, 2] = body_id(A), body_id(B), A['link']
    rec[:, 3:10] = cands[sel]
    rec[:, 11] = A['mu'] * B['mu']
    parts['reduction'] = mr
    out.update(info, sel=sel, margin=min(margin, mr), records=rec, edge_picked=any(ident[k][0] == 2 for k in sel))
    return out


def collide(state, nobj=3, edges=True, repose=True, ext=0.0, sphere=True):
    """The contact list of one state (61): dict(records [<= MAXC, 12] in pair order, pairs [(group, sa, sb, pair dict)] of every
    pair of the table, total (contacts before the cap)).  A batch of states [..., 61] gives a list of such dicts."""
    st = np.asarray(state, dtype=np.float64)
    if st.ndim > 1:
        return [collide(s, nobj, edges, repose, ext, sphere) for s in st.reshape(-1, st.shape[-1])]
    X = shape_frames(st, repose)
    pairs = [(g, sa, sb, pair(X, sa, sb, edges, ext, sphere)) for g, sa, sb in pair_table(nobj)]
    rec = np.concatenate([np.zeros((0, 12))] + [p[3]['records'] for p in pairs])
    return dict(records=rec[:MAXC], pairs=pairs, total=len(rec))


# ---------------------------------------------------------------------------------------------- comparison with a float32 list
EXT = 1e-4                    # the extended candidate lists reach this far beyond every threshold (above THRESHOLD)
IDENT_TOL = 1e-4              # two distinct candidates of a hull pair differ by far more than this in point, normal or distance


def _diff(c, rows):
    """max |c - row| over {x, n, dist} of one record against candidate rows [m, 7]."""
    return np.abs(rows - np.asarray(c, np.float64)[3:10]).max(axis=1) if len(rows) else np.zeros(0)


def check_block(block, p, thr, tol, stats, where, partial=False):
    """One pair's block of a float32 list against the reference pair dict p.  A STABLE pair (margin above thr) must agree in
    identity -- count, ids, mu and the set of candidates picked -- and in value to tol; a SET-ASIDE pair gets the weaker check:
    every contact coincides to tol with some candidate of the pair's candidate list, extended by what the reference dropped within
    EXT of a threshold.  Returns a list of failures."""
    bad = []
    ref = p['records']
    stats['pairs'] += 1
    if p['margin'] <= thr:
        stats['aside'] += 1
        rows = np.concatenate([p['cands'][:, :7], p['extended']])
        for c in block:
            d = _diff(c, rows)
            if not len(d) or d.min() > tol:
                bad.append((where, 'set-aside pair: a contact that is no candidate', float(d.min()) if len(d) else None))
            elif len(ref) and (tuple(c[:3]) != tuple(ref[0, :3]) or np.float32(c[11]) != np.float32(ref[0, 11])):
                bad.append((where, 'set-aside pair: ids or mu'))
        return bad
    if len(block) != len(ref) and not (partial and len(block) < len(ref)):
        return [(where, 'stable pair: count', len(block), len(ref), p['margin'])]
    free = list(range(len(ref)))
    for c in block:
        d = _diff(c, ref[free, 3:10])
        k = int(np.argmin(d))
        if d[k] > IDENT_TOL:
            bad.append((where, 'stable pair: another candidate picked', float(d[k]), p['margin']))
            continue
        stats['contacts'] += 1
        stats['worst'] = max(stats['worst'], float(d[k]) / tol)
        if d[k] > tol:
            bad.append((where, 'stable pair: value', float(d[k]), p['margin']))
        if tuple(c[:3]) != tuple(ref[free[k], :3]) or np.float32(c[11]) != np.float32(ref[free[k], 11]):
            bad.append((where, 'stable pair: ids or mu'))
        free.pop(k)
    return bad


def check_list(rec, ref, thr, tol, stats, where):
    """A float32 contact list [n, 12] (the float oracle's, the device's) against collide()'s result for the state it was made
    from: the list is cut into the pairs' blocks in pair order -- a stable pair's block has the reference's count, a set-aside
    pair's block is what coincides with that pair's candidates (at most four) -- every block is checked (check_block), and nothing
    of the list may be left over.  Returns a list of failures."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 12)
    bad, cur, S = [], 0, shapes()
    for g, sa, sb, p in ref['pairs']:
        if p['margin'] > thr:
            k = min(len(p['records']), len(rec) - cur)
            if len(p['records']):
                bad += check_block(rec[cur:cur + k], p, thr, tol, stats, where + (g, sa, sb), partial=cur + k == MAXC)
        else:
            rows = np.concatenate([p['cands'][:, :7], p['extended']])
            key = (body_id(S[sa]), body_id(S[sb]), S[sa]['link'])
            k = 0
            while k < 4 and cur + k < len(rec) and tuple(rec[cur + k, :3]) == key and len(rows) and _diff(rec[cur + k], rows).min() <= tol:
                k += 1
            if k or len(p['records']):
                bad += check_block(rec[cur:cur + k], p, thr, tol, stats, where + (g, sa, sb))
        cur += k
    if cur != len(rec):
        bad.append((where, 'contacts that no pair explains, or a block cut short', cur, len(rec)))
    if len(rec) > MAXC:
        bad.append((where, 'more than MAXC contacts', len(rec)))
    return bad


def coverage(ref, cov):
    """Adds what the reference's result reaches to the coverage counts `cov` (a dict of counters)."""
    S = shapes()
    for g, sa, sb, p in ref['pairs']:
        if not len(p['records']):
            continue
        cov['group ' + g] = cov.get('group ' + g, 0) + 1
        if S[sa]['kind'] == 1 and S[sb]['kind'] == 2 and S[sa]['idx'] >= 7:
            cov['finger or skin on object %d' % S[sb]['idx']] = cov.get('finger or skin on object %d' % S[sb]['idx'], 0) + 1
        if g == 'C' and S[sa]['idx'] < 7:
            cov['arm link on the table'] = cov.get('arm link on the table', 0) + 1
        for name, hit in (('edge candidate picked', p['edge_picked']), ('more than 4 candidates', p['n_cand'] > 4),
                          ('speculative pick', p['speculative']), ('three-point manifold', p['three']),
                          ('128-candidate cap', p['capped'])):
            cov[name] = cov.get(name, 0) + int(bool(hit))
    cov['48-contact cap'] = cov.get('48-contact cap', 0) + int(ref['total'] > MAXC)
    return cov


COVERAGE_KEYS = ['group A', 'group B', 'group C', 'group D', 'arm link on the table', 'edge candidate picked',
                 'more than 4 candidates', 'speculative pick', 'three-point manifold', '128-candidate cap', '48-contact cap']
