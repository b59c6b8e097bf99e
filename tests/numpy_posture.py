"""A float64 reference of the clearance queries at candidate postures (rr_posture_clearance, include/realrobot.h), for the tests (a
helper module: pytest does not collect it).

Posture (e, k) is env e's state row with its eleven joint columns replaced, so the reference is tests/numpy_distance.py, unchanged,
on the N * K substituted rows; what this module adds is the reduction: the nearest pair of a row, when the reference alone can decide
it, and a wrapper that holds the nearest records to every bound of numpy_distance.compare."""
import numpy as np

from tests import numpy_collide as ncol
from tests import numpy_distance as nd

CONTROLS = ('neighbours_posture', 'neighbour_envs_postures', 'posture_ignored')


def rows(state, postures):
    """state [N, 61], postures [N, K, 11] -> the N * K state rows [N * K, 61] with substituted joints, row e * K + k."""
    st, po = np.asarray(state), np.asarray(postures)
    N, K = po.shape[:2]
    out = np.repeat(st, K, axis=0).copy()
    out[:, :11] = po.reshape(N * K, 11)
    return out


def clearance(ref):
    """What takes part in the minimum, [R, Q]: the sphere gap where culled, else the distance (0 where the hulls overlap)."""
    return np.where(ref['culled'], ref['gap'], np.maximum(ref['d'], 0.0))


def nearest(ref):
    """(j* [R], decided [R]) of a reference over R rows: with c the clearance, m = min c and S = {j : c_j < m + DECIDE}, a row is
    decided when every item of S is decided and either |S| == 1 (one pair nearer than all others by a millimetre) or m == 0 (the
    tie of overlapping pairs at zero, which goes to the lowest index); then j* = min S.  An undecided row's j* means nothing."""
    c = clearance(ref)
    m = c.min(axis=1)
    S = c < (m + nd.DECIDE)[:, None]
    decided = (ref['decided'] | ~S).all(axis=1) & ((S.sum(axis=1) == 1) | (m == 0))
    return S.argmax(axis=1), decided


def first_minimum(row_distance):
    """The device's reduction rule on a distance row [..., Q], restated: d < best over ascending j from best = +inf, pair 0 where
    nothing is below +inf -- the first minimum, and a NaN never wins."""
    d = np.asarray(row_distance)
    flat = d.reshape(-1, d.shape[-1])
    out = np.zeros(len(flat), np.int64)
    for r, row in enumerate(flat):
        best = np.inf
        for j, x in enumerate(row):
            if x < best:
                best, out[r] = x, j
    return out.reshape(d.shape[:-1])


def compare_nearest(out, ref, tol, pairs, jstar, decided):
    """The nearest records of the device (host columns of posture_clearance flattened to R rows) against the reference on the
    decided nearest rows: rows are grouped by winning pair, and each group goes through numpy_distance.compare as a one-pair
    table, with the reference's `world` keys remapped to the group's row numbers.  Returns (figures, failures)."""
    fig, fails = {}, []
    for j in sorted(set(jstar[decided].tolist())):
        r = np.nonzero(decided & (jstar == j))[0]
        cols = {k: np.asarray(out[k])[r][:, None] for k in ('distance', 'lower', 'point_a', 'point_b', 'normal', 'status')}
        sub = {k: ref[k][r, j][:, None] for k in ('d', 'v', 'gap', 'culled', 'decided', 'expect')}
        sub['world'] = {(i, s): ref['world'][int(e), s] for i, e in enumerate(r) for s in pairs[j].tolist()}
        f, bad = nd.compare(cols, sub, tol, pairs[j:j + 1])
        for k, v in f.items():
            fig[k] = fig.get(k, 0) + v if k in ('items', 'decided', 'separated', 'overlapping', 'culled') else max(fig.get(k, v), v)
        fails += ['pair %d: %s' % (j, b) for b in bad]
    return fig, fails


def compare(out, ref, tol, pairs):
    """Everything of the device's output that is judged against a reference (host columns of posture_clearance with the leading
    [N, K] flattened to R rows): per item the status on decided items, |distance - exact| on decided separated items, no status 3;
    per decided nearest row the winning pair and the record.  Returns (figures, failures); figures first, then the verdicts."""
    pd, ps = np.asarray(out['pair_distance'], dtype=np.float64), np.asarray(out['pair_status'])
    dec = ref['decided']
    sep = dec & (ref['expect'] == 0)
    jstar, rowdec = nearest(ref)
    fig = dict(items=int(dec.size), decided=int(dec.sum()), rows=len(jstar), decided_rows=int(rowdec.sum()))
    fig['status_mismatches'] = int((ps[dec] != ref['expect'][dec]).sum())
    fig['status3_on_decided'] = int((ps[dec] == 3).sum())
    fig['distance_error'] = float(np.abs(pd - ref['d'])[sep].max()) if sep.any() else 0.0
    fig['cull_gap_error'] = float(np.abs(pd - ref['gap'])[dec & ref['culled']].max()) if (dec & ref['culled']).any() else 0.0
    fig['pair_mismatches'] = int((np.asarray(out['pair'])[rowdec] != jstar[rowdec]).sum())
    fails = ['%s %d > 0' % (k, fig[k]) for k in ('status_mismatches', 'status3_on_decided', 'pair_mismatches') if fig[k]]
    if not fig['distance_error'] <= tol:
        fails.append('distance_error %.3g > %.3g' % (fig['distance_error'], tol))
    if not fig['cull_gap_error'] <= nd.GAP_TOL:
        fails.append('cull_gap_error %.3g > %.3g' % (fig['cull_gap_error'], nd.GAP_TOL))
    ok = rowdec & (np.asarray(out['pair']) == jstar)            # (a row with the wrong winner is counted above: its record belongs to another pair)
    nfig, nfails = compare_nearest(out, ref, tol, pairs, jstar, ok)
    fig.update({'nearest_' + k: v for k, v in nfig.items()})
    return fig, fails + nfails


# ---------------------------------------------------------------------------------------------- the tests' inputs (fixed seeds)
def robot_pairs():
    """ROBOT_PAIRS: the pairs of the step's collision table with a robot shape on either side (80 of 92)."""
    S = ncol.shapes()
    return np.array([p for p in nd.collision_pairs(3).tolist() if S[p[0]]['kind'] == 1 or S[p[1]]['kind'] == 1], np.int32)


def case_r_inputs():
    """Case R: N = 4, K = 4 -- (state [4, 61], postures [4, 4, 11], pairs [80, 2])."""
    return nd.states(4, 115), np.ascontiguousarray(nd.states(16, 116)[:, :11].reshape(4, 4, 11)), robot_pairs()


def control_postures(state, postures, control):
    """The postures a deliberately wrong implementation would have used."""
    if control == 'neighbours_posture':
        return np.roll(postures, 1, axis=1)
    if control == 'neighbour_envs_postures':
        return np.roll(postures, 1, axis=0)
    if control == 'posture_ignored':
        return np.ascontiguousarray(np.broadcast_to(np.asarray(state)[:, None, :11], postures.shape))
    raise ValueError(control)


_refs = {}


def case_r(max_distance=None, variant=None, control=None):
    """The reference of case R over its 16 rows (or a variant's / a control's), computed once per process and left unchanged.  The
    cull changes no distance, so a culled reference is derived from the plain one of the same variant / control."""
    key = (max_distance, variant, control)
    if key not in _refs:
        st, po, pairs = case_r_inputs()
        if max_distance is not None:
            plain = case_r(None, variant, control)
            ref = dict(plain)
            ref['culled'] = plain['gap'] > max_distance
            ref['decided'] = np.where(np.abs(plain['gap'] - max_distance) >= nd.DECIDE_CULL, (np.abs(plain['d']) >= nd.DECIDE) | ref['culled'], False)
            ref['expect'] = np.where(ref['culled'], 2, np.where(plain['d'] > 0, 0, 1))
        else:
            ref = nd.reference(rows(st, po if control is None else control_postures(st, po, control)), pairs, variant=variant)
        _refs[key] = ref
    return _refs[key]


def grid_inputs():
    """The grid case: N = 67, K = 2, one pair (skin_00 x cube)."""
    n = nd.names()
    return nd.states(67, 105), np.ascontiguousarray(nd.states(134, 106)[:, :11].reshape(67, 2, 11)), np.array([(n['skin_00'], n['cube'])], np.int32)


def grid_case():
    if 'grid' not in _refs:
        st, po, pairs = grid_inputs()
        _refs['grid'] = nd.reference(rows(st, po), pairs)
    return _refs['grid']
