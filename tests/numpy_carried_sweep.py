"""A float64 restatement of the swept clearance with carried objects (rr_carried_sweep, include/realrobot.h), for the tests (a helper
module: pytest does not collect it).

Built from tests/numpy_sweep.py (the reach table, the joint masks, the advancement's rules) and tests/numpy_carry.py (the carried
rows: T_object = T_link(q) o rel composed in float64 through the link table, another road than the device's body table): the lower
bounds are tests/numpy_distance.reference on numpy_carry.carried_rows(state, q(t), links, rel), the bounds are
numpy_sweep.reach_table() with, for a shape of an object attached to a link on body b, the mask "ancestors-or-self of b" and the
reach chain[k][b] + rho, rho = |centre of the shape's bounding sphere in b's frame| + its radius.  It calls no kernel.

The fixture tests/golden/carried_sweep.npz (make_carried_sweep.py): N = 4 envs, K = 8 segments, 18 pairs, the float64 profile of every
pair at 65 uniform t WITH THE CARRIED OBJECTS MOVING, and the nearest pair's profile of the arm alone (the objects left where the
state has them).  Env 0 nothing attached; env 1 the cube on the gripper base, rel captured; env 2 the cube on finger_01 and the tomato
on lbr_iiwa_link_4, rel given; env 3 all three on the gripper base, rel captured.

Negative controls (CONTROLS), the wrong kernels a test must be able to tell from a right one:
  object_left_behind          -- the objects are staged from the state and have no joints: what k_swept_clearance would do;
  carried_shape_has_no_joints -- the carried objects move, but a carried shape's mask is empty: a (carried, static) pair gets
                                 B = 0 and is never looked at again;
  staged_at_start_only        -- the right bound, but the object is composed at t = 0 and frozen there."""
import os

import numpy as np

from real_robots_amd.model import load_model
from tests import numpy_carry as nc
from tests import numpy_collide as ncol
from tests import numpy_distance as nd
from tests import numpy_step as ns
from tests import numpy_sweep as sw

CONTROLS = ('object_left_behind', 'carried_shape_has_no_joints', 'staged_at_start_only')
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'carried_sweep.npz')
N, K, SAMPLES = 4, 8, sw.SAMPLES
LINK_BASE, LINK_FINGER, LINK_MID = nc.LINK_BASE, nc.LINK_FINGER, nc.LINK_MID
LINKS = np.array([[-1, -1, -1], [LINK_BASE, -1, -1], [LINK_FINGER, LINK_MID, -1], [LINK_BASE, LINK_BASE, LINK_BASE]], np.int32)
CAPTURED = np.array([1, 1, 0, 1], np.uint8)          # env 2's rel poses are GIVEN
ROWS = [(e, k) for e in range(N) for k in range(K)]


def chain_table():
    """C [11, 11] float64: C[k, b] = the sum of |body_jpos[m]| over the bodies m on the chain from b up to, but not including, k; 0
    where joint k is not an ancestor-or-self of body b."""
    m = ns.model()
    C = np.zeros((ns.NB, ns.NB))
    for b in range(ns.NB):
        r, k = 0.0, b
        while k >= 0:
            C[k, b] = r
            r = r + np.linalg.norm(np.asarray(m['body_jpos'][k], dtype=np.float64))
            k = m['parent'][k]
    return C


def rho(link, rel7, s):
    """|centre of shape s's bounding sphere in the frame of the body that carries link| + its radius, for an object at rel7 (xyz + xyzw)
    in the link's COM frame."""
    m = ns.model()
    sph = np.array(load_model()['shape_sphere'], dtype=np.float64)[s]
    rel7 = np.asarray(rel7, dtype=np.float64)
    x = rel7[:3] + nc.quat_to_mat(rel7[3:]) @ sph[:3]
    return float(np.linalg.norm(np.asarray(m['link_pos'][link], dtype=np.float64) + np.asarray(m['link_rot'][link], dtype=np.float64) @ x) + sph[3])


def masks_and_reach(pairs, links, rel):
    """(M [Q, 2, 11] bool, R [Q, 2, 11]) of the two shapes of every pair: a robot shape's own, the carrying body's mask and
    chain + rho for a shape of an attached object (links [n_obj], rel [n_obj, 7] of the env), nothing for the rest."""
    S, m = ncol.shapes(), ns.model()
    RT, JM, C = sw.reach_table(), sw.joint_masks(), chain_table()
    pairs = np.asarray(pairs).reshape(-1, 2)
    M, R = np.zeros((len(pairs), 2, ns.NB), bool), np.zeros((len(pairs), 2, ns.NB))
    for j in range(len(pairs)):
        for side in range(2):
            s = int(pairs[j, side])
            M[j, side], R[j, side] = JM[s], RT[:, s]
            if S[s]['kind'] == 2 and links[S[s]['idx']] >= 0:
                l = int(links[S[s]['idx']])
                b = int(m['link_body'][l])
                M[j, side] = np.asarray(m['anc'][b]) > 0
                R[j, side] = np.where(M[j, side], C[:, b] + rho(l, rel[S[s]['idx']], s), 0.0)
    return M, R


def pair_bounds(dq, pairs, links, rel, control=None):
    """B [Q]: sum over the joints in exactly one of the two masks of |dq_k| (reach_a[k] + reach_b[k])."""
    if control in ('object_left_behind', 'carried_shape_has_no_joints'):
        return sw.pair_bounds(dq, pairs)
    M, R = masks_and_reach(pairs, links, rel)
    adq = np.abs(np.asarray(dq, dtype=np.float64))
    return np.array([(adq * (R[j, 0] + R[j, 1]))[M[j, 0] ^ M[j, 1]].sum() for j in range(len(M))])


def carried_row(state_row, q, links, rel):
    """The state row [61] float64 at posture q with every attached object where its link carries it."""
    return nc.carried_rows(np.asarray(state_row, dtype=np.float64)[None], np.asarray(q, dtype=np.float64)[None, None], np.asarray(links)[None],
                           np.asarray(rel, dtype=np.float64)[None])[0]


def lower_bounds(state_row, q, pairs, links, rel):
    """The float64 lower bound of every pair at posture q with the carried objects carried there: the exact distance, 0 where the hulls overlap."""
    return np.maximum(nd.reference(carried_row(state_row, q, links, rel)[None], pairs)['d'][0], 0.0)


def advance(state_row, q0, q1, pairs, links, rel, safety, tolerance, control=None, max_steps=sw.MAX_STEPS, b_scale=1.0, low_shift=0.0):
    """The advancement of one segment with carried objects -> numpy_sweep.advance's dict.  b_scale, low_shift: every B times the one,
    every lower bound plus the other (the tests' probe for borderline decisions)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    if control == 'object_left_behind':
        return sw.advance(state_row, q0, q1, pairs, safety, tolerance, max_steps=max_steps)
    dq, Q = q1 - q0, len(pairs)
    B = pair_bounds(dq, pairs, links, rel, control) * b_scale
    frozen = carried_row(state_row, q0, links, rel) if control == 'staged_at_start_only' else None
    free, t, steps, evals = np.zeros(Q), 0.0, 0, 0
    while True:
        due = np.nonzero(free <= t)[0]
        q = q0 + t * dq
        low = sw.lower_bounds(frozen, q, pairs[due]) if frozen is not None else lower_bounds(state_row, q, pairs[due], links, rel)
        g = np.maximum(low + low_shift, 0.0) - safety
        steps, evals = steps + 1, evals + len(due)
        ok = g > tolerance
        hits = due[~ok]
        with np.errstate(divide='ignore'):
            free[due[ok]] = np.where(B[due[ok]] > 0, t + g[ok] / np.where(B[due[ok]] > 0, B[due[ok]], 1.0), np.inf)
        out = dict(steps=steps, evaluations=evals, q_stop=q)
        if len(hits):
            return dict(out, status=1, fraction=t, pair=int(hits.min()), free=np.minimum(free, 1.0))
        tn = free.min()
        if tn >= 1.0:
            return dict(out, status=0, fraction=1.0, pair=-1, free=np.minimum(free, 1.0))
        if steps >= max_steps:
            return dict(out, status=3, fraction=t, pair=int(np.argmin(free)), free=np.minimum(free, 1.0))
        t = tn


def profile(state_row, seg, pairs, links, rel, samples=SAMPLES):
    """[samples, Q] float64: the signed distance of every pair at uniform t along the segment, the carried objects moving."""
    t = np.arange(samples) / (samples - 1.0)
    q0, q1 = np.asarray(seg[0], dtype=np.float64), np.asarray(seg[1], dtype=np.float64)
    rows = nc.carried_rows(np.asarray(state_row, dtype=np.float64)[None], (q0 + t[:, None] * (q1 - q0))[None], np.asarray(links)[None],
                           np.asarray(rel, dtype=np.float64)[None])
    return nd.reference(rows, pairs)['d']


def carried_pairs(pairs, links):
    """[Q] bool: the pair has a shape of an object attached in this env (links [n_obj])."""
    S = ncol.shapes()
    return np.array([any(S[s]['kind'] == 2 and links[S[s]['idx']] >= 0 for s in p) for p in np.asarray(pairs).reshape(-1, 2).tolist()])


def classify(prof, arm_nearest, seg, safety, carried):
    """The classes of one row from its profile [65, Q], the arm-alone nearest profile [65], its end postures and the carried pairs [Q]
    -> a set: numpy_sweep.classify's classes, and `carried_hits_arm_free` where a pair with a carried shape comes within safety midway
    while the arm alone stays clear of safety by more than 5 mm."""
    out = sw.classify(prof, seg, safety)
    t = np.arange(len(prof)) / (len(prof) - 1.0)
    below = np.nonzero(prof.min(axis=1) <= safety)[0]
    if len(below) and t[below[0]] > 0.1 and arm_nearest.min() > safety + 5e-3 and carried[np.argmin(prof[below[0]])]:
        out.add('carried_hits_arm_free')
    return out


_fix = None


def fixture():
    """The committed fixture: states [4, 61] and segments [4, 8, 2, 11] float32, pairs [Q, 2], links [4, 3], rel [4, 3, 7] float64 (the
    reference's: captured in float64 from the float32 states, env 2's given), rel_given [4, 3, 7] float32 (what env 2 hands to the
    library), profile [4, 8, 65, Q] and arm_nearest [4, 8, 65] float64, restated [4, 8, 4] int32 ({status, pair, steps, evaluations} of `advance`), safety,
    tolerance.  Loaded once per process and left unchanged."""
    global _fix
    if _fix is None:
        z = np.load(FIXTURE)
        _fix = {k: z[k] for k in z.files}
        _fix['safety'], _fix['tolerance'] = float(z['safety']), float(z['tolerance'])
        assert (_fix['links'] == LINKS).all()
    return _fix


def classes():
    f = fixture()
    return {(e, k): classify(f['profile'][e, k], f['arm_nearest'][e, k], f['segments'][e, k].astype(np.float64), f['safety'], carried_pairs(f['pairs'], f['links'][e]))
            for e, k in ROWS}


_runs = {}


def run(e, k, control=None, b_scale=1.0, low_shift=0.0):
    """The restatement (or a control, or a probe) on row (e, k) of the fixture, computed once per process."""
    key = (e, k, control, b_scale, low_shift)
    if key not in _runs:
        f = fixture()
        _runs[key] = advance(f['states'][e], f['segments'][e, k, 0], f['segments'][e, k, 1], f['pairs'], f['links'][e], f['rel'][e], f['safety'], f['tolerance'],
                             control, b_scale=b_scale, low_shift=low_shift)
    return _runs[key]
