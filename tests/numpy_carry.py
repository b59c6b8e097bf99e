"""A float64 reference of the posture queries with CARRIED objects (rr_set_attachments, include/realrobot.h), for the tests (a helper
module: pytest does not collect it).

It takes another road than the kernels: the COM frame of the carrying link comes from tests/numpy_kinematics._link_frames(q) (the
link table of rr_link_poses, not the moving body's frame the device table holds), T_object = T_link o rel is composed in float64
with quaternions turned into matrices, and the result is SUBSTITUTED into the object columns of the rows of numpy_posture.rows; on
those rows run tests/numpy_distance.reference, numpy_penetration.compare and numpy_signed_gradient's formula and witnesses,
unchanged.  The gradient's reference is central differences of that float64 signed distance WITH THE CARRIED OBJECT MOVING -- the
rows are composed anew at q +- H e_k --, not a Jacobian formula.

The fixture (seeded, N = 5 envs, three objects, K = 3 postures) is the smallest that can still go wrong: every attachment pattern
once -- env 0 none, env 1 the cube on link 8 (the gripper base), env 2 the cube on a finger link and the tomato on a mid-arm link,
env 3 all three on link 8, env 4 the mustard with a GIVEN rel pose that has nothing to do with where its state puts it -- and pair
tables of seven (no multiple of the four waves) and of two pairs (waves 2 and 3 without a pair)."""
import numpy as np

from real_robots_amd import _native as nat
from tests import numpy_collide as ncol
from tests import numpy_distance as nd
from tests import numpy_kinematics as nk
from tests import numpy_posture as npo
from tests import numpy_rays as nr
from tests import numpy_signed_gradient as nsg
from tests import numpy_step as ns

N, NOBJ, K = 5, 3, 3
SEED = 7                      # chosen on the CPU so that tests/test_numpy_carry.py's conditions hold
LINK_BASE, LINK_FINGER, LINK_MID = 8, 10, 4          # gripper `base`, finger_01, lbr_iiwa_link_4
LINKS = np.array([[-1, -1, -1], [LINK_BASE, -1, -1], [LINK_FINGER, LINK_MID, -1], [LINK_BASE, LINK_BASE, LINK_BASE], [-1, -1, LINK_BASE]], np.int32)
CAPTURED = np.array([1, 1, 1, 1, 0], np.uint8)        # the envs whose rel poses are captured from the state; env 4's is GIVEN
GIVEN = np.array([0.02, -0.03, 0.16, 0.1, -0.2, 0.3, 0.9])          # env 4's mustard in link 8's COM frame (the quaternion is not normalised: the library does that)
MOVE = 0.35                   # rad: joint 1 of the "it moves" posture, away from the attach posture


def quat_to_mat(q):
    """xyzw quaternions [..., 4] (normalised here) -> rotation matrices [..., 3, 3], float64."""
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def object_pose(state, o):
    """(R [..., 3, 3], p [..., 3]) of object o in state rows [..., 61]."""
    st = np.asarray(state, dtype=np.float64)
    c = 22 + 13 * o
    return quat_to_mat(st[..., c + 3:c + 7]), st[..., c:c + 3]


def capture(state, links):
    """rel [N, n_obj, 7] float64: T_link(q)^-1 o T_object of state [N, 61] for every attached object (links [N, n_obj] >= 0), the
    identity pose for a free one."""
    st = np.asarray(state, dtype=np.float64)
    links = np.asarray(links)
    Rl, pl = nk._link_frames(st[:, :ns.NB])
    rel = np.zeros(links.shape + (7,))
    rel[..., 6] = 1.0
    for e, o in zip(*np.nonzero(links >= 0)):
        Ro, po = object_pose(st[e], o)
        R, p = Rl[e, links[e, o]], pl[e, links[e, o]]
        rel[e, o, :3] = R.T @ (po - p)
        rel[e, o, 3:] = nk.mat_to_quat(R.T @ Ro)
    return rel


def rel_in_link(rows, links, K_):
    """The pose of every attached object of rows [N * K, 61] in its link's frame AT THE ROW'S OWN JOINTS -> [N * K, n_obj, 7]: for a
    carried object it is the same in all K rows of an env."""
    return capture(rows, np.repeat(np.asarray(links), K_, axis=0))


def carried_rows(state, postures, links, rel):
    """state [N, 61], postures [N, K, 11], links [N, n_obj], rel [N, n_obj, 7] -> the N * K rows of numpy_posture.rows as float64 with
    the pose columns of every attached object replaced by T_link(posture) o rel."""
    po = np.asarray(postures, dtype=np.float64)
    rows = npo.rows(np.asarray(state, dtype=np.float64), po)
    links, rel = np.asarray(links), np.asarray(rel, dtype=np.float64)
    Kp = po.shape[1]
    Rl, pl = nk._link_frames(rows[:, :ns.NB])
    for e, o in zip(*np.nonzero(links >= 0)):
        Rr, tr = quat_to_mat(rel[e, o, 3:]), rel[e, o, :3]
        c = 22 + 13 * o
        for r in range(e * Kp, (e + 1) * Kp):
            R, p = Rl[r, links[e, o]], pl[r, links[e, o]]
            rows[r, c:c + 3] = p + R @ tr
            rows[r, c + 3:c + 7] = nk.mat_to_quat(R @ Rr)
    return rows


def attached_items(links, pairs, K_):
    """[N * K, Q] bool: the item has a shape of an attached object on either side."""
    S = ncol.shapes()
    links = np.asarray(links)
    obj = np.array([[S[s]['idx'] if S[s]['kind'] == 2 else -1 for s in p] for p in np.asarray(pairs).reshape(-1, 2).tolist()])      # [Q, 2]
    att = np.concatenate([links >= 0, np.zeros((len(links), 1), bool)], 1)                                                         # (column -1: not an object)
    per_env = att[:, obj[:, 0]] | att[:, obj[:, 1]]                                                                                # [N, Q]
    return np.repeat(per_env, K_, axis=0)


def masks(links, pairs, K_):
    """(mA, mB) [N * K, Q, 11]: joint k moves shape A / B of the item -- a robot shape's body, or the body that carries an attached
    object; no columns for a static shape or a free object."""
    S, m = ncol.shapes(), ns.model()
    links = np.asarray(links)
    pairs = np.asarray(pairs).reshape(-1, 2)
    out = np.zeros((2, len(links), len(pairs), ns.NB))
    for side in range(2):
        for j, s in enumerate(pairs[:, side].tolist()):
            if S[s]['kind'] == 1:
                out[side, :, j] = m['anc'][S[s]['idx']]
            elif S[s]['kind'] == 2:
                for e in range(len(links)):
                    l = links[e, S[s]['idx']]
                    if l >= 0:
                        out[side, e, j] = m['anc'][int(m['link_body'][l])]
    return np.repeat(out[0], K_, axis=0), np.repeat(out[1], K_, axis=0)


def differences(state, postures, links, rel, pairs, items, h=nsg.H):
    """(d0, dplus, dminus) of numpy_signed_gradient.differences on the listed (row, pair) items, with the carried objects moving: the
    rows are composed anew at postures +- h e_k.  Everything else stays NaN."""
    po = np.asarray(postures, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    R, Q = po.shape[0] * po.shape[1], len(pairs)
    d0, dp, dm = np.full((R, Q), np.nan), np.full((R, Q, ns.NB), np.nan), np.full((R, Q, ns.NB), np.nan)
    steps = [(None, 0.0)] + [(k, sg * h) for k in range(ns.NB) for sg in (1.0, -1.0)]
    for k, dq in steps:
        p = po.copy()
        if k is not None:
            p[:, :, k] += dq
        rows = carried_rows(state, p, links, rel)
        for r in sorted(set(i[0] for i in items)):
            js = sorted(set(i[1] for i in items if i[0] == r))
            d = nd.reference(rows[r:r + 1], pairs[js])['d'][0]
            if k is None:
                d0[r, js] = d
            else:
                (dp if dq > 0 else dm)[r, js, k] = d
    return d0, dp, dm


# ---------------------------------------------------------------------------------------------- the tests' inputs (fixed seed)
def seven_pairs():
    n = nd.names()
    return np.array([(n['cube'], n['shelf']), (n['cube'], n['table']), (n['cube'], n['finger_00']), (n['cube'], n['tomato']),
                     (n['tomato'], n['lbr_iiwa_link_6']), (n['lbr_iiwa_link_5'], n['table']), (n['mustard'], n['cube'])], np.int32)


def two_pairs():
    n = nd.names()
    return np.array([(n['cube'], n['table']), (n['mustard'], n['cube'])], np.int32)


def own_link_pair():
    """(cube, the shape of link 8): in an env whose cube is carried by link 8 its distance does not depend on the joints."""
    n = nd.names()
    return np.array([(n['cube'], n['base'])], np.int32)


_fix = {}


def inputs():
    """(state [5, 61] f32, postures [5, 3, 11] f32, links [5, 3] i32, given rel pose [5, 3, 7] f32 (env 4's row counts)): the attach
    state and K postures, the attach posture + U(-0.5, 0.5) rad clipped to the joint limits."""
    if 'in' not in _fix:
        rng = np.random.default_rng(SEED)
        st = nr.states(N, NOBJ, SEED + 100).astype(np.float64)
        lim = ns.model()['body_limits']
        st[:, 7:11] = np.clip(st[:, 7:11], lim[7:11].min(1) * 0.3, lim[7:11].max(1) * 0.3)           # (fingers half open: something fits between them)
        n = {name: nat.LINK_NAMES.index(name) for name in ('skin_00', 'skin_10', 'finger_01', 'lbr_iiwa_link_4')}

        def put(e, o, pos):
            st[e, 22 + 13 * o:25 + 13 * o] = pos
        between = lambda e: 0.5 * (ns.link_pose(st[e, :11], n['skin_00'])[1] + ns.link_pose(st[e, :11], n['skin_10'])[1])
        put(1, 0, between(1))
        put(2, 0, ns.link_pose(st[2, :11], n['finger_01'])[1] + [0.0, 0.0, -0.05])
        put(2, 1, ns.link_pose(st[2, :11], n['lbr_iiwa_link_4'])[1] + [0.05, 0.09, 0.0])
        put(3, 0, between(3))
        put(3, 1, between(3) + [0.03, 0.0, 0.02])
        put(3, 2, between(3) + [-0.05, 0.03, 0.0])
        st = st.astype(np.float32)
        po = st[:, None, :11].astype(np.float64) + rng.uniform(-0.5, 0.5, size=(N, K, 11))
        po = np.clip(po, lim.min(1), lim.max(1)).astype(np.float32)
        rel = np.zeros((N, NOBJ, 7), np.float32)
        rel[..., 6] = 1.0
        rel[4, 2] = GIVEN
        _fix['in'] = (st, np.ascontiguousarray(po), LINKS.copy(), rel)
    return _fix['in']


def moved_posture():
    """[5, 1, 11] f32: every env's attach posture with joint 1 moved by MOVE rad (towards the middle of its range)."""
    st = inputs()[0]
    lim = ns.model()['body_limits']
    po = st[:, None, :11].astype(np.float64).copy()
    mid = 0.5 * (lim[1].min() + lim[1].max())
    po[:, 0, 1] += np.where(po[:, 0, 1] > mid, -MOVE, MOVE)
    return np.ascontiguousarray(po.astype(np.float32))


def reference_rel():
    """The rel poses [5, 3, 7] float64 of the fixture as float64 computes them: captured for envs 0..3, GIVEN (normalised) for env 4."""
    st, _, links, given = inputs()
    rel = capture(st, np.where(CAPTURED[:, None] > 0, links, -1))
    g = given[4, 2].astype(np.float64)
    rel[4, 2] = np.concatenate([g[:3], g[3:] / np.linalg.norm(g[3:])])
    return rel


def golden():
    """tests/golden/carry_gradient.npz (tests/golden/make_carry.py) as a dict of arrays, loaded once."""
    import os
    if 'golden' not in _fix:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'carry_gradient.npz')) as z:
            _fix['golden'] = {k: z[k] for k in z.files}
        assert int(_fix['golden']['seed']) == SEED, 'tests/golden/carry_gradient.npz was made for another seed: python -m tests.golden.make_carry'
    return _fix['golden']


def reference(rel=None, pairs=None, postures=None):
    """numpy_distance.reference on the carried rows of the fixture (rel: what attachments() read back, None: float64's own capture; pairs
    None: the seven; postures None: the fixture's K).  The float64-capture reference of the seven pairs is computed once per process."""
    st, po, links, _ = inputs()
    key = 'ref' if rel is None and pairs is None and postures is None else None
    if key and key in _fix:
        return _fix[key]
    ref = nd.reference(carried_rows(st, po if postures is None else postures, links, reference_rel() if rel is None else rel),
                       seven_pairs() if pairs is None else pairs)
    if key:
        _fix[key] = ref
    return ref
