"""Writes tests/golden/carried_sweep.npz: the fixture of the carried-sweep tests (tests/numpy_carried_sweep.py reads it).

    python tests/golden/make_carried_sweep.py            (about a minute of float64 qhull on eight processes)

states [4, 61] and segments [4, 8, 2, 11] float32, pairs [18, 2] and links [4, 3] int32, rel [4, 3, 7] float64 (the reference's rel
poses: captured in float64 from the float32 states for envs 1 and 3, given for env 2), rel_given [4, 3, 7] float32 (what env 2 hands
to the library), profile [4, 8, 65, 18] float64 -- the signed distance (tests/numpy_distance.reference) of every pair at 65 uniform t
along every segment WITH THE CARRIED OBJECTS MOVING --, arm_nearest [4, 8, 65] float64 -- the nearest pair's distance with the objects
left where the state has them --, restated [4, 8, 4] int32 -- {status, pair, steps, evaluations} of the float64 restatement
(numpy_carried_sweep.advance), which tests/test_numpy_carried_sweep.py computes again --, safety = 0.01 and tolerance = 1e-3.

Env 0 has nothing attached and is env 0 of the swept-clearance fixture (its cube where finger_00's bounding sphere is half way, tm = 0.5),
the tomato moved off the shelf.  Envs
1..3 hold their objects past the finger tips and beside the gripper, clear of every robot shape of the pair table; the state has
each object where its link holds it at the base motion's start qa.  The base motion (qa, qa + dq), |dq|inf = 0.5 rad, open
fingers, is one a seeded random search found (BASES): the arm alone stays clear of everything by 4 cm while a carried shape passes
through the table or the shelf between two ends that are clear by 3 cm; in env 1 the motion is clear of everything and the FREE tomato
is put where the carried cube's centre is half way.  With tm the t of the deepest sample, the eight rows of an env:
  0 free                 qa -> qa + 0.25 tm dq
  1 hit midway           qa -> qa + (tm + 0.1) dq
  2 tunnel               qa -> qa + dq
  3 start in collision   qa + tm dq -> qa + dq
  4 zero length, free        qa -> qa
  5 zero length, colliding   qa + tm dq -> the same
  6 the tunnel backwards     qa + dq -> qa
  7 the fingers close while the arm backs away: the (carried, finger) pairs get a bound
The classes are asserted on the profiles alone, as tests/test_numpy_carried_sweep.py asserts them again."""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import numpy_carried_sweep as cs  # noqa: E402
from tests import numpy_carry as nc  # noqa: E402
from tests import numpy_collide as ncol  # noqa: E402
from tests import numpy_distance as nd  # noqa: E402
from tests import numpy_kinematics as nk  # noqa: E402
from tests import numpy_step as ns  # noqa: E402
from tests import numpy_sweep as sw  # noqa: E402
from tests.golden import make_swept_clearance as base  # noqa: E402

SAFETY, TOLERANCE = base.SAFETY, base.TOLERANCE
OPEN = base.OPEN
# where the objects are held, in the COM frame of the carrying link (xyz + xyzw): past the finger tips, beside the gripper, beside the arm
HOLD = {(1, 0): (cs.LINK_BASE, (0.0, 0.0, 0.24, 0.0, 0.0, 0.0, 1.0)),
        (2, 0): (cs.LINK_FINGER, (0.0, 0.0, 0.14, 0.1, -0.2, 0.3, 0.9)), (2, 1): (cs.LINK_MID, (0.0, 0.16, 0.0, 0.3, 0.0, 0.1, 0.9)),
        (3, 0): (cs.LINK_BASE, (0.0, 0.0, 0.24, 0.0, 0.0, 0.383, 0.924)), (3, 1): (cs.LINK_BASE, (0.0, 0.16, 0.02, 0.0, 0.0, 0.0, 1.0)),
        (3, 2): (cs.LINK_BASE, (0.0, -0.17, 0.0, 0.0, 0.707, 0.0, 0.707))}
# (qa[0..6], dq[0..6]) of the base motions of envs 1..3, |dq|inf = 0.5 rad: found by a seeded random search for the docstring's conditions
BASES = {1: (np.array([-0.197, 0.548, -0.073, -1.013, 0.753, -0.851, 0.395]), np.array([-0.5, -0.216, 0.439, -0.5, 0.422, 0.377, 0.454])),
         2: (np.array([-0.577, 0.655, -0.067, -0.705, -0.077, 1.511, -0.19]), np.array([0.201, -0.034, 0.135, 0.093, 0.286, -0.5, -0.436])),
         3: (np.array([0.723, 1.261, -0.485, -0.372, -0.148, -0.161, -0.485]), np.array([-0.5, -0.242, -0.113, -0.058, 0.168, -0.096, -0.285]))}
PARK = {1: (-0.2, 0.75, 0.9), 2: (-0.2, -0.75, 0.9)}          # a free object that plays no part: in the air beside the table


def pair_table():
    n = nd.names()
    t = [('cube', 'table'), ('cube', 'shelf'), ('cube', 'tomato'), ('cube', 'base'), ('cube', 'finger_00'), ('cube', 'finger_11'),
         ('tomato', 'table'), ('tomato', 'shelf'), ('tomato', 'lbr_iiwa_link_6'), ('mustard', 'table'), ('mustard', 'cube'), ('mustard', 'shelf'),
         ('finger_00', 'table'), ('finger_10', 'shelf'), ('base', 'table'), ('lbr_iiwa_link_6', 'table'),
         ('finger_01', 'finger_11'),          # link x link: the joints 0..6 are above both
         ('skin_01', 'shelf')]
    return np.array([(n[a], n[b]) for a, b in t], np.int32)


def held_state(row, e, qa):
    """row [61] float64 with q = qa, no velocities and env e's attached objects where HOLD has them at qa; the others parked."""
    row = row.copy()
    row[:11], row[11:22] = qa, 0.0
    for o in range(3):
        c = 22 + 13 * o
        row[c + 7:c + 13] = 0.0
        if (e, o) in HOLD:
            l, rel = HOLD[e, o]
            R, p = ns.link_pose(qa, l)
            row[c:c + 3] = p + R @ np.array(rel[:3])
            row[c + 3:c + 7] = nk.mat_to_quat(R @ nc.quat_to_mat(rel[3:]))
        else:
            row[c:c + 3] = PARK[o]
            row[c + 3:c + 7] = (0.0, 0.0, 0.0, 1.0)
    return row


def _rel(e, row32):
    rel = nc.capture(row32[None].astype(np.float64), np.where(cs.CAPTURED[e], cs.LINKS[e], -1)[None])[0]
    for o in range(3):
        if cs.LINKS[e, o] >= 0 and not cs.CAPTURED[e]:
            g = np.array(HOLD[e, o][1], dtype=np.float32).astype(np.float64)
            rel[o] = np.concatenate([g[:3], g[3:] / np.linalg.norm(g[3:])])
    return rel


def base_motion(e, pairs, template):
    """Env e's base motion -> (state row float32, qa, dq, tm), its conditions asserted on a 17-sample profile."""
    qa, dq = np.concatenate([BASES[e][0], OPEN]), np.concatenate([BASES[e][1], np.zeros(4)])
    assert np.abs(dq).max() == 0.5
    carried = cs.carried_pairs(pairs, cs.LINKS[e])
    row = held_state(template, e, qa).astype(np.float32)
    rel_e = _rel(e, row)
    if e == 1:
        l, rel = HOLD[e, 0]
        R, p = ns.link_pose(qa + 0.5 * dq, l)
        row[35:38] = p + R @ np.array(rel[:3])          # the free tomato in the cube's way
    seg = np.stack([qa, qa + dq])
    prof = cs.profile(row, seg, pairs, cs.LINKS[e], rel_e, samples=17)
    arm = base._profile((row, seg, pairs, 17)).min(axis=1)
    d = prof[:, carried].min(axis=1)
    print('env %d: deepest %.3f at t %.3f by pair %d, ends %.3f %.3f, arm alone %.3f, pairs without a carried shape %.3f'
          % (e, d.min(), d.argmin() / 16.0, prof[d.argmin()].argmin(), d[0], d[-1], arm.min(), prof[:, ~carried].min()))
    assert arm.min() > SAFETY + 0.03 and prof[:, ~carried].min() > SAFETY + 0.03 and d[0] > SAFETY + 0.02 and d[-1] > SAFETY + 0.02 and d.min() < -0.01 and 4 <= d.argmin() <= 12
    return row, qa, dq, d.argmin() / 16.0


def build():
    pairs = pair_table()
    st0, sg0 = base.build()
    template = nd.states(1, 41)[0].astype(np.float64)
    states, segs = np.zeros((cs.N, 61), np.float32), np.zeros((cs.N, cs.K, 2, 11))
    rel = np.zeros((cs.N, 3, 7))
    rel[..., 6] = 1.0
    close = np.zeros(11)
    close[[7, 9]] = -0.4
    for e in range(cs.N):
        if e == 0:
            states[0] = st0[0]
            states[0, 35] = -0.1          # (the tomato off the shelf: this table has the (tomato, shelf) pair)
            qa, dq, tm = sg0[0, 0, 0].astype(np.float64), (sg0[0, 2, 1] - sg0[0, 2, 0]).astype(np.float64), 0.5
        else:
            states[e], qa, dq, tm = base_motion(e, pairs, template)
            rel[e] = _rel(e, states[e])
        qm, qb = qa + tm * dq, qa + dq
        segs[e] = [(qa, qa + 0.25 * tm * dq), (qa, qa + (tm + 0.1) * dq), (qa, qb), (qm, qb), (qa, qa), (qm, qm), (qb, qa), (qa, qa - 0.3 * dq + close)]
    given = np.zeros((cs.N, 3, 7), np.float32)
    given[..., 6] = 1.0
    for (e, o), (l, r) in HOLD.items():
        if not cs.CAPTURED[e]:
            given[e, o] = r
    return states, segs.astype(np.float32), pairs, rel, given


def _profiles(args):
    row, seg, pairs, links, rel = args
    r = cs.advance(row, seg[0], seg[1], pairs, links, rel, SAFETY, TOLERANCE)
    return cs.profile(row, seg, pairs, links, rel), base._profile((row, seg, pairs, cs.SAMPLES)).min(axis=1), (r['status'], r['pair'], r['steps'], r['evaluations'])


def main():
    states, segs, pairs, rel, given = build()
    with mp.Pool(8) as pool:
        got = pool.map(_profiles, [(states[e], segs[e, k], pairs, cs.LINKS[e], rel[e]) for e, k in cs.ROWS])
    prof = np.array([g[0] for g in got]).reshape(cs.N, cs.K, cs.SAMPLES, len(pairs))
    arm = np.array([g[1] for g in got]).reshape(cs.N, cs.K, cs.SAMPLES)
    restated = np.array([g[2] for g in got], np.int32).reshape(cs.N, cs.K, 4)
    print('the restatement: status', restated[..., 0].tolist(), 'steps', restated[..., 2].tolist())
    count = {}
    for e, k in cs.ROWS:
        cls = cs.classify(prof[e, k], arm[e, k], segs[e, k].astype(np.float64), SAFETY, cs.carried_pairs(pairs, cs.LINKS[e]))
        B = cs.pair_bounds(segs[e, k, 1].astype(np.float64) - segs[e, k, 0].astype(np.float64), pairs, cs.LINKS[e], rel[e])
        d = prof[e, k].min(axis=1)
        print('row (%d, %d): %-50s min d %+.4f at t %.3f (pair %d), d(0) %+.4f, d(1) %+.4f, arm alone %+.4f, rate / bound %.3f, still pairs move %.2g'
              % ((e, k, ','.join(sorted(cls)), d.min(), d.argmin() / (cs.SAMPLES - 1.0), prof[e, k][d.argmin()].argmin(), d[0], d[-1], arm[e, k].min()) + sw.rate_ratio(prof[e, k], B)))
        for c in cls:
            count[c] = count.get(c, 0) + 1
    print(count)
    for e in range(cs.N):
        got = [cs.classify(prof[e, k], arm[e, k], segs[e, k].astype(np.float64), SAFETY, cs.carried_pairs(pairs, cs.LINKS[e])) for k in range(cs.K)]
        assert 'free' in got[0] and 'free' in got[4] and 'tunnel' in got[2] and 'tunnel' in got[6] and 'start_in_collision' in got[3] and 'start_in_collision' in got[5], (e, got)
        assert e == 0 or ('carried_hits_arm_free' in got[1] and 'carried_hits_arm_free' in got[2]), (e, got)
    np.savez_compressed(cs.FIXTURE, states=states, segments=segs, pairs=pairs, links=cs.LINKS, rel=rel, rel_given=given, profile=prof, arm_nearest=arm, restated=restated,
                        safety=np.float64(SAFETY), tolerance=np.float64(TOLERANCE))
    print('wrote', cs.FIXTURE, os.path.getsize(cs.FIXTURE), 'bytes')


if __name__ == '__main__':
    main()
