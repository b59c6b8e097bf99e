"""CPU: the float64 numpy narrow phase (tests/numpy_collide.py) against the oracle's (oracle/rr_oracle.c collide_pair / collide).

The oracle and the device kernel are the same algorithm written operation for operation by the same hand
(tests/test_gpu_contacts_fuzz.py holds them bit for bit); numpy_collide restates the documented rule on another road and without
any cull.  Against the float64 build it must agree to 1e-9 in points, normals and distances and exactly in ids, counts, order and
mu -- both sides are float64 with the same inputs -- pair by pair (Oracle.pair_contacts) and as whole lists (Oracle.contacts()),
with the edge pass on and off.  Against the float32 build -- whose lists the device's are, bit for bit -- a pair whose decision
margin (computed by the reference alone) is above THRESHOLD must agree in identity (count, ids, mu, the set of candidates picked)
and in value to TOLERANCE; the pairs below it are set aside, at most SET_ASIDE_CAP of the pairs that produce output, and still
every one of their contacts must coincide to TOLERANCE with a candidate of the reference's list for that pair, extended by what it
dropped within numpy_collide.EXT of a threshold.

MEASURED on the float32 oracle build (python -m tests.test_numpy_collide 3000 40: this file's states plus 3000 random postures
and poses and 40 command trajectories, all seeded; edge pass on; 4379 states, 20269 pairs with output, 184 of them disagreeing in
identity): the largest decision margin of a pair that disagreed in identity was 2.71e-8 m, the next 2.66e-8, 1.08e-8, 8.3e-9 -- every
disagreement sat on an (almost) exact tie, far below one float32 rounding of these lengths, because the margin is a minimum over
every decision of a pair and rounding comes near very few of them.  THRESHOLD, the smallest value at which no stable pair disagrees,
doubled for states not sampled, is 5.5e-8 (4.6 % of the pairs are then set aside).  The largest difference over the stable pairs was
4.87e-7, doubled: TOLERANCE = 1e-6.  (The test's own 179 states alone gave 1.93e-9 and 2.01e-7: too small a sample.)  Both come
from the oracle build and are never tuned on the device; tests/test_gpu_numpy_collide.py imports them.  numpy_collide.check_list,
the comparison a device list needs (it cuts a whole list into the pairs' blocks), also runs here on the float32 oracle's lists.

A FINDING of the cull-free reference (test_the_bounding_sphere_rule_drops_only_far_speculative_candidates): the bounding-sphere test
of collide_pair is not an exact shortcut of the vertex rule.  Near a sharp corner the margin-grown polytope reaches beyond radius +
margin, and the vertex rule alone would give a speculative candidate there (seen: 16.7 mm and 19.2 mm away) that the sphere test
drops, in the oracle and on the device alike.  The reference therefore states the sphere test as part of the rule (sphere=True).
"""
import numpy as np
import pytest

from oracle.kinematics import generate_plan
from oracle.oracle import Oracle
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_collide as nc
from tests import numpy_step as ns
from tests.test_gpu_contacts_fuzz import _grasp_script
from tests.test_oracle_pins import _edge_crossing_pose
from tests.test_pair_cull import random_state

THRESHOLD = 5.5e-8            # decision margin (m) above which a pair is stable (measured 2.71e-8, see above)
TOLERANCE = 1e-6              # |float32 - numpy| of points, normals, distances over the stable pairs (measured 4.87e-7)
SET_ASIDE_CAP = 0.10
F64_TOL = 1e-9

_states_cache = {}
_ref_cache = {}


def _f32(s):
    return np.asarray(s, np.float32).astype(np.float64)


def _mat_to_quat(R):
    w = np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def states():
    """[(tag, objects, state61 rounded to float32)], seeded: trajectories under full-range random commands (links pressed into the
    table) and under macro plans (pushes) for 1-3 objects, the grasp script, the edge-crossing poses, random postures and poses
    like test_pair_cull's, an object sunk into the table, the bottle teleported around the wrist (the 128-candidate cap), a pile
    of objects on the gripper pressed on the table (the 48-contact cap)."""
    if _states_cache:
        return _states_cache['s']
    out = []
    for nobj in (1, 2, 3):
        for seed in (1, 2):
            o = Oracle(nobj, 32, 32)
            o.reset()
            for t in range(360):
                o.step(synthetic_actions([seed], t, seed=seed)[0].astype(np.float64))
                if t % 30 == 29:
                    out.append(('commands', nobj, _f32(o.state)))
        o = Oracle(nobj, 32, 32)
        o.reset()
        rng = np.random.default_rng(10 + nobj)
        plan = generate_plan(o.state[:11], rng.uniform([-0.15, -0.35], [-0.05, 0.35], size=(2, 2)) * [[1, 1], [1, -1]])
        for t in range(800):
            o.step(np.asarray(plan[t], np.float64))
            if t >= 240 and t % 40 == 0:
                out.append(('macro', nobj, _f32(o.state)))
    o = Oracle(1, 32, 32)
    o.reset()
    for _ in range(100):
        o.step(None)
    for t, c in enumerate(_grasp_script()):
        o.step(c.astype(np.float64))
        if t >= 262 and t % 8 == 0:
            out.append(('grasp', 1, _f32(o.state)))
    for gap, tilt in [(0.002, -40.0), (0.0005, -55.0), (-0.001, -40.0), (0.012, -30.0), (-0.0003, -50.0), (0.019, -45.0)]:
        o.reset()
        s = o.state
        s[22:29] = _edge_crossing_pose(gap, tilt)[0]
        out.append(('edge', 1, _f32(s)))
    o = Oracle(3, 32, 32)
    rng = np.random.default_rng(20261017)
    for case in range(45):
        random_state(o, rng, case)
        out.append(('random', 3, _f32(o.state)))
    # special poses: the cube sunk 1 cm into the table top; the bottle around the wrist; the three objects around the gripper
    # with the arm pressed on the table
    o.reset()
    s = o.state
    s[22:25] = [-0.1, 0.0, 0.2794 + 0.03]
    out.append(('sunk', 3, _f32(s)))
    S = nc.shapes()
    wrist = [k for k, sh in enumerate(S) if sh['kind'] == 1 and sh['idx'] == 6][0]
    for q3 in (0.6, 1.1):
        s = o.state
        s[:11] = [0.3, q3, 0.0, -1.2, 0.0, 0.5, 0.0, 0, 0, 0, 0]
        R, p = nc.shape_frames(s, repose=False)
        c = R[wrist] @ S[wrist]['V'].mean(0) + p[wrist]
        s[22 + 26:25 + 26], s[25 + 26:29 + 26] = c, _mat_to_quat(R[wrist])
        out.append(('wrist', 3, _f32(s)))
        tip = R[wrist] @ (S[wrist]['V'].mean(0) + [0, 0, 0.12]) + p[wrist]
        for k in range(3):
            s[22 + 13 * k:25 + 13 * k] = tip + [0.03 * (k - 1), 0.02 * (k - 1), 0.0]
        out.append(('pile', 3, _f32(s)))
    _states_cache['s'] = out
    return out


def reference(k, edges):
    """collide() of state k without the re-pose (what Oracle.pair_contacts sees), cached over the tests."""
    if (k, edges) not in _ref_cache:
        _, nobj, s = states()[k]
        _ref_cache[(k, edges)] = nc.collide(s, nobj, edges=edges, repose=False, ext=nc.EXT)
    return _ref_cache[(k, edges)]


def _selection(edges):
    """Every state with the edge pass on; every third one (and all edge-crossing poses) with it off."""
    return [k for k, (tag, _, _) in enumerate(states()) if edges or k % 3 == 0 or tag == 'edge']


def _assert_coverage(cov, edges):
    print("coverage: " + ', '.join('%s %d' % kv for kv in sorted(cov.items())))
    need = nc.COVERAGE_KEYS + ['finger or skin on object %d' % i for i in range(3)]
    missing = [k for k in need if not cov.get(k) and not (k == 'edge candidate picked' and not edges)]
    assert not missing, missing
    if not edges:
        assert not cov.get('edge candidate picked')


@pytest.mark.parametrize('edges', [1, 0], ids=['edges', 'no_edges'])
def test_float64_oracle_pair_by_pair_and_whole_lists(edges):
    """1e-9 in points, normals, distances; ids, counts, order and mu exact -- every pair of the table through
    Oracle.pair_contacts, and the whole list of the step through Oracle.contacts() (pair order, the 48-contact cap, the
    out-of-bounds re-pose before the narrow phase).  The one exception that turned up, exact ties, is stated where it is handled."""
    oracles = {n: Oracle(n, 32, 32, edge_contacts=edges) for n in (1, 2, 3)}
    cov, npairs, ncont, worst, lists, permuted = {}, 0, 0, 0.0, 0, 0
    for k in _selection(edges):
        tag, nobj, s = states()[k]
        o = oracles[nobj]
        ref = reference(k, edges)
        nc.coverage(ref, cov)
        o.state = s
        for g, sa, sb, p in ref['pairs']:
            c = o.pair_contacts(sa, sb)[0]
            assert len(c) == len(p['records']), (tag, k, g, sa, sb, len(c), len(p['records']), p['margin'])
            if len(c):
                npairs += 1
                ncont += len(c)
                assert np.array_equal(c[:, [0, 1, 2, 11]], p['records'][:, [0, 1, 2, 11]]), (tag, k, g, sa, sb)
                d = float(np.abs(c[:, 3:10] - p['records'][:, 3:10]).max())
                if d > F64_TOL and min(p['order_gap'], p['margin']) < 1e-12:
                    # the one exception that turned up: an EXACT tie of a first-maximum selection (gap below 1e-12 m: float64
                    # rounding).  A square face resting flat has its second and third corner equidistant from the diagonal
                    # through the anchor, and the same points come out in another order (held as a set, to 1e-9); two vertices
                    # mirror images of each other about the line give another third point (held to the reference's candidates,
                    # to 1e-9).  Which of the two is the first maximum is rounding, on either side.
                    probe = dict(pairs=0, aside=0, contacts=0, worst=0.0)
                    assert not nc.check_block(c, p, 1e-12, F64_TOL, probe, (tag, k, g, sa, sb))
                    permuted += 1
                    continue
                worst = max(worst, d)
                assert d <= F64_TOL, (tag, k, g, sa, sb, d, p['margin'])
        # the whole list of a step from this state: the re-pose of an object out of bounds comes first
        full = ref if not ns.out_of_bounds(s[22:61].reshape(3, 13)[:nobj, :3]).any() else nc.collide(s, nobj, edges=edges)
        o.state = s
        o.step(None)
        c = o.contacts()
        assert len(c) == len(full['records']) == min(full['total'], nc.MAXC), (tag, k, len(c), full['total'])
        if len(c):
            assert np.array_equal(c[:, [0, 1, 2, 11]], full['records'][:, [0, 1, 2, 11]]), (tag, k)
            if np.abs(c[:, 3:10] - full['records'][:, 3:10]).max() > F64_TOL:      # (an exact tie, see above: block by block as sets)
                assert any(len(p['records']) and min(p['order_gap'], p['margin']) < 1e-12 for _, _, _, p in full['pairs']), (tag, k)
                probe = dict(pairs=0, aside=0, contacts=0, worst=0.0)
                assert not nc.check_list(c, full, 1e-12, F64_TOL, probe, (tag, k))
        lists += 1
    print("\nfloat64 oracle, edges=%d: %d pairs compared, %d contacts compared, %d whole lists, set-aside share 0 (none is set aside), "
          "worst share of the tolerance used %.2g" % (edges, npairs, ncont, lists, worst / F64_TOL))
    print("pairs whose points came out in another order on an exact tie (order gap below 1e-12): %d" % permuted)
    _assert_coverage(cov, edges)


def test_an_object_out_of_bounds_is_reposed_before_the_narrow_phase():
    """The whole-list comparison of a state with an object below the table top: its contacts are those of the start pose."""
    o = Oracle(3, 32, 32)
    o.reset()
    for _ in range(150):
        o.step(None)
    s = o.state
    s[22:25] = [0.2, 0.0, 0.1]
    s = _f32(s)
    assert ns.out_of_bounds(s[22:25])
    ref = nc.collide(s, 3)
    o.state = s
    o.step(None)
    c = o.contacts()
    probe = dict(pairs=0, aside=0, contacts=0, worst=0.0)
    assert len(c) == len(ref['records']) > 0 and not nc.check_list(c, ref, -1.0, F64_TOL, probe, ())
    assert nc.check_list(c, nc.collide(s, 3, repose=False), -1.0, F64_TOL, probe, ())      # (without the re-pose: another list)


def test_the_bounding_sphere_rule_drops_only_far_speculative_candidates():
    """Without the sphere test the vertex rule finds more, over every state of this file: only in pairs whose spheres are apart, and
    only speculative candidates more than 1.5 cm away (no force can come from them within a step below 3 m/s of closing speed).  It
    does find some: the sphere test is a rule of its own, not a shortcut.  The table of spheres itself is checked against the
    vertices: every sphere contains its shape, and none is more than 1 % larger than the farthest vertex asks for."""
    sph = nc._spheres()
    for s, sh in enumerate(nc.shapes()):
        r = np.linalg.norm(sh['V'] - sph[s, :3], axis=1).max()
        assert r <= sph[s, 3] * (1 + 1e-6) and sph[s, 3] <= 1.01 * r + 1e-6, (s, r, sph[s, 3])
    extra = 0
    for k, (tag, nobj, s) in enumerate(states()):
        X = nc.shape_frames(s, repose=False)
        for g, sa, sb, p in reference(k, 1)['pairs']:
            if p['margin_parts'].get('sphere') is None:
                continue
            q = nc.pair(X, sa, sb, sphere=False)
            extra += len(q['records'])
            assert all(c[9] > 0.015 for c in q['records']), (k, sa, sb, q['records'])
    print("\ncontacts of the vertex rule that the bounding-sphere rule drops: %d (all more than 1.5 cm away)" % extra)
    assert extra > 0


def measure_float32(edges, verbose=False):
    """The float32 oracle build pair by pair against the reference: returns (stats, failures, cov, rows) with rows = per pair with
    output (margin, identity agrees, largest difference of the matched contacts) -- what THRESHOLD and TOLERANCE were measured on."""
    oracles = {n: Oracle(n, 32, 32, f32=True, edge_contacts=edges) for n in (1, 2, 3)}
    stats = dict(pairs=0, aside=0, contacts=0, worst=0.0)
    bad, cov, rows = [], {}, []
    for k in _selection(edges):
        tag, nobj, s = states()[k]
        o = oracles[nobj]
        ref = reference(k, edges)
        nc.coverage(ref, cov)
        o.state = s
        for g, sa, sb, p in ref['pairs']:
            c = o.pair_contacts(sa, sb)[0]
            if not len(c) and not len(p['records']):
                continue
            bad += nc.check_block(c, p, THRESHOLD, TOLERANCE, stats, (tag, k, g, sa, sb))
            if verbose:
                probe = dict(pairs=0, aside=0, contacts=0, worst=0.0)
                fails = nc.check_block(c, p, -1.0, 1.0, probe, ())
                ident = not [f for f in fails if 'value' not in f[1]]
                rows.append((p['margin'], ident, probe['worst']))
    return stats, bad, cov, rows


@pytest.mark.parametrize('edges', [1, 0], ids=['edges', 'no_edges'])
def test_float32_oracle_stable_pairs_agree_and_set_aside_pairs_pick_candidates(edges):
    stats, bad, cov, _ = measure_float32(edges)
    share = stats['aside'] / max(stats['pairs'], 1)
    print("\nfloat32 oracle, edges=%d: %d pairs compared, %d contacts compared, set-aside share %.3f, worst share of the tolerance "
          "used %.2f" % (edges, stats['pairs'], stats['contacts'], share, stats['worst']))
    assert not bad, bad[:10]
    assert stats['pairs'] > (500 if edges else 150) and share <= SET_ASIDE_CAP, (stats, share)
    _assert_coverage(cov, edges)


def test_float32_whole_lists_cut_into_pair_blocks():
    """check_list (what the GPU test runs on the device's lists) on the float32 oracle's whole lists."""
    oracles = {n: Oracle(n, 32, 32, f32=True) for n in (1, 2, 3)}
    stats = dict(pairs=0, aside=0, contacts=0, worst=0.0)
    bad, n = [], 0
    for k in _selection(1):
        tag, nobj, s = states()[k]
        if ns.out_of_bounds(s[22:61].reshape(3, 13)[:nobj, :3]).any():
            continue
        o = oracles[nobj]
        o.state = s
        o.step(None)
        bad += nc.check_list(o.contacts(), reference(k, 1), THRESHOLD, TOLERANCE, stats, (tag, k))
        n += 1
    share = stats['aside'] / max(stats['pairs'], 1)
    print("\nfloat32 oracle, whole lists: %d lists, %d pairs compared, %d contacts compared, set-aside share %.3f, worst share of the "
          "tolerance used %.2f" % (n, stats['pairs'], stats['contacts'], share, stats['worst']))
    assert not bad, bad[:10]
    assert n > 100 and stats['contacts'] > 1500 and share <= SET_ASIDE_CAP


def _more_states(n_random, seeds):
    """A larger seeded sample for the measurement: more random postures and poses, more command trajectories."""
    out = []
    o = Oracle(3, 32, 32)
    rng = np.random.default_rng(77)
    for case in range(n_random):
        random_state(o, rng, case)
        out.append(('random+', 3, _f32(o.state)))
    for seed in seeds:
        nobj = 1 + seed % 3
        o = Oracle(nobj, 32, 32)
        o.reset()
        for t in range(600):
            o.step(synthetic_actions([seed], t, seed=seed)[0].astype(np.float64))
            if t % 20 == 19:
                out.append(('commands+', nobj, _f32(o.state)))
    return out


if __name__ == '__main__':
    # python -m tests.test_numpy_collide [n_random [n_trajectories]]: the measurement THRESHOLD and TOLERANCE come from, on the
    # test's states plus a larger seeded sample
    import sys
    n_random = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    states()
    _states_cache['s'] = _states_cache['s'] + _more_states(n_random, range(3, 3 + (int(sys.argv[2]) if len(sys.argv) > 2 else 9)))
    _, _, _, rows = measure_float32(1, verbose=True)
    rows = np.array(rows, dtype=float)
    dis = rows[rows[:, 1] == 0]
    thr = float(dis[:, 0].max()) if len(dis) else 0.0
    stable = rows[rows[:, 0] > thr]
    print("%d states, %d pairs with output; %d disagree in identity, margins (largest first) %s" % (
        len(states()), len(rows), len(dis), np.sort(dis[:, 0])[::-1][:8]))
    print("measured threshold %.3g; largest difference over the stable pairs %.3g; set aside at 2 x threshold: %.3f" % (
        thr, stable[:, 2].max(), float((rows[:, 0] <= 2 * thr).mean())))
