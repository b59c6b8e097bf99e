"""GPU tests (-m gpu) of the K8 row: batched DLS IK and device-side macro plans, checked against the numpy checker
(oracle/kinematics.py -- test infrastructure, float64, same algorithm) and the reference's tracking known answers."""
import json
import os

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from oracle.kinematics import EE_LINK, generate_plan, ik_candidates, inverse_kinematics, link_pose, plan_way_points, quat_from_euler
from tests.test_ik_plan_cases import perimeter_segment_counts

pytestmark = pytest.mark.gpu
ORIENT = quat_from_euler(0, 3.14, -1.57)


IK_TOL = 1e-3       # rad: device (float32) vs checker (float64) on the same branch, both converged


def test_batched_ik_reaches_cartesian_targets():
    """Every converged device solution reaches its target to the residual pybullet is asked for (1e-3, env.py:372-375) and
    equals the checker's solution for the SAME seed to IK_TOL = 1e-3 rad in all seven joints; the seed the device picked is
    the one the checker picks (converged first, then elbow height) unless the two keys tie to 1e-4 m."""
    N = 64
    env = BatchedREALRobotEnv(N, objects=1, width=64, height=64)
    rng = np.random.default_rng(4)
    pos = np.stack([rng.uniform(-0.25, 0.05, N), rng.uniform(-0.4, 0.4, N), rng.uniform(0.42, 0.6, N)], 1)
    tg = np.concatenate([pos, np.tile(ORIENT, (N, 1))], 1)
    q, err = env.ik(tg)
    assert (err < 2e-3).mean() > 0.95
    n_same, worst = 0, 0.0
    for i in range(N):
        if err[i] < 2e-3:
            assert np.linalg.norm(link_pose(q[i].astype(np.float64), EE_LINK)[1] - pos[i]) < 3e-3
        cands = ik_candidates(np.zeros(11), pos[i], ORIENT)
        conv = [c for c in cands if c[1] < 1e-2]
        if not conv or not err[i] < 1e-2:
            assert not conv and not err[i] < 1e-2, (i, err[i], [c[1] for c in cands])     # both sides agree that nothing converged
            continue
        # the device's solution is one of the checker's candidates (final iterate; or the iterate before it when that one's
        # residual is within float32 rounding of the threshold, where the two precisions stop one update apart)
        d = [min(np.abs(c[0][:7] - q[i][:7]).max(), np.abs(c[3][:7] - q[i][:7]).max() if abs(c[4] - 1e-3) < 2e-5 else np.inf)
             for c in conv]
        k = int(np.argmin(d))
        assert d[k] < IK_TOL, (i, d, err[i])
        worst = max(worst, d[k])
        best = max(conv, key=lambda c: c[2])
        assert conv[k][2] > best[2] - 1e-4, (i, "device picked another branch", conv[k][2], best[2])
        n_same += 1
    assert n_same >= 0.9 * N
    print("device IK vs checker, same branch: worst %.2e rad over %d targets" % (worst, n_same))
    assert np.all(q[:, 7:] == 0)          # fingers keep their current values (pybullet returns all movable dofs)
    env.close()


def test_device_macro_plan_matches_host_plan_and_tracks_reference_checkpoints():
    """reference tests/test_actions.py:69-71,147-152 on the HIP path: following the plan, gripper base within 0.01 m of
    (p1, 0.6) @199, (p1, 0.46) @249, (p2, 0.46) @749 and home @999 (objects parked on the shelf)."""
    pairs = [((-0.25, -0.5), (0.05, 0.0)), ((0.05, 0.0), (-0.25, 0.5)), ((-0.25, 0.5), (-0.25, -0.5)), ((0.05, 0.0), (0.05, 0.0))]
    N = len(pairs)
    env = BatchedREALRobotEnv(N, objects=1, width=64, height=64)
    for i in range(N):
        env.set_object_pose(i, 0, [0.2, 0.0, 0.45, 0, 0, 0, 1])
    macro = np.array(pairs, dtype=np.float32)
    env.plan_macro(macro)
    plan0 = env.get_plan(0)
    assert plan0.shape == (1000, 9)
    host = generate_plan(np.zeros(11), pairs[0])
    assert np.abs(plan0[:100] - host[:100]).max() < 1e-6                        # home2 segment
    assert np.abs(plan0 - host).max() < IK_TOL                                  # same IK branches along the path, same solutions
    base = nat.LINK_NAMES.index('base')
    home = np.array([-0.55, 0.0, 1.27])
    for t in range(1000):
        env.step_plan()
        if t in (199, 249, 749, 999):
            lp = env.link_poses()[:, base, :3]
            for i, (p1, p2) in enumerate(pairs):
                tgt = {199: [p1[0], p1[1], 0.6], 249: [p1[0], p1[1], 0.46], 749: [p2[0], p2[1], 0.46], 999: home}[t]
                assert np.linalg.norm(lp[i] - tgt) < 0.01, (t, i)
    assert (env.host(nat.F_TIMESTEP) == 1000).all()
    env.close()


def test_all_36_perimeter_pairs_of_the_reference_script():
    """reference tests/test_actions.py:101-152 enumerates all 36 ordered pairs of six perimeter points and prints
    "Failed!" when the gripper base is more than 0.01 m from a way point at t = 199, 249, 749, 849, 999 (it asserts
    nothing).  The same enumeration here, one env per pair, objects parked on the shelf (test_actions.py:95-98), with the
    bounds this implementation of the documented semantics reaches (rate limit 0.2 / 0.3 rad of env.py:314-321 and the
    10 % per step position motor: 0.02-0.03 rad per step):
      * home at t = 999: < 0.01 m for all 36;
      * (p1, 0.46) at t = 249: < 0.012 m for all 36;
      * (p1, 0.6) at t = 199: < 0.01 m when p1 is not at the reach limit, < 0.012 m for (-0.25, 0) (1.8 rad of joint
        travel from home2 in 100 steps is marginal), < 0.08 m for the corners (0.05, +-0.5) where the arm is stretched
        out and the IK solution is a long way round;
      * t = 849: the script's check point there is raw_xy[849] = home2 (-0.41, 0, 1.14) -- its xy_parts list holds 500 rows of
        (p2, 0.46) and 50 of (p2, 0.6), so index 849 falls 50 steps INTO the home2 segment (test_actions.py:62-71) -- i.e.
        50 steps after a way point up to 1.6 rad away, which 0.02-0.03 rad per step cannot cover.  What IS asserted: from
        the joints at t = 799 the joints at t = 849 follow the documented recursion q <- q + 0.1 clip(home2 - q, +-maxDiff)
        (rate limit env.py:314-321, 10 % per step position motor SURVEY A.1.4) to 0.02 rad (0.03 rad at t = 899, where the
        median pair is within 1 cm of home2).  A real pybullet run of the script would settle whether its motor is faster."""
    perimeter = [(a, b) for a in (-0.25, 0.05) for b in (-0.5, 0.0, 0.5)]
    pairs = [(p1, p2) for p1 in perimeter for p2 in perimeter]
    N = len(pairs)
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    for i in range(N):
        env.set_object_pose(i, 0, [0.2, 0.0, 0.75, 0, 0, 0, 1])
        env.set_object_pose(i, 1, [0.2, -0.3, 0.75, 0, 0, 0, 1])
        env.set_object_pose(i, 2, [0.2, 0.3, 0.75, 0, 0, 0, 1])
    env.plan_macro(np.array(pairs, dtype=np.float32))
    # the p1 -> p2 rows of every pair are cut into as many constant runs as float64 arithmetic on the float32 pair gives (the
    # table pinned in tests/test_ik_plan_cases.py): 7 for the six pairs at distance 0.3, where the reference's exact float64
    # inputs give 6
    runs = []
    for i in range(N):
        mid = env.get_plan(i)[250:750].view(np.uint32)
        runs.append(1 + int((mid[1:] != mid[:-1]).any(axis=1).sum()))
    assert runs == perimeter_segment_counts(), runs
    assert [runs[i] for i, (p1, p2) in enumerate(pairs) if p1[1] == p2[1] and p1[0] != p2[0]] == [7] * 6
    base = nat.LINK_NAMES.index('base')
    home = np.array([-0.55, 0.0, 1.27])
    dist = {}
    home2_q = np.zeros(9)
    home2_q[5] = home2_q[6] = np.pi / 2
    max_diff = np.array([0.2, 0.2, 0.2, 0.2, 0.2, 0.3, 0.3, 0.1, 0.1])
    q_pred = None
    for t in range(1000):
        env.step_plan()
        if t == 799:
            q_pred = env.host(nat.F_JOINTS).astype(np.float64)
        elif 799 < t <= 899:
            q_pred = q_pred + 0.1 * np.clip(home2_q - q_pred, -max_diff, max_diff)
        if t == 849:
            dq = np.abs(env.host(nat.F_JOINTS) - q_pred).max()
            assert dq < 0.02, dq
            far = np.linalg.norm(env.link_poses()[:, base, :3] - np.array([-0.41, 0.0, 1.14]), axis=1)
            print("t=849: gripper base %.3f .. %.3f m from home2 (the reference script's 1 cm check point)" % (far.min(), far.max()))
        if t == 899:
            assert np.abs(env.host(nat.F_JOINTS) - q_pred).max() < 0.03
            far = np.linalg.norm(env.link_poses()[:, base, :3] - np.array([-0.419, 0.0, 1.14]), axis=1)
            assert np.median(far) < 0.01 and far.max() < 0.12       # a joint with more than 2 rad to go is still on its way
        if t in (199, 249, 749, 999):
            lp = env.link_poses()[:, base, :3]
            for i, (p1, p2) in enumerate(pairs):
                tgt = {199: [p1[0], p1[1], 0.6], 249: [p1[0], p1[1], 0.46], 749: [p2[0], p2[1], 0.46], 999: home}[t]
                dist[(t, i)] = float(np.linalg.norm(lp[i] - tgt))
    # Pair by pair against the oracle's run of the same script under the documented motor model (tests/golden/macro_sensitivity.json,
    # asserted on the oracle in tests/test_oracle_pins.py): the device plans with its own IK (rr_plan_macro, 1e-3 rad from the
    # checker's plans) and steps in fp32 -- its way-point distances follow the oracle's to DEV_TOL -- and the reference script's
    # own 0.01 m (tests/test_actions.py:147-152) holds wherever the documented model reaches it with that margin to spare:
    # all 36 pairs at t = 999, the 35 reachable ones at t = 749, the 18 at t = 199; at t = 249 the model itself ends 9.75 mm
    # from (p1, 0.46) for the slowest pair, so the device is held to the oracle's residual + DEV_TOL there (<= 0.0102 m).
    import json
    fx = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'macro_sensitivity.json')))
    assert [tuple(map(tuple, p)) for p in fx['pairs']] == pairs
    fixture = np.array(fx['distance_m']['kp=0.1,rate_limit=on'])
    DEV_TOL = 6e-4
    worst = {}
    for col, t in ((0, 199), (1, 249), (2, 749), (4, 999)):
        for i in range(N):
            d, f = dist[(t, i)], fixture[i, col]
            worst[t] = max(worst.get(t, 0.0), abs(d - f))
            assert abs(d - f) < DEV_TOL, (t, pairs[i], d, f)
            if f < 0.01 - DEV_TOL:
                assert d < 0.01, (t, pairs[i], d)
    print("device vs oracle way-point distances, worst difference per check point [m]:", {k: round(v, 6) for k, v in worst.items()})
    assert sum(dist[(249, i)] < 0.01 for i in range(N)) >= 30 and max(dist[(249, i)] for i in range(N)) < 0.0102
    assert (env.host(nat.F_TIMESTEP) == 1000).all() and (env.host(nat.F_ERRFLAGS) == 0).all()
    env.close()


def test_step_macro_replans_on_new_action_and_facade_macro_env():
    env = BatchedREALRobotEnv(2, objects=1, width=64, height=64)
    a = np.array([[[-0.1, -0.2], [0.0, 0.2]], [[-0.2, 0.1], [0.0, -0.3]]])
    for _ in range(5):
        env.step_macro(a)
    assert (env._macro_step == 5).all()
    b = a.copy()
    b[1, 0, 0] = -0.15
    env.step_macro(b)
    assert env._macro_step.tolist() == [6, 1]
    env.close()
    import real_robots_amd as rr
    e = rr.make('REALRobot2020-R1M1-v0', eye_width=64, eye_height=64)
    e.reset()
    act = {'macro_action': np.array([[-0.1, -0.2], [0.0, 0.2]]), 'render': False}
    for _ in range(3):
        obs, r, done, info = e.step(act)
    assert e.plan_step == 2 and e.planned_actions.shape == (1000, 9)
    c = rr.make('REALRobot2020-R2C1-v0', eye_width=64, eye_height=64)
    c.reset()
    ca = {'cartesian_command': np.array([-0.1, 0.1, 0.5, *ORIENT]), 'gripper_command': np.array([0.2, 0.1]), 'render': False}
    for _ in range(120):
        obs, r, done, info = c.step(ca)
    assert np.linalg.norm(c.get_part_pos('base') - np.array([-0.1, 0.1, 0.5])) < 0.01
    assert abs(obs['joint_positions'][7] - 0.2) < 5e-3
    e.close()
    c.close()


def test_single_seed_ik_is_the_reference_call_pattern_and_a_parameter():
    """solver={'ik_single_seed': True} (RR_SOLVER_IK_SINGLE_SEED): rr_plan_macro solves every way point ONCE from the env's current
    joints, the reference's literal call pattern (env.py:421-427).  The device's plans equal the float64 checker's plans of the same
    pattern (oracle.kinematics.generate_plan(single_seed=True)) to IK_TOL wherever the solve converged, and differ from the default's
    (best of several seeds) for some pair -- the flag acts.  What either pattern does to the reference's tracking script is the
    fixture tests/golden/ik_seed_sensitivity.json (the default meets the script's 1 cm where the literal pattern, with THIS solver,
    misses it for half of the pairs)."""
    pairs = [((-0.25, -0.5), (0.05, 0.0)), ((0.05, 0.0), (-0.25, 0.5)), ((-0.25, 0.5), (-0.25, -0.5)), ((0.05, 0.5), (0.05, -0.5)),
             ((-0.25, 0.0), (0.05, 0.5)), ((0.05, -0.5), (-0.25, 0.0))]
    N = len(pairs)
    macro = np.array(pairs, dtype=np.float32)
    plans = {}
    for single in (False, True):
        env = BatchedREALRobotEnv(N, objects=1, width=64, height=64, solver={'ik_single_seed': single})
        env.plan_macro(macro)
        plans[single] = np.stack([env.get_plan(i) for i in range(N)])
        env.close()
    home2 = np.zeros(9)
    home2[5] = home2[6] = np.pi / 2
    worst, n_cmp = 0.0, 0
    rows = [150, 225, 300, 500, 740, 775]                           # one row of every IK segment
    for i, pr in enumerate(pairs):
        # the checker's plan of the same pattern, way point by way point (generate_plan(single_seed=True) row for row), with the
        # number of updates each solve took: a row is compared iff its float64 solve converged before update 500 of 1000 (a
        # solve that has not ends wherever its iterations leave it: float32 and float64 differ freely there) -- and EVERY such
        # row agrees to IK_TOL; they are at least 70 % of the rows (28 of 36 for the checker alone)
        way = plan_way_points(macro[i].astype(np.float64))
        for r in rows:
            first, target = [w for w in way if w[0] <= r][-1]
            q, err, _, _, _, updates = ik_candidates(np.zeros(11), target, ORIENT, single_seed=True)[0]
            if not updates < 500:
                continue
            d = np.abs(plans[True][i][r] - q[:9]).max()
            assert d < IK_TOL, (pr, r, d, err, updates)
            n_cmp += 1
            worst = max(worst, d)
        assert np.abs(plans[True][i][:100] - home2).max() < 1e-6 and np.abs(plans[True][i][800:900] - home2).max() < 1e-6
        assert np.abs(plans[True][i][900:]).max() < 1e-6
    assert n_cmp >= 0.7 * 6 * N, n_cmp
    assert np.abs(plans[True] - plans[False]).max() > 0.1
    fx = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'ik_seed_sensitivity.json')))['table']
    assert fx['kp=0.5,ik_single_seed=False']['pairs_within_1cm'][1:] == [36, 35, 36, 36]
    assert fx['kp=0.5,ik_single_seed=True']['pairs_within_1cm'][1] < 30
    print("single-seed plans: all %d of %d IK rows whose float64 solve converged equal the checker's to %.0e rad (worst %.2e)" % (n_cmp, 6 * N, IK_TOL, worst))
