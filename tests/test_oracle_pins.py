"""CPU tests (-m "not gpu"): pin the oracle against the known answers the reference tree holds and against
independent restatements (URDF-direct FK fixture, numpy mass matrix, analytic free fall / motor lag)."""
import json
import os

import numpy as np
import pytest

from oracle.oracle import Oracle, LINK_NAMES
from tests import numpy_camera as nc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, 'golden', 'fk_golden.json')))


def q11_from_cmd(cmd):
    q = np.zeros(11)
    q[:7] = cmd[:7]
    q[7] = q[9] = cmd[7]
    q[8] = q[10] = -cmd[8]
    return q


def set_q(o, q11):
    s = o.state
    s[:11] = q11
    s[11:22] = 0
    o.state = s


def test_fk_matches_urdf_fixture():
    o = Oracle(3, 32, 32)
    for case in GOLD['cases']:
        set_q(o, q11_from_cmd(np.array(case['cmd'])))
        for link, pos in case['links'].items():
            got = o.link_pose(link)[:3]
            assert np.allclose(got, pos, atol=2e-6), (link, got, pos)


def test_reference_known_answers_home_postures():
    """reference tests/test_actions.py:60,65-66,150: gripper base at home / home2 within 0.01 m."""
    ka = GOLD['reference_known_answers']
    o = Oracle(3, 32, 32)
    assert np.linalg.norm(o.link_pose('base')[:3] - ka['home_base']) < ka['tolerance']
    h2 = np.zeros(9)
    h2[5] = h2[6] = np.pi / 2
    set_q(o, q11_from_cmd(h2))
    assert np.linalg.norm(o.link_pose('base')[:3] - ka['home2_base']) < ka['tolerance']


def test_reference_tracking_home2_then_home():
    """reference tests/test_actions.py:69-71,147-152: following the plan, `base` is within 0.01 m of the checkpoint
    at the end of each 100-step segment (home2 segment, then home)."""
    ka = GOLD['reference_known_answers']
    o = Oracle(3, 32, 32)
    h2 = np.zeros(9)
    h2[5] = h2[6] = np.pi / 2
    for _ in range(100):
        o.step(h2)
    assert np.linalg.norm(o.link_pose('base')[:3] - ka['home2_base']) < ka['tolerance']
    for _ in range(100):
        o.step(np.zeros(9))
    assert np.linalg.norm(o.link_pose('base')[:3] - ka['home_base']) < ka['tolerance']


def test_rest_heights_generate_goals_thresholds():
    """reference generate_goals.py:249-272 isOnTable: cube/mustard z < 0.33, tomato z < 0.34 once settled;
    settle criterion generate_goals.py:46 (dpos < 1e-4)."""
    o = Oracle(3, 32, 32)
    for _ in range(400):
        o.step(None)
    _, _, p = o.obs()
    prev = p.copy()
    o.step(None)
    _, _, p = o.obs()
    assert np.abs(p - prev).max() < 1e-4
    top = 0.08 + 0.199403
    assert top + 0.035 < p[0, 2] < 0.33       # cube centre = top + 0.04 minus bevel
    assert top + 0.05 < p[1, 2] < 0.34        # tomato upright: top + 0.0532
    assert top + 0.03 < p[2, 2] < 0.33        # mustard lying on its side
    assert np.allclose(p[:, :2], [[-0.1, 0.0], [-0.1, -0.3], [-0.1, 0.3]], atol=0.03)


def test_free_fall_matches_semi_implicit_euler():
    o = Oracle(1, 32, 32)
    v, z, dt, k = 0.0, o.obs()[2][0, 2], 0.005, 0.04      # z0 = 0.45 (stored as float32 in the model blob)
    for _ in range(25):
        o.step(None)
        v = v + dt * (-v * (k + k * abs(v))) - dt * 9.81
        z = z + dt * v
        assert abs(o.obs()[2][0, 2] - z) < 1e-9


def test_motor_first_order_lag():
    """unobstructed joint follows q <- q + 0.1 (target - q) (kp 0.1, kd 1, dt 0.005)."""
    o = Oracle(1, 32, 32)
    tgt = np.zeros(9)
    tgt[0] = 0.15
    q = 0.0
    for _ in range(30):
        o.step(tgt)
        q = q + 0.1 * (0.15 - q)
        assert abs(o.obs()[0][0] - q) < 1e-6


def test_action_protocol_rate_limit_clip_coupling():
    o = Oracle(1, 32, 32)
    big = np.array([3.0, -3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 1.5, 1.5])
    o.step(big)
    j, _, _ = o.obs()
    # env.py:317: the target moves at most maxDiff per step; the motor covers 10% of it
    maxdiff = np.array([.2, .2, .2, .2, .2, .3, .3, .1, .1])
    # (all 11 motors driven at once: 50 PGS sweeps leave a few % coupling residual, hence the tolerance)
    assert np.allclose(np.abs(j), 0.1 * maxdiff, atol=4e-3)
    assert np.all(np.abs(j) <= 0.1 * maxdiff * 1.12)
    # clipping to [min_joints, max_joints] (robot.py:58-67,192) and gripper coupling a[8] <= 2 a[7] (robot.py:193),
    # exercised on collision-free motions
    o.reset()
    cmd = np.zeros(9)
    cmd[0], cmd[6] = 3.0, -3.1
    cmd[7], cmd[8] = 0.4, 1.5
    for _ in range(600):
        o.step(cmd)
    j, _, _ = o.obs()
    assert abs(j[0] - 0.666 * np.pi) < 2e-3
    assert abs(j[6] + 0.972 * np.pi) < 2e-3
    assert abs(j[7] - 0.4) < 2e-3 and abs(j[8] - 0.8) < 2e-3


def test_non_finite_action_rejected():
    o = Oracle(1, 32, 32)
    a = np.zeros(9)
    a[3] = np.nan
    assert o.step(a) == -1            # the reference asserts (robot.py:189)
    assert o.timestep == 0


def test_out_of_bounds_object_reset():
    """env.py:257-264: z < 0.08 or (x > 0.11 and z < 0.29) -> object_poses."""
    o = Oracle(2, 32, 32)
    o.set_object_pose(0, [0.5, 0.5, 0.05, 0, 0, 0, 1])
    o.set_object_pose(1, [0.2, 0.0, 0.25, 0, 0, 0, 1])
    o.step(None)
    _, _, p = o.obs()
    assert np.allclose(p[0], [-0.1, 0.0, 0.45], atol=1e-3)
    assert np.allclose(p[1], [-0.1, -0.3, 0.45], atol=1e-3)


def test_mass_matrix_against_independent_numpy_formula():
    """M = sum_b m_b Jv_b^T Jv_b + Jw_b^T I_b Jw_b from host kinematics (different formulation from the oracle's
    composite-rigid-body recursion)."""
    from real_robots_amd.model import load_model
    from tests.numpy_step import forward, mass_matrix_and_potential
    m = load_model()
    rng = np.random.default_rng(5)
    o = Oracle(1, 32, 32)
    for _ in range(3):
        q = rng.uniform(-1.5, 1.5, 11)
        set_q(o, q)
        M, bias = o.mass_matrix()
        Mref, _ = mass_matrix_and_potential(q)
        assert np.allclose(M, Mref, atol=1e-6)
        assert np.all(np.linalg.eigvalsh(M) > 0)
        # gravity torque = d(potential)/dq by finite differences
        def pot(qq):
            R2, p2, _ = forward(qq)
            return sum(m['body_mass'][b] * 9.81 * (p2[b] + R2[b] @ m['body_com'][b])[2] for b in range(11))
        g = np.array([(pot(q + 1e-6 * np.eye(11)[i]) - pot(q - 1e-6 * np.eye(11)[i])) / 2e-6 for i in range(11)])
        assert np.allclose(bias, g, atol=1e-4)   # qd = 0 -> bias is pure gravity


def test_f32_and_f64_oracle_agree_in_free_motion():
    a, b = Oracle(3, 32, 32), Oracle(3, 32, 32, f32=True)
    rng = np.random.default_rng(1)
    act = rng.uniform(-1, 1, 9)
    act[7:] = abs(act[7:])
    for t in range(200):
        a.step(act)
        b.step(act)
    d = np.abs(a.state - b.state)
    assert d[:22].max() < 1e-4                      # robot q, qd: free motion, rounding only
    for o3 in range(3):                             # resting objects: poses agree, velocities are contact jitter
        assert d[22 + 13 * o3: 29 + 13 * o3].max() < 1e-3
        assert d[29 + 13 * o3: 35 + 13 * o3].max() < 5e-2


def test_touch_sensor_fires_when_gripper_closes_on_cube():
    o = Oracle(1, 32, 32)
    for _ in range(100):
        o.step(None)
    # bring the gripper above the cube, open, descend, close (joint-space script)
    from oracle.kinematics import inverse_kinematics, quat_from_euler
    orient = quat_from_euler(0, 3.14, -1.57)
    def goto(z, grip, n):
        q = inverse_kinematics(o.state[:11], [-0.1, 0.0, z], orient)
        cmd = np.concatenate([q[:7], grip])
        mx = 0
        for _ in range(n):
            o.step(cmd)
            mx = max(mx, o.obs()[1].max())
        return mx
    goto(0.55, [0.5, 0.0], 150)
    assert goto(0.47, [0.5, 0.0], 150) == 0, "open gripper around the cube: no skin contact force"
    mx = goto(0.47, [0.0, 0.0], 150)
    assert mx > 1.0, "closing the gripper on the cube must register a touch force"
    goto(0.60, [0.0, 0.0], 200)
    assert o.obs()[2][0, 2] > 0.40, "the grasped cube is lifted with the gripper"
    assert o.obs()[1][[1, 3]].min() > 1.0      # both distal skins (skin_01, skin_11) keep pressing


def test_raster_properties():
    o = Oracle(3, 128, 128)
    for _ in range(100):
        o.step(None)
    rgb, depth, mask = o.render()
    ids, counts = np.unique(mask, return_counts=True)
    assert set(ids.tolist()) == {-1, 0, 1, 2, 3, 4}       # background, robot, table, cube, tomato, mustard
    assert (rgb[mask == -1] == 255).all() and (depth[mask == -1] == 1.0).all()
    # table top (z = 0.2794) seen from z = 1.2: GL depth of view distance ~0.9206
    n, f, w = 0.1, 100.0, 1.2 - (0.08 + 0.199403)
    d_expected = 0.5 * ((f + n) / (f - n) - 2 * f * n / ((f - n) * w)) + 0.5
    table_px = depth[(mask == 1)]
    assert abs(np.median(table_px) - d_expected) < 2e-4
    # image-right = world +y: mustard (y = +0.3) right of the cube, tomato (y = -0.3) left
    cx = lambda uid: np.argwhere(mask == uid)[:, 1].mean()
    assert cx(3) < cx(2) < cx(4)
    # robot base (x = -0.55) is at the top of the image (image-up = world -x)
    assert np.argwhere(mask == 0)[:, 0].mean() < np.argwhere(mask == 1)[:, 0].mean()


def test_render_resolution_320x240():
    o = Oracle(3, 320, 240)
    rgb, depth, mask = o.render()
    assert rgb.shape == (240, 320, 3) and depth.shape == (240, 320) and mask.shape == (240, 320)
    assert (mask == 1).sum() > 5000


def test_reference_macro_plan_tracking():
    """reference tests/test_actions.py:69-71,101-117,147-152: following the 1000-step macro plan, gripper `base` is
    within 0.01 m of (p1, 0.6) @199, (p1, 0.46) @249, (p2, 0.46) @749 and home @999 (objects parked on the shelf as
    the reference test does, test_actions.py:94-97). The reference also lists a checkpoint @849 that falls 50 steps
    into the home2 segment (raw_xy[849]); like the reference (which only prints "Failed!") it is not asserted.
    Perimeter points whose z = 0.6 way-point is out of reach with the gripper pointing down ((0.05, +-0.5)) are
    excluded."""
    from oracle.kinematics import generate_plan
    o = Oracle(1, 32, 32)
    home = np.array(GOLD['reference_known_answers']['home_base'])
    for p1, p2 in [((-0.25, -0.5), (0.05, 0.0)), ((0.05, 0.0), (-0.25, 0.5))]:
        o.reset()
        o.set_object_pose(0, [0.2, 0.0, 0.45, 0, 0, 0, 1])
        plan = generate_plan(o.state[:11], [p1, p2])
        assert plan.shape == (1000, 9)
        tg = {199: [p1[0], p1[1], 0.6], 249: [p1[0], p1[1], 0.46], 749: [p2[0], p2[1], 0.46], 999: home}
        for i in range(1000):
            o.step(plan[i])
            if i in tg:
                assert np.linalg.norm(o.link_pose('base')[:3] - tg[i]) < 0.01, (p1, p2, i)


def test_table_top_coverage_and_depth_match_analytic_ray_casting():
    """Known answer for the camera + rasteriser conventions (SURVEY 8c "raster of a single axis-aligned box"): the top
    face of the table (an axis-aligned rectangle at z = 0.279403) is ray-cast analytically in float64 with the OpenGL
    look-at / perspective matrices of env.py:136-141,253-255,518,548-551, the sample-point convention ndc_x = 2 col / W - 1,
    ndc_y = 2 (H - 1 - row) / H - 1, and GL depth 0.5 z_ndc + 0.5 (the matrices are tests/numpy_camera.py's, built from the
    camera frame and glFrustum).  Every pixel whose ray meets the rectangle's plane
    inside the strip -0.15 < x < 0.05 (clear of robot, shelf and the parked cube) must be table (mask 1) exactly when
    the hit lies inside the rectangle's y range, with the analytic depth to 1e-6."""
    W = H = 128
    o = Oracle(1, W, H)
    o.set_object_pose(0, [0.2, 0.0, 0.45, 0, 0, 0, 1])          # cube parked on the shelf side, outside the strip
    rgb, depth, mask = o.render()
    V, Pm = nc.eye_camera(W, H)                                  # the float64 ray caster's eye camera (tests/numpy_camera.py)
    inv = np.linalg.inv(Pm @ V)
    z_top, ylo, yhi = 0.279403, -0.505576, 0.495054
    checked = 0
    for row in range(H):
        for col in range(W):
            nd = np.array([2.0 * col / W - 1.0, 2.0 * (H - 1 - row) / H - 1.0])
            a = inv @ np.array([nd[0], nd[1], -1.0, 1.0]); b = inv @ np.array([nd[0], nd[1], 1.0, 1.0])
            a, b = a[:3] / a[3], b[:3] / b[3]
            lam = (z_top - a[2]) / (b[2] - a[2])
            hit = a + lam * (b - a)
            if not (-0.15 < hit[0] < 0.05) or min(abs(hit[1] - ylo), abs(hit[1] - yhi)) < 1e-4:
                continue
            inside = ylo < hit[1] < yhi
            assert (mask[row, col] == 1) == inside, (row, col, hit)
            if inside:
                c = Pm @ V @ np.append(hit, 1.0)
                assert abs(depth[row, col] - (0.5 * c[2] / c[3] + 0.5)) < 1e-6
                checked += 1
    assert checked > 1000


def test_sliding_friction_matches_coulomb_pyramid():
    """Known answer for the friction rows: a cube at rest on the table is given 0.4 m/s along world +y (a tangent
    direction of btPlaneSpace1 for an up-pointing normal).  While it slides, the deceleration must be mu g plus Bullet's
    linear damping v (0.04 + 0.04 |v|) with mu = friction(cube) x friction(table) = 0.5 x 1.0 (cube.urdf / table.urdf
    <lateral_friction>), and the cube must then stop and stay stopped (friction bounds +-mu lambda_n hold it)."""
    o = Oracle(1, 32, 32)
    for _ in range(300):
        o.step(None)
    st = o.state.copy()
    st[22 + 8] = 0.4                                   # object 0: pos3 quat4 lin3 ang3 -> lin.y
    o.state = st
    mu, g, dt = 0.5, 9.81, 0.005
    v_prev, sliding = 0.4, 0
    for k in range(40):
        o.step(None)
        v = o.state[22 + 8]
        if v > 0.02:
            a = (v_prev - v) / dt
            assert abs(a - (mu * g + v_prev * (0.04 + 0.04 * v_prev))) < 5e-3, (k, a)
            sliding += 1
        v_prev = v
    assert sliding >= 12 and abs(o.state[22 + 8]) < 1e-6 and abs(o.state[22 + 7]) < 1e-6     # stopped, no sideways drift
    assert abs(o.state[22 + 2] - st[22 + 2]) < 1e-4                                            # still resting on the table


def test_resting_contact_forces_carry_the_weight():
    """Static equilibrium known answer: for an object at rest on the table the normal forces reported by the contact list
    (Kuka.get_contacts column `normal force`, robot.py:131-150) sum to m g, with m from the object URDFs (cube 1.5 kg,
    tomato 3 kg, mustard 2 kg) -- pins the normal rows, ERP handling and the impulse -> force conversion."""
    o = Oracle(3, 32, 32)
    for _ in range(400):
        o.step(None)
    c = o.contacts()
    for ob, mass in enumerate((1.5, 3.0, 2.0)):
        sel = c[:, 0] == 16 + ob
        assert 3 <= sel.sum() <= 4 and (c[sel, 1] < 0).all()            # a 3-4 point manifold against a static body
        assert abs(c[sel, 10].sum() - mass * 9.81) < 2e-3 * mass * 9.81, (ob, c[sel, 10].sum())


def test_collision_hull_reduction_error():
    """Bullet collides the full convex hull of every OBJ; the compiled model keeps <= 192 vertices (an inner
    approximation) and <= 192 facet planes (an outer approximation) per shape.  The deviation of either from the full hull,
    recorded by tools/compile_model.py in the blob, must stay below 1 mm for every shape (0.3 mm for the shapes the task
    touches: objects, gripper, fingers, skins, table, shelf).  For the three objects the numbers are re-measured
    independently against the full hull vertex sets of the reference's OBJ files (tests/golden/full_hulls.npz, written by
    tools/compile_model.py with RR_FULL_HULLS_OUT): support functions of the full hull, of the vertex subset and (by linear
    programming) of the plane subset along 120 random directions."""
    import os
    from real_robots_amd.model import load_model
    m = load_model()
    dev, nv, nf = m['shape_dev'], m['shape_nv'], m['shape_nf']
    ns = int(m['dims'][2])
    assert dev.shape == (ns, 2) and (dev >= 0).all()
    assert dev.max() < 1.0e-3, dev.max()
    owner = m['shape_owner']
    arm = [s for s in range(ns) if owner[s][0] == 1 and 1 <= owner[s][2] <= 7] + [2]        # lbr_iiwa_link_1..7 and link_0
    task = [s for s in range(ns) if s not in arm]
    assert dev[task].max() < 3.1e-4, dev[task].max()
    assert nv.max() <= 192 and nf.max() <= 192 and int(m['dims'][8]) == 192 and int(m['dims'][9]) == 192
    from scipy.optimize import linprog
    rng = np.random.default_rng(0)
    D = rng.normal(size=(120, 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    hulls = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'full_hulls.npz'))
    names = [str(n) for n in hulls['names']]
    assert len(names) == ns

    # objects: the OBJ is used unscaled in the object frame (cube.urdf, tomato.urdf, mustard.urdf)
    for s, fn in zip(range(ns - 3, ns), ('cube', 'tomato', 'mustard')):
        assert names[s] == fn
        full = (hulls['hull_%d' % s].astype(np.float64) @ D.T).max(0)
        sub = (m['shape_verts'][s][:nv[s]] @ D.T).max(0)
        assert (full - sub).max() < 1.0e-3 and (full - sub).min() > -1e-6, (fn, (full - sub).max())
        pl = m['shape_planes'][s][:nf[s]].astype(np.float64)
        for d, f in zip(D[:40], full[:40]):
            r = linprog(-d, A_ub=pl[:, :3], b_ub=pl[:, 3], bounds=[(None, None)] * 3, method='highs')
            assert r.status == 0 and -1e-6 < -r.fun - f < 1.0e-3, (fn, -r.fun - f)


def test_resting_objects_come_to_complete_rest():
    """With the anchor of the contact manifold taken with a tolerance (reduce4) and the torsional friction rows of the
    URDFs' rolling / spinning coefficients (cube.urdf:6-7 1e-4, mustard.urdf:6-7 1e-2), the bevelled cube (88 hull vertices,
    a whole face within micrometres of the table) and the mustard bottle stop completely; the settle criterion of the
    reference's goal generator (generate_goals.py:46: position change < 1e-4, 20 consecutive steps) holds for all three."""
    o = Oracle(3, 32, 32)
    prev = None
    calm = 0
    for t in range(600):
        o.step(None)
        ob = o.state[22:].reshape(3, 13)
        if prev is not None:
            calm = calm + 1 if (np.abs(ob[:, :3] - prev[:, :3]).max() < 1e-4 and np.abs(ob[:, 3:7] - prev[:, 3:7]).max() < 1e-3) else 0
        prev = ob.copy()
    assert calm >= 300
    assert np.abs(ob[0, 7:]).max() < 1e-6 and np.abs(ob[2, 7:]).max() < 1e-6      # cube, mustard: all velocities
    assert np.abs(ob[1, 7:10]).max() < 2e-3 and np.abs(ob[1, 10:]).max() < 1e-2   # the 12-gon can keeps a residual creep
    assert np.abs(ob[0, 3:6]).max() < 1e-6                                        # the cube lies flat on its face


def test_torsional_friction_rows_match_an_independent_numpy_solver():
    from tests import numpy_step
    """Known answer for the rolling / spinning friction rows (tomato.urdf:6-7: 1e-3 each, table lateral friction 1.0 ->
    combined 1e-3): the tomato can lying on its side, rolling along the table, is stepped once by the oracle and by an
    independent numpy step (tests/numpy_step.py) over the oracle's own contact points.  Velocities must agree to 1e-8 (of 5.5 rad/s); the
    torsional impulses must be active (leaving the rows out changes the result by far more than the tolerance), and a
    rolling can must come to rest within a second."""
    o = Oracle(3, 32, 32)
    st = o.state.copy()
    st[22 + 13: 22 + 26] = [-0.1, -0.3, 0.2794 + 0.0362 + 0.0005, np.sin(np.pi / 4), 0, 0, np.cos(np.pi / 4), 0, 0, 0, 0, 0, 0]   # axis along world y
    o.state = st
    for _ in range(80):
        o.step(None)
    st = o.state.copy()
    assert abs(st[22 + 13 + 2] - (0.2794 + 0.0362)) < 2e-3            # lying on its side on the table
    st[22 + 13 + 7: 22 + 13 + 13] = [0.2, 0.0, 0.0, 0.0, 0.2 / 0.0362, 0.0]      # rolling without slipping along +x
    o.state = st
    full = st.copy()
    o.step(None)
    c = o.contacts()
    sel = c[c[:, 0] == 17]
    assert len(sel) >= 2 and (sel[:, 1] < 0).all()
    res = numpy_step.step(full, np.zeros(9), c)                        # (the whole step: tomato rows only couple to the tomato)
    v, w = res['state'][22 + 13 + 7: 22 + 13 + 10], res['state'][22 + 13 + 10: 22 + 26]
    assert np.allclose(res['mat'][c[:, 0] == 17], [0.5 * 1.0, 0.01 * 0.01, 1e-3, 1e-3], rtol=1e-6)    # mu, rest, roll, spin
    after = o.state[22 + 13: 22 + 26]
    assert np.abs(after[7:10] - v).max() < 1e-8 and np.abs(after[10:13] - w).max() < 1e-8
    lt = [lam for row, lam in zip(res['rows'], res['lam']) if row[0] == 'torsional' and c[row[1], 0] == 17]
    assert np.abs(lt).max() > 1e-6                                     # the torsional rows carry impulse here
    w0 = numpy_step.step(full, np.zeros(9), c, drop=('torsional',))['state'][22 + 13 + 10: 22 + 26]
    assert np.abs(w0 - w).max() > 1e-4
    for _ in range(200):
        o.step(None)
    assert np.abs(o.state[22 + 13 + 7: 22 + 26]).max() < 2e-2          # stopped rolling (it started at 5.5 rad/s; the 12-gon keeps a residual rocking)


def _edge_crossing_pose(gap=0.002, tilt_deg=-40.0):
    """Cube pose that puts one of its long edges across the shelf's front top edge (x = 0.079, z = 0.381, along y; shape
    `table_upper`), tilted so that both end points of the cube edge are outside the shelf's margin zone: returns (pose7,
    expected normal shelf -> cube, expected contact point)."""
    from oracle.kinematics import quat_from_euler
    from real_robots_amd.model import load_model
    m = load_model()
    cube = int(m['dims'][2]) - 3                                                    # the objects are the last three shapes
    E = m['shape_edges'][cube][:m['shape_ne'][cube]].astype(np.float64)             # the cube's long edges (owner frame)
    k = [i for i in range(len(E)) if abs(E[i, 3]) > 0.05 and E[i, 7] < 0 and E[i, 8] < 0 and E[i, 10] < 0 and E[i, 11] < 0][0]
    q = np.array(quat_from_euler(np.radians(45.0), np.radians(tilt_deg), 0.0))     # roll 45: that edge is the lowest one; then tilt
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    mid = R @ (E[k, :3] + 0.5 * E[k, 3:6])
    d1 = R @ E[k, 3:6]
    n = np.cross(d1, [0.0, 1.0, 0.0]); n /= np.linalg.norm(n)
    if n[2] < 0:
        n = -n
    on_shelf_edge = np.array([0.079, 0.02, 0.381])
    pos = on_shelf_edge + gap * n - mid
    return np.concatenate([pos, q]), n, on_shelf_edge + 0.5 * gap * n


def test_edge_edge_contact_known_answer():
    """Two edges crossing away from any vertex: a tilted cube edge 2 mm above the shelf's front edge.
    The vertex tests only see speculative candidates more than a centimetre away, and the edges pass through each other; the
    edge pass adds the contact at the crossing point, along the common normal of the two edges, and it stops the cube."""
    pose, n_exp, x_exp = _edge_crossing_pose()
    res = {}
    for edges in (0, 1):
        o = Oracle(1, 32, 32, edge_contacts=edges)
        o.reset()
        o.set_object_pose(0, pose)
        s = o.state
        s[22 + 7:22 + 10] = -1.0 * n_exp          # approaching along the normal at 1 m/s
        o.state = s
        o.step(None)
        res[edges] = (o.contacts(), o.state[22 + 7:22 + 10] @ n_exp)
    c0, c1 = res[0][0], res[1][0]
    # vertex tests alone (since round 5 the shelf's rim carries sample points every 2 cm, tools/compile_model.py): the nearest candidate
    # is a rim sample 3.5 mm from a cube FACE -- with that face's normal, 30 degrees off the edges' common normal -- not the crossing
    assert (c0[:, 9] > 0.003).all() and res[0][1] < -0.7
    assert np.degrees(np.arccos(np.clip(c0[np.argmin(c0[:, 9]), 6:9] @ n_exp, -1, 1))) > 20.0
    # with the edge pass the crossing itself is the pair's deepest contact; the other points of the manifold are unchanged
    assert len(c1) == len(c0) and (c1[1:] == c0[1:]).all()
    e = c1[int(np.argmin(c1[:, 9]))]
    assert e[0] == 16 and e[1] == -1
    # (the shelf's vertices are float32 in the model blob and the expected numbers use the rounded 0.079 / 0.381)
    assert np.abs(e[6:9] - n_exp).max() < 1e-3 and abs(e[9] - 0.002) < 2e-4 and np.abs(e[3:6] - x_exp).max() < 5e-4
    assert res[1][1] > -0.45          # speculative contact: the approach speed is cut to distance / dt = 0.4 m/s


def test_warm_starting_carries_the_normal_impulses_over():
    """Warm starting (Bullet: persistent manifolds + m_warmstartingFactor 0.85): the normal impulse of a
    contact starts from 0.85 x the impulse of the previous step's contact it is matched to.  With a single solver iteration
    per step a cold start cannot hold three resting objects (they sink by more than a millimetre); the warm start converges
    over the steps.  At the default 50 iterations both rest, the warm start with a quarter of the residual velocity."""
    res = {}
    for iters in (1, 50):
        for ws in (0.0, 0.85):
            o = Oracle(3, 32, 32, solver_iters=iters, warmstart=ws)
            o.reset()
            for _ in range(300):
                o.step(None)
            c = o.contacts()
            c = c[c[:, 0] >= 16]
            res[iters, ws] = (c[:, 9].min(), np.abs(o.state[22:].reshape(3, 13)[:, 7:]).max(),
                              [c[c[:, 0] == 16 + i, 10].sum() for i in range(3)])
    assert res[1, 0.0][0] < -1.0e-3 and res[1, 0.85][0] > -5.0e-4
    assert res[50, 0.85][1] < 0.5 * res[50, 0.0][1] and res[50, 0.85][1] < 5e-4
    m = np.array([1.5, 3.0, 2.0]) * 9.81           # weights of cube, tomato, mustard (obj_mass)
    assert np.abs(np.array(res[50, 0.85][2]) - m).max() < 0.02 * m.max()
    # a state set from outside has no history; handing the contact list over restores it
    a, b = Oracle(1, 32, 32, solver_iters=2), Oracle(1, 32, 32, solver_iters=2)          # (few iterations: the start matters)
    for _ in range(60):
        a.step(None)
    b.state = a.state
    b.set_contact_cache(a.contacts())
    a.step(None); b.step(None)
    assert np.abs(a.state - b.state).max() < 1e-12
    b.state = a.state                               # cold
    a.step(None); b.step(None)
    assert np.abs(a.state - b.state).max() > 1e-9


def test_reference_macro_script_all_36_pairs_at_the_reference_tolerance():
    """reference tests/test_actions.py:62-71,101-117,147-152: ALL 36 ordered pairs of the six perimeter points, objects parked on
    the shelf (test_actions.py:95-98), gripper `base` against the script's way points at t = 199, 249, 749, 999 with the script's
    own 0.01 m -- asserted wherever the documented motor model (kp 0.1, 10 % of the command error per step, behind the rate limit
    of env.py:314-321) reaches it, with the exact residual recorded where it does not:
      * t = 249, (p1, 0.46): all 36 (worst 9.75 mm: the arm is still closing the last millimetres of the 14 cm descent);
      * t = 999, home: all 36 (1.0 mm);
      * t = 749, (p2, 0.46): 35 of 36; ((0.05, 0.5) -> (-0.25, -0.5)) is 16.9 mm off: the longest sweep of the script, 500 steps
        are not enough at 0.02-0.03 rad per step;
      * t = 199, (p1, 0.6): the 18 pairs whose p1 is (-0.25, +-0.5) or (0.05, 0); p1 = (-0.25, 0) misses by 0.2 mm (10.2 mm: 1.8 rad
        of joint travel from home2 in 100 steps), the corners (0.05, -0.5) / (0.05, 0.5) by 61.6 / 21.4 mm (reach limit: the IK has
        no exact solution there, under every motor variant of tests/golden/macro_sensitivity.json).
    t = 849 is the open question of DESIGN.md 2 (out of reach under the documented model) and is only compared with the fixture.
    The run must also reproduce the committed sensitivity fixture (same plans, same oracle) to 1e-6 m."""
    import json
    from oracle.kinematics import generate_plan
    fx = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'macro_sensitivity.json')))
    pairs = [tuple(map(tuple, p)) for p in fx['pairs']]
    assert len(pairs) == 36
    fixture = np.array(fx['distance_m']['kp=0.1,rate_limit=on'])
    home, home2 = np.array([-0.55, 0.0, 1.27]), np.array([-0.419, 0.0, 1.14])
    got = np.zeros((36, 5))
    for i, (p1, p2) in enumerate(pairs):
        o = Oracle(3, 64, 64)
        o.reset()
        for k, p in enumerate([[0.2, 0.0, 0.75], [0.2, -0.3, 0.75], [0.2, 0.3, 0.75]]):
            o.set_object_pose(k, np.array(p + [0, 0, 0, 1.0]))
        plan = generate_plan(np.zeros(11), [p1, p2])
        tg = {199: [p1[0], p1[1], 0.6], 249: [p1[0], p1[1], 0.46], 749: [p2[0], p2[1], 0.46], 849: home2, 999: home}
        for t in range(1000):
            o.step(plan[t])
            if t in tg:
                got[i, fx['check_steps'].index(t)] = np.linalg.norm(o.link_pose('base')[:3] - tg[t])
    assert np.abs(got - fixture).max() < 2e-5, np.abs(got - fixture).max()       # (the fixture is rounded to 1e-5)
    tol = fx['tolerance_of_the_reference_script_m']
    assert tol == 0.01
    c199, c249, c749, c999 = got[:, 0], got[:, 1], got[:, 2], got[:, 4]
    assert (c249 < tol).all() and c249.max() < 0.0098
    assert (c999 < tol).all() and c999.max() < 0.0011
    over749 = [i for i in range(36) if c749[i] >= tol]
    assert over749 == [30] and pairs[30] == ((0.05, 0.5), (-0.25, -0.5)) and c749[30] < 0.0170
    reach199 = [i for i in range(36) if pairs[i][0] in ((-0.25, -0.5), (-0.25, 0.5), (0.05, 0.0))]
    assert len(reach199) == 18 and (c199[reach199] < tol).all()
    for i in range(36):
        p1 = pairs[i][0]
        if p1 == (-0.25, 0.0):
            assert 0.0100 <= c199[i] < 0.0103, (i, c199[i])
        elif p1 == (0.05, -0.5):
            assert c199[i] < 0.0617
        elif p1 == (0.05, 0.5):
            assert c199[i] < 0.0215
