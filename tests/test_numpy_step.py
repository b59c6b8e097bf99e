"""CPU tests (-m "not gpu"): the float64 oracle against an independent float64 numpy restatement of the step (tests/numpy_step.py).

The oracle is the reference every GPU test of the step compares with; here it meets a computation that shares nothing with it
but the model data and Bullet's documented semantics: the joint-space bias from the Lagrangian by complex step, contact
Jacobians by complex-step kinematics, rows as dense Jacobians over generalised velocities, materials combined from the
shapes' own values.  Both start from the same state and contact history; the oracle's records give the contact points,
normals and distances, everything else the numpy step derives itself.
"""
import numpy as np
import pytest

import oracle.oracle as oracle_mod
from oracle.kinematics import inverse_kinematics, quat_from_euler
from oracle.oracle import Oracle, params_from_solver
from tests import numpy_step as ns
from tests.test_gpu_object_dynamics import patched_blob

TOL_V = 1e-8           # post-step velocities (rad/s, m/s)
TOL_P = 1e-10          # post-step poses
CONTROL = 1e3          # a negative control must move the result by this many tolerances at least
CRUSH_OK = 1e5         # N: in float64 the tolerances hold far above CRUSH_FORCE (2 kN, tests/test_gpu_contacts_fuzz.py) -- the grasp,
                       # the press and the pile reach 3-25 kN

ORIENT = quat_from_euler(0, 3.14, -1.57)


def _goto(o, xyz, grip, n):
    q = inverse_kinematics(o.state[:11], xyz, ORIENT)
    cmd = np.concatenate([q[:7], grip])
    for _ in range(n):
        o.step(cmd)
    return cmd


def _scene_grasp(nobj=3):
    """1: the gripper closed on the cube, lifting it."""
    o = Oracle(nobj, 32, 32)
    for _ in range(100):
        o.step(None)
    _goto(o, [-0.1, 0, 0.55], [0.5, 0], 150)
    _goto(o, [-0.1, 0, 0.47], [0.5, 0], 150)
    _goto(o, [-0.1, 0, 0.47], [0, 0], 150)
    return o, _goto(o, [-0.1, 0, 0.5], [0, 0], 30)


def _scene_press():
    """2: the closed gripper pressing the cube into the table."""
    o, _ = _scene_grasp()
    return o, _goto(o, [-0.1, 0, 0.42], [0, 0], 40)


def _scene_pile():
    """3: the cube lying on the mustard bottle, a finger pressing on both."""
    o = Oracle(3, 32, 32)
    o.set_object_pose(0, [-0.1, 0.3, 0.55, 0, 0, 0, 1])
    for _ in range(150):
        o.step(None)
    _goto(o, [-0.1, 0.3, 0.6], [0, 0], 120)
    return o, _goto(o, [-0.1, 0.3, 0.47], [0, 0], 60)


def _scene_limit():
    """4: joint 2 driven past its upper limit, joint 4 racing into its lower one, elbow up (no contact of the arm)."""
    o = Oracle(3, 32, 32)
    for _ in range(60):
        o.step(None)
    st = o.state.copy()
    lim = ns.model()['body_limits']
    st[1], st[12] = -lim[1][1] + 0.3, 0.0
    st[3], st[14] = lim[3][0] + 0.05, -25.0
    st[5], st[16] = lim[5][1] - 0.01, 6.0
    prev = o.contacts()
    o.state = st
    o.set_contact_cache(prev)
    cmd = np.concatenate([st[:7], [0.0, 0.0]])
    cmd[5] += 0.3
    return o, cmd


def _scene_free():
    """5: the arm swinging fast in free space; the objects in flight, spinning (anisotropic tomato and mustard: gyroscopic)."""
    o = Oracle(3, 32, 32)
    rng = np.random.default_rng(11)
    st = o.state.copy()
    st[:11] = [0.3, -0.4, 0.2, 0.6, -0.3, 0.5, 0.1, 0.3, -0.2, 0.3, -0.2]
    st[11:22] = rng.uniform(-40, 40, 11)
    for i, (p, v, w) in enumerate((([-0.2, -0.3, 0.8], [0.3, 0.1, 1.0], [12.0, -30.0, 8.0]),
                                   ([-0.1, 0.0, 0.9], [-0.2, 0.4, 0.0], [25.0, 10.0, -35.0]),
                                   ([0.0, 0.3, 0.75], [0.1, -0.3, 2.0], [-18.0, 22.0, 40.0]))):
        q = rng.normal(size=4)
        st[22 + 13 * i: 35 + 13 * i] = np.concatenate([p, q / np.linalg.norm(q), v, w])
    o.state = st
    return o, rng.uniform(-1, 1, 9) * [1, 1, 1, 1, 1, 1, 1, 0, 0] + [0, 0, 0, 0, 0, 0, 0, 0.4, 0.3]


def _scene_grasp1():
    """6: scene 1 with the cube alone (one object: no object x object pair, and the lifted cube touches nothing static)."""
    return _scene_grasp(1)


def _scene_pile2():
    """7: two objects: the tomato dropped onto the cube, then a finger pressing it down against the cube's side."""
    o = Oracle(2, 32, 32)
    o.set_object_pose(1, [-0.1, 0.0, 0.40, 0, 0, 0, 1])
    o.set_object_pose(0, [-0.1, 0.0, 0.32, 0, 0, 0, 1])
    for _ in range(150):
        o.step(None)
    _goto(o, [-0.1, 0.0, 0.6], [0, 0], 120)
    return o, _goto(o, [-0.1, 0.0, 0.52], [0, 0], 60)


SCENES = {'grasp': _scene_grasp, 'press': _scene_press, 'pile': _scene_pile, 'limit': _scene_limit, 'free': _scene_free,
          'grasp1': _scene_grasp1, 'pile2': _scene_pile2}
NOBJ = {'grasp1': 1, 'pile2': 2}          # objects of a scene (the others: 3)
_cache = {}


def scene(name):
    """(state, contact history, action) of a scene, built once."""
    if name not in _cache:
        o, cmd = SCENES[name]()
        assert o.n_objects == NOBJ.get(name, 3)
        _cache[name] = (o.state.copy(), o.contacts(), np.asarray(cmd, dtype=np.float64))
    return _cache[name]


def variants():
    d = ns.default_dynamics().astype(np.float32)
    heavy = d.copy()
    heavy[0, 0], heavy[0, 1:4] = 7.5, [0.004, 0.012, 0.0075]          # a heavy anisotropic cube
    low = d.copy()
    low[:, 4] = 0.1
    bouncy = d.copy()
    bouncy[:, 5], bouncy[:, 6], bouncy[:, 7] = 0.8, 0.05, 0.05
    solver = dict(motor_kp=0.2, motor_kd=0.6, motor_max_force=300.0, warmstart=0.5, lin_damping=0.1, ang_damping=0.2, erp=0.35,
                  rate_limit=False)
    return {'default': (d, None, 50), 'heavy_aniso': (heavy, None, 50), 'low_friction': (low, None, 50),
            'bouncy_rolling': (bouncy, None, 50), 'solver': (d, solver, 50), 'iters1': (d, None, 1)}


VARIANTS = variants()


def oracle_step(monkeypatch, name, variant):
    """The float64 oracle on the variant's patched model: one step from the scene -> (post-step state, contact records).  (The
    variants' rows are [3, 8]; a scene with fewer objects uses the leading ones.)"""
    dyn, solver, iters = VARIANTS[variant]
    st, prev, cmd = scene(name)
    with monkeypatch.context() as m:
        m.setattr(oracle_mod, 'model_blob', lambda b=patched_blob(dyn): b)
        o = Oracle(NOBJ.get(name, 3), 32, 32, solver_iters=iters, **params_from_solver(solver))
    o.state = st
    o.set_contact_cache(prev)
    o.step(cmd)
    return o.state.copy(), o.contacts()


def numpy_step(name, variant, contacts, dyn=None, **kw):
    drow, solver, iters = VARIANTS[variant]
    st, prev, cmd = scene(name)
    k = NOBJ.get(name, 3)
    dyn = drow if dyn is None else dyn
    return ns.step(st, cmd, contacts, dyn=dyn[:k].astype(np.float64), prev=prev, solver=solver, solver_iters=iters, nobj=k, **kw)


def deviation(a, b):
    """(worst velocity difference, worst pose difference) of two 61-states (every object slot: an absent object's must pass
    through unchanged on both sides)."""
    d = np.abs(np.asarray(a) - np.asarray(b))
    v = np.concatenate([d[11:22], d[22:].reshape(3, 13)[:, 7:].ravel()])
    p = np.concatenate([d[:11], d[22:].reshape(3, 13)[:, :7].ravel()])
    return float(v.max()), float(p.max())


def kinds(res, contacts):
    """What the step's problem holds: active row kinds and the contact pairs that carry impulse."""
    act = {k for (k, *_), lam in zip(res['rows'], res['lam']) if abs(lam) > 1e-9}
    cls = lambda b: 'object' if b >= 16 else 'robot' if b >= 0 else 'static'
    pairs = {(cls(int(c[0])), cls(int(c[1]))) for c, l in zip(contacts, res['lambda_n']) if l > 1e-9}
    return act, pairs


EXPECT = {'grasp': {('robot', 'object'), ('object', 'static')}, 'press': {('robot', 'object'), ('object', 'static')},
          'pile': {('robot', 'object'), ('object', 'object'), ('object', 'static')}, 'limit': set(), 'free': set(),
          'grasp1': {('robot', 'object')}, 'pile2': {('robot', 'object'), ('object', 'object'), ('object', 'static')}}


def test_fk_matches_urdf_fixture():
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fk_golden.json')))
    from oracle.oracle import LINK_NAMES
    for case in gold['cases']:
        cmd = np.array(case['cmd'])
        q = np.concatenate([cmd[:7], [cmd[7], -cmd[8], cmd[7], -cmd[8]]])
        for link, pos in case['links'].items():
            _, p = ns.link_pose(q, LINK_NAMES.index(link))
            assert np.allclose(p, pos, atol=2e-6), (link, p, pos)


def _postures(rng):
    lim = ns.model()['body_limits']
    out = [rng.uniform(np.minimum(lim[:, 0], lim[:, 1]), np.maximum(lim[:, 0], lim[:, 1])) for _ in range(4)]
    straight = np.zeros(11)                       # elbow straight, every wrist axis aligned with the arm
    wrist = rng.uniform(-1, 1, 11)
    wrist[5] = 0.0                                # wrist axes 5 and 7 aligned
    wrist[3] = 1e-9                               # elbow straight
    return out + [straight, wrist]


def test_bias_and_inverse_mass_against_the_oracle():
    """M, the bias b(q, qd) with qd up to 40 rad/s and M^-1 of the oracle's recursive Newton-Euler pass against the Lagrangian
    by complex step, at random and near-singular postures."""
    rng = np.random.default_rng(4)
    o = Oracle(1, 32, 32)
    worst = [0.0, 0.0, 0.0]
    for q in _postures(rng):
        for qd in (np.zeros(11), rng.uniform(-40, 40, 11), np.full(11, 40.0)):
            s = o.state
            s[:11], s[11:22] = q, qd
            o.state = s
            M, b = o.mass_matrix()
            pr = ns.prep(s, ns.default_dynamics(1), nobj=1)
            Minv = np.linalg.inv(M)
            e = (np.abs(pr['M'] - M).max() / np.abs(M).max(), np.abs(pr['bias'] - b).max() / max(1.0, np.abs(b).max()),
                 np.abs(pr['Minv'] - Minv).max() / np.abs(Minv).max())
            worst = [max(a, c) for a, c in zip(worst, e)]
            assert e[0] < 1e-12 and e[1] < 1e-11 and e[2] < 1e-9, (q, qd, e)
            if qd.any():             # the velocity terms are there: leaving them out moves b by far more
                assert np.abs(ns.bias(q, qd, coriolis=False) - b).max() > 1e3 * e[1] * max(1.0, np.abs(b).max())
    print("numpy vs oracle: M %.1e, b %.1e, M^-1 %.1e (relative)" % tuple(worst))


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', list(SCENES))
def test_one_step_matches_the_numpy_step(monkeypatch, name, variant):
    st1, co = oracle_step(monkeypatch, name, variant)
    res = numpy_step(name, variant, co)
    dv, dp = deviation(res['state'], st1)
    fmax = float(co[:, 10].max()) if len(co) else 0.0
    print("%s/%s: %d contacts, %d rows, fmax %.0f N: |dv| %.1e |dpose| %.1e" % (name, variant, len(co), len(res['rows']), fmax, dv, dp))
    assert fmax < CRUSH_OK
    assert dv < TOL_V and dp < TOL_P, (dv, dp)
    assert np.allclose(res['lambda_n'], co[:, 10] * ns.DT, rtol=1e-9, atol=1e-9)
    assert np.array_equal(res['mat'][:, 0], co[:, 11])              # mu: the same products of the same float32 inputs
    act, pairs = kinds(res, co)
    assert EXPECT[name] <= pairs, pairs
    k = NOBJ.get(name, 3)
    assert np.array_equal(res['state'][22 + 13 * k:], scene(name)[0][22 + 13 * k:])      # absent objects' slots: untouched
    if name in ('grasp', 'grasp1'):                                  # both finger links carry impulse
        fingers = {int(c[0]) for c, l in zip(co, res['lambda_n']) if l > 1e-9 and 0 <= c[0] < 16}
        assert {7, 8} & fingers and {9, 10} & fingers, fingers
    if name == 'limit':
        assert 'limit' in act and not any(0 <= c[0] < 16 for c in co)
    if name == 'free':
        assert not any(0 <= c[0] < 16 for c in co) and not len(co)
    if name in ('grasp', 'press', 'pile', 'grasp1', 'pile2') and variant != 'iters1':
        assert {'normal', 'friction', 'torsional'} <= act, act


def test_negative_controls_move_the_result():
    """Each of these slips moves the numpy step far from the oracle: the check above can see them (with one, two and three
    objects)."""
    mp = pytest.MonkeyPatch()
    ratios = {}
    try:
        st1, co = oracle_step(mp, 'free', 'default')
        ratios['free/coriolis'] = deviation(numpy_step('free', 'default', co, drop=('coriolis',))['state'], st1)[0] / TOL_V
        ratios['free/gyroscopic'] = deviation(numpy_step('free', 'default', co, drop=('gyroscopic',))['state'], st1)[0] / TOL_V
        for name in ('grasp', 'pile', 'grasp1', 'pile2'):
            st1, co = oracle_step(mp, name, 'heavy_aniso')
            rolled = np.roll(VARIANTS['heavy_aniso'][0], 1, axis=0)          # a neighbour's row (one object: the mustard's)
            ratios[name + '/neighbour row'] = deviation(numpy_step(name, 'heavy_aniso', co, dyn=rolled)['state'], st1)[0] / TOL_V
            st1, co = oracle_step(mp, name, 'iters1')
            ratios[name + '/reversed normals'] = deviation(numpy_step(name, 'iters1', co, drop=('reverse_normals',))['state'], st1)[0] / TOL_V
            st1, co = oracle_step(mp, name, 'default')
            ratios[name + '/torsional'] = deviation(numpy_step(name, 'default', co, drop=('torsional',))['state'], st1)[0] / TOL_V
    finally:
        mp.undo()
    print("negative controls, worst |dv| / TOL_V: " + ', '.join('%s %.1e' % kv for kv in ratios.items()))
    assert min(ratios.values()) > CONTROL, ratios


def test_warm_start_pairs_with_the_previous_step():
    """The warm start matters in these scenes (one sweep: the start is most of the answer) and the numpy matching reproduces it:
    a cold numpy step is far from the oracle's warm one."""
    mp = pytest.MonkeyPatch()
    try:
        for name in ('grasp', 'pile'):
            st1, co = oracle_step(mp, name, 'iters1')
            dyn, solver, iters = VARIANTS['iters1']
            s, prev, cmd = scene(name)
            cold = ns.step(s, cmd, co, dyn=dyn.astype(np.float64), prev=None, solver_iters=1)
            assert deviation(cold['state'], st1)[0] > CONTROL * TOL_V
            assert (ns.warm_start(co, prev, 0.85) > 0).sum() >= 5
    finally:
        mp.undo()
