"""The float64 reference of the step's joint torque inputs (tests/numpy_torque.py) on its own: the wrapper, the free-arm rollout and
the hold condition the GPU test (tests/test_gpu_joint_torques.py) puts to the device.  No GPU."""
import numpy as np

from tests import numpy_actuators as na
from tests import numpy_dynamics as nd
from tests import numpy_step as ns
from tests import numpy_torque as nt

Q0 = nt.HOLD_POSTURES


def _state(q, qd=None, seed=0):
    """A 61-entry state: joints (q, qd), the objects at the model's start poses with some velocity."""
    rng = np.random.default_rng(seed)
    s = np.zeros(61)
    s[:11], s[11:22] = q, (np.zeros(11) if qd is None else qd)
    ob = np.zeros((3, 13))
    ob[:, :7] = ns.model()['obj_pose0'][:3]
    ob[:, 7:] = rng.normal(0, 0.3, (3, 6))
    s[22:] = ob.reshape(-1)
    return s


def test_wrapper_changes_qds_by_the_closed_form_and_nothing_else():
    rng = np.random.default_rng(1)
    st = np.stack([_state(q, rng.normal(0, 2.0, 11), k) for k, q in enumerate(Q0)])
    dyn = np.broadcast_to(ns.default_dynamics(), (3, 3, 8))
    tau = rng.uniform(-200, 200, (3, 11))
    tau[1] = 0.0                                   # a zero row inside a non-zero table
    prep0 = ns.prep
    base = ns.prep(st, dyn)
    with nt.applied(tau):
        assert ns.prep is not prep0
        got = ns.prep(st, dyn)
    assert ns.prep is prep0 and na.unconstrained_velocities.__module__ == na.__name__      # both put back
    assert set(got) == set(base)
    for k in base:
        if k != 'qds':
            assert np.array_equal(got[k], base[k]), k
    want = base['qds'] + ns.DT * np.einsum('nij,nj->ni', base['Minv'], tau)
    assert np.array_equal(got['qds'], want)
    assert np.array_equal(got['qds'][1], base['qds'][1]) and np.abs(got['qds'][0] - base['qds'][0]).max() > 1e-3
    # the controls' terms: -tau, and M in the place of M^-1
    with nt.applied(tau, 'negated'):
        neg = ns.prep(st, dyn)['qds']
    assert np.allclose(neg - base['qds'], -(want - base['qds']), rtol=0, atol=1e-12)
    with nt.applied(tau, 'mass'):
        mass = ns.prep(st, dyn)['qds']
    assert np.array_equal(mass, base['qds'] + ns.DT * np.einsum('nij,nj->ni', base['M'], tau))
    # put back after an exception too
    try:
        with nt.applied(tau):
            raise RuntimeError
    except RuntimeError:
        pass
    assert ns.prep is prep0


def test_zero_torque_returns_preps_own_arrays():
    st, dyn = _state(Q0[0], np.ones(11)), ns.default_dynamics()
    seen = []
    prep0 = ns.prep

    def spy(*a, **k):
        seen.append(prep0(*a, **k))
        return seen[-1]
    ns.prep = spy
    try:
        with nt.applied(np.zeros(11)):
            got = ns.prep(st, dyn)
        with nt.applied(-np.zeros((1, 11))):        # negative zeros are zeros
            got2 = ns.prep(st, dyn)
    finally:
        ns.prep = prep0
    assert got is seen[0] and got2 is seen[1]
    for k in got:
        assert got[k] is seen[0][k]


def test_numpy_step_with_no_robot_rows_is_the_free_arm_step():
    """What the rollout relies on: motors off, no joint within the limit window, no robot contact -> numpy_step.step leaves the
    joints at (q + dt qd*', qd*'), exactly; the per-joint step of tests/numpy_actuators.py too."""
    rng = np.random.default_rng(2)
    lim = ns.model()['body_limits']
    for k, q in enumerate(Q0):
        for j in range(11):
            if lim[j][0] < lim[j][1]:
                assert min(q[j] - lim[j][0], lim[j][1] - q[j]) >= ns.LIMIT_WINDOW
        qd = rng.normal(0, 1.0, 11)
        tau = rng.uniform(-100, 100, 11)
        st = _state(q, qd, k)
        with nt.applied(tau):
            r = ns.step(st, np.zeros(9), np.zeros((0, 12)), solver={'motor_max_force': 0.0})
            ra = na.step(st, np.zeros(9), np.zeros((0, 12)), max_force=0.0)
        assert not any(row[0] == 'limit' for row in r['rows']) and not r['lam'].any()
        q1, qd1 = nt.free_arm_step(q, qd, tau)
        assert np.array_equal(r['state'][:11], q1) and np.array_equal(r['state'][11:22], qd1)
        assert np.array_equal(ra['state'][:22], r['state'][:22])
        # ... and with the motors on the torque is feed-forward under the position motor: the motor rows take it up
        with nt.applied(tau):
            rm = ns.step(st, np.zeros(9), np.zeros((0, 12)))
        assert np.abs(rm['state'][11:22] - qd1).max() > 1e-3


def test_free_arm_holds_under_the_float64_bias():
    """tau = the float64 bias of tests/numpy_dynamics.reference at the present (q, qd), zero joint damping: q stays to rounding."""
    z = np.zeros(11)
    qs = nt.free_arm_rollout(Q0, nt.HOLD_STEPS, lambda q, qd: nd.reference(q, qd, inverse=False)['bias'], damping=z)
    print("float64 bias: drift", nt.drift(qs))
    assert nt.drift(qs).max() < 1e-12
    # with the model's joint damping and the arm at rest the hold is as good (the damping term vanishes with qd)
    qs = nt.free_arm_rollout(Q0, 5, lambda q, qd: nd.reference(q, qd, inverse=False)['bias'])
    assert nt.drift(qs).max() < 1e-12


def test_hold_condition_on_the_reference():
    """The GPU test's condition on the reference alone: over HOLD_STEPS = 50 steps from the three postures at rest the drift with
    tau = the float32-rounded bias is at most HOLD_RATIO = 0.05 of the drift with tau = 0 -- with a factor of 3 to spare (measured:
    ratios of 1e-7 to 4e-7; the arm falls by 0.6 to 0.9 rad in its most mobile joint without torques)."""
    z = np.zeros(11)
    held = nt.drift(nt.free_arm_rollout(Q0, nt.HOLD_STEPS, nt.float32_bias, damping=z))
    free = nt.drift(nt.free_arm_rollout(Q0, nt.HOLD_STEPS, lambda q, qd: np.zeros_like(q), damping=z))
    print("drift held", held, "free", free, "ratio", held / free)
    assert (free > 0.1).all()
    assert (3.0 * held <= nt.HOLD_RATIO * free).all()


def test_qds_ceiling_takes_the_torque_into_its_bias_term():
    st = np.stack([_state(q, np.ones(11)) for q in Q0])
    pr = ns.prep(st, np.broadcast_to(ns.default_dynamics(), (3, 3, 8)))
    c0 = nt.qds_ceiling(pr, st[:, 11:22], np.zeros((3, 11)))
    bterm = np.abs(ns.DT * np.einsum('nij,nj->ni', pr['Minv'], pr['bias'])).max(1, keepdims=True)
    assert np.allclose(c0, 2e-4 + 2e-6 * 1.0 + 5e-5 * bterm, rtol=1e-12)
    # tau = bias: the term vanishes
    assert np.allclose(nt.qds_ceiling(pr, st[:, 11:22], pr['bias']), 2e-4 + 2e-6, rtol=1e-12)
