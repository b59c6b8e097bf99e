"""The float64 reference of the step's external wrenches (tests/numpy_wrench.py) on its own: the generalised force against the
derivative of the work, the wrapper, and the negative controls on the inputs the GPU test (tests/test_gpu_external_wrenches.py) puts
to the device.  No GPU."""
import os

import numpy as np
import pytest

from tests import numpy_actuators as na
from tests import numpy_step as ns
from tests import numpy_torque as nt
from tests import numpy_wrench as nw

NB = ns.NB
# edge_states(21, 3) of tests/test_gpu_numpy_step.py as recorded (tests/test_gpu_round6.py describes the file): the GPU test's states
# need a device to be drawn; its first five are the GPU test's N = 5 inputs
STATES = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prep_thread_per_env.npz'))['state']


def _centres(q):
    R, p, _ = ns.forward(q)
    return p + np.einsum('...bij,bj->...bi', R, ns.model()['body_com']), R


def test_generalised_force_is_the_derivative_of_the_work():
    """tau_k = d/dq_k sum_b F_b . c_b(q) for forces (central difference over q), and for torques the rate of the bodies' rotations:
    sum_b T_b . omega_b with omega_b = vee(dR_b/dq_k R_b^T)."""
    rng = np.random.default_rng(4)
    h = 1e-6
    for q in np.concatenate([nt.HOLD_POSTURES, rng.uniform(-1.5, 1.5, (3, NB))]):
        w = rng.normal(0, 20.0, (14, 6))
        R, p, ax = ns.forward(q)
        pr = dict(R=R, p=p, axis=ax)
        tau = nw.generalised_force(pr, w)
        num = np.zeros(NB)
        for k in range(NB):
            e = np.zeros(NB)
            e[k] = h
            (cp, Rp), (cm, Rm) = _centres(q + e), _centres(q - e)
            dR = np.einsum('bij,bkj->bik', (Rp - Rm) / (2 * h), R)                      # [omega]x per body
            omega = np.stack([dR[:, 2, 1], dR[:, 0, 2], dR[:, 1, 0]], -1)
            num[k] = (w[:NB, :3] * (cp - cm) / (2 * h)).sum() + (w[:NB, 3:] * omega).sum()
        assert np.abs(tau - num).max() < 1e-6 * (1 + np.abs(tau).max()), (tau, num)
        # the object rows play no part in it
        w2 = w.copy()
        w2[NB:] = 0.0
        assert np.array_equal(nw.generalised_force(pr, w2), tau)
        # a wrench on the last finger body alone reaches exactly the joints of its root path
        w3 = np.zeros((14, 6))
        w3[10] = [3.0, -2.0, 5.0, 0.3, 0.2, -0.4]
        t3 = nw.generalised_force(pr, w3)
        assert (t3[[7, 8]] == 0).all() and (t3[[0, 1, 2, 3, 4, 5, 6, 9, 10]] != 0).all()


def test_zero_table_returns_preps_own_arrays_and_both_functions_are_put_back():
    st, dyn, _, w = nw.case_inputs(5, states=STATES)
    prep0, uv0 = ns.prep, na.unconstrained_velocities
    seen = []

    def spy(*a, **k):
        seen.append(prep0(*a, **k))
        return seen[-1]
    ns.prep = spy
    try:
        with nw.applied(np.zeros((14, 6)), dyn[0]):
            got = ns.prep(st[0].astype(np.float64), dyn[0])
        with nw.applied(-np.zeros((5, 14, 6))):            # negative zeros are zeros
            got2 = ns.prep(st.astype(np.float64), dyn)
        # object rows only: qds is the record's own array; robot rows only: ovs and ows are
        with nw.applied(w[4], dyn[4]):
            got3 = ns.prep(st[4].astype(np.float64), dyn[4])
        with nw.applied(w[3], dyn[3]):
            got4 = ns.prep(st[3].astype(np.float64), dyn[3])
    finally:
        ns.prep = prep0
    assert got is seen[0] and got2 is seen[1]
    assert got3['qds'] is seen[2]['qds'] and got3['ovs'] is not seen[2]['ovs']
    assert got4['ovs'] is seen[3]['ovs'] and got4['ows'] is seen[3]['ows'] and got4['qds'] is not seen[3]['qds']
    for k in got3:
        if k not in ('qds', 'ovs', 'ows'):
            assert got3[k] is seen[2][k] and got4[k] is seen[3][k], k
    try:
        with nw.applied(w[0], dyn[0]):
            assert ns.prep is not prep0 and na.unconstrained_velocities is not uv0
            raise RuntimeError
    except RuntimeError:
        pass
    assert ns.prep is prep0 and na.unconstrained_velocities is uv0


def test_wrapper_adds_the_closed_forms():
    st, dyn, _, w = nw.case_inputs(5, states=STATES)
    s, d, w64 = st.astype(np.float64), dyn.astype(np.float64), w.astype(np.float64)
    base = ns.prep(s, d)
    with nw.applied(w64):
        got = ns.prep(s, d)
        uv = na.unconstrained_velocities(base, s[:, NB:2 * NB], ns.model()['body_damping'])
    m = ns.model()
    c = base['p'] + np.einsum('nbij,bj->nbi', base['R'], m['body_com'])
    tau = np.zeros((5, NB))
    for n in range(5):
        for k in range(NB):
            for b in range(NB):
                if m['anc'][b, k]:
                    tau[n, k] += base['axis'][n, k] @ (np.cross(c[n, b] - base['p'][n, k], w64[n, b, :3]) + w64[n, b, 3:])
    assert np.allclose(got['qds'], base['qds'] + ns.DT * np.einsum('nij,nj->ni', base['Minv'], tau), rtol=0, atol=1e-12)
    assert np.allclose(uv, base['qds'] + ns.DT * np.einsum('nij,nj->ni', base['Minv'], tau), rtol=0, atol=1e-9)
    assert np.allclose(got['ovs'], base['ovs'] + ns.DT * w64[:, NB:, :3] / d[..., :1], rtol=0, atol=1e-14)
    assert np.allclose(got['ows'], base['ows'] + ns.DT * np.einsum('noij,noj->noi', base['oIinv'], w64[:, NB:, 3:]), rtol=0, atol=1e-12)
    # an object the out-of-bounds rule sends home takes the wrench at its home pose: prep's oIinv is that pose's
    for k in base:
        if k not in ('qds', 'ovs', 'ows'):
            assert np.array_equal(got[k], base[k]), k
    # the zero targets of the table keep their values
    assert np.array_equal(got['qds'][[2, 4]], base['qds'][[2, 4]])
    assert np.array_equal(got['ovs'][[2, 3]], base['ovs'][[2, 3]]) and np.array_equal(got['ows'][4, [0, 2]], base['ows'][4, [0, 2]])


@pytest.mark.parametrize('N', [5, 21])
def test_every_control_differs_from_the_feature_by_more_than_the_gpu_ceilings(N):
    """On the GPU test's inputs (N = 5: its very states; N = 21: every edge of edge_states, drawn like its N = 70): each wrong feature, and the previous step's table, lies further than TWICE the float32 ceilings of
    the GPU test from the reference with the wrench applied, on every env whose relevant rows are non-zero -- so a device within
    the ceilings of the feature misses every control."""
    st, dyn, w_prev, w = nw.case_inputs(N, states=STATES)
    s, d = st.astype(np.float64), dyn.astype(np.float64)
    base = ns.prep(s, d)
    want = nw.add_to(base, w, d)
    ceil = nw.prep_ceilings(base, st, w, d)
    robot, obj = (w[:, :NB] != 0).any((1, 2)), (w[:, NB:] != 0).any((1, 2))
    assert not robot[2] and not obj[2] and robot[3] and not obj[3] and obj[4] and not robot[4] and (robot & obj).sum() == N - 3
    for name, rel in nw_controls(robot, obj).items():
        other = nw.add_to(base, w_prev if name == 'one step late' else w, d, 'applied' if name == 'one step late' else name)
        r = control_ratio(other, want, ceil)
        print("N=%d control %-13s smallest ratio over its envs %.1f" % (N, name, r[rel].min()))
        assert (r[rel] > 2.0).all(), (name, np.flatnonzero(rel & (r <= 2.0)))
        assert (r[~robot & ~obj] == 0).all()


def nw_controls(robot, obj):
    """control -> the envs whose relevant rows are non-zero (bool [N])."""
    return {'negated': robot | obj, 'mass': robot | obj, 'no_arm': robot, 'no_ancestors': robot, 'model_mass': obj, 'one step late': robot | obj}


def control_ratio(got, want, ceil):
    """Per env: the largest |got - want| / ceiling over qd*, v*, w*."""
    cq, cv, cw = ceil
    return np.maximum(np.maximum((np.abs(got['qds'] - want['qds']) / cq).max(1), (np.abs(got['ovs'] - want['ovs']) / cv).max((1, 2))),
                      (np.abs(got['ows'] - want['ows']) / cw).max((1, 2)))
