"""The per-joint float64 step (tests/numpy_actuators.py) pinned against the yardstick it restates: with rows that are constant over
the joints it returns the very state of `numpy_step.step(..., solver={...})` on the scenes of tests/test_numpy_step.py (contacts
from the float64 oracle), for the default constants and for SECOND of tests/test_gpu_solver_params.py -- same arithmetic in the
same order, so equality is exact.  Plus two per-joint properties that need no other implementation: a joint with max_force 0 has a
motor impulse of exactly 0, and a joint with kp 0 and kd 1 has motor target velocity 0 whatever the command."""
import numpy as np
import pytest

import oracle.oracle as oracle_mod
from oracle.oracle import Oracle, params_from_solver
from tests import numpy_actuators as na
from tests import numpy_step as ns
from tests.test_gpu_solver_params import SECOND
from tests.test_numpy_step import NOBJ, SCENES, scene

SETS = {'default': None, 'second': SECOND}


def _oracle_contacts(name, solver):
    st, prev, cmd = scene(name)
    o = Oracle(NOBJ.get(name, 3), 32, 32, **params_from_solver(solver))
    o.state = st
    o.set_contact_cache(prev)
    o.step(cmd)
    return o.contacts()


@pytest.mark.parametrize('sset', list(SETS))
@pytest.mark.parametrize('name', list(SCENES))
def test_constant_rows_reproduce_the_scalar_step_exactly(name, sset):
    solver = SETS[sset]
    st, prev, cmd = scene(name)
    k = NOBJ.get(name, 3)
    contacts = _oracle_contacts(name, solver)
    dyn = ns.default_dynamics(k)
    want = ns.step(st, cmd, contacts, dyn=dyn, prev=prev, solver=solver, nobj=k)
    P = dict(ns.SOLVER_DEFAULTS, **(solver or {}))
    # once through the defaults of the helper, once with explicit arrays of 11
    for kw in ({}, dict(kp=np.full(11, P['motor_kp']), kd=np.full(11, P['motor_kd']), max_force=np.full(11, P['motor_max_force']),
                        damping=np.array(ns.model()['body_damping'], dtype=np.float64))):
        got = na.step(st, cmd, contacts, dyn=dyn, prev=prev, solver=solver, nobj=k, **kw)
        assert np.array_equal(got['state'], want['state']), np.abs(got['state'] - want['state']).max()
        assert np.array_equal(got['lam'], want['lam']) and np.array_equal(got['qds'], want['prep']['qds'])


@pytest.mark.parametrize('name', ['grasp', 'press', 'free'])
def test_a_joint_without_motor_force_has_no_motor_impulse(name):
    st, prev, cmd = scene(name)
    contacts = _oracle_contacts(name, None)
    force = np.full(11, 100000.0)
    force[[2, 8]] = 0.0
    got = na.step(st, cmd, contacts, prev=prev, max_force=force)
    ref = na.step(st, cmd, contacts, prev=prev)
    assert [r[0] for r in got['rows'][:11]] == ['motor'] * 11
    assert got['lam'][2] == 0.0 and got['lam'][8] == 0.0
    assert ref['lam'][2] != 0.0 and ref['lam'][8] != 0.0          # (not vacuous: these motors work in the scalar step)
    assert np.all(got['lam'][[0, 1, 3, 4, 5, 6, 7, 9, 10]] != 0.0)
    assert not np.array_equal(got['state'], ref['state'])


def test_a_joint_with_kp_0_and_kd_1_has_target_velocity_0_whatever_the_command():
    st, prev, _ = scene('free')
    contacts = np.zeros((0, 12))
    kp, kd = np.full(11, 0.1), np.full(11, 1.0)
    kp[[1, 4]] = 0.0
    rng = np.random.default_rng(0)
    seen = []
    for _ in range(4):
        cmd = rng.uniform(-1.5, 1.5, 9)
        got = na.step(st, cmd, contacts, kp=kp, kd=kd)
        assert got['vt'][1] == 0.0 and got['vt'][4] == 0.0
        seen.append(got['vt'].copy())
    assert np.ptp(np.array(seen)[:, [0, 2, 3, 5, 6]], axis=0).min() > 0      # the other arm joints' targets follow the command


def test_per_joint_damping_enters_the_unconstrained_velocities():
    st, prev, cmd = scene('press')
    d0 = np.array(ns.model()['body_damping'], dtype=np.float64)
    scale = np.linspace(0.0, 4.0, 11)
    got = na.step(st, cmd, np.zeros((0, 12)), damping=d0 * scale)
    pr = got['prep']
    qd = np.asarray(st, dtype=np.float64)[11:22]
    # M qdd = -bias - damping qd, joint by joint
    M = np.linalg.inv(pr['Minv'])
    res = M @ ((got['qds'] - qd) / ns.DT) + pr['bias'] + d0 * scale * qd
    assert np.abs(res).max() < 1e-9 * max(1.0, np.abs(pr['bias']).max())
    assert not np.array_equal(got['qds'], pr['qds'])
