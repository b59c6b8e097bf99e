"""The float64 reference of the step's external wrenches (rr_set_external_wrenches), for the tests; a helper module: pytest does not
collect it.  tests/numpy_step.py is not edited: `applied(w, dyn)` replaces its `prep` for the length of a `with` block by a wrapper
that adds the three terms of the feature to the returned record --
    qds += DT * Minv @ tau,   tau_k = sum over the bodies b that joint k moves of a_k . ((c_b - p_k) x F_b + T_b),  c_b = p_b + R_b com_b
    ovs += DT * F / m         m the ENV's own mass, dyn[..., 0]
    ows += DT * oIinv @ T     prep's world inverse inertia of the pose that counts
-- so that `numpy_step.step` sees the wrench; motors, limit rows and contacts act on top, unchanged.  tests/numpy_actuators.step forms
its own qd* from prep's M^-1 and bias, so its `unconstrained_velocities` is wrapped the same way for the same block.  Both are put
back on exit.  w is [..., 14, 6]: rows 0..10 the robot bodies, rows 11.. the objects; a row is {F, T} in the world frame.

`mode` states the wrong features the GPU test's negative controls are judged against, on the reference side:
  'negated'       -w in w's place;
  'mass'          m in the place of 1 / m (and the world inertia in the place of its inverse), M in the place of M^-1;
  'no_arm'        c_b - p_k dropped: the force taken at the joint's origin, where it has no moment;
  'no_ancestors'  a body's wrench reaching its own joint only;
  'model_mass'    the model's object mass in the place of the env's.
(The sixth control, a wrench applied one step late, is the reference with the previous step's table: it needs no mode.)"""
import contextlib

import numpy as np

from tests import numpy_actuators as na
from tests import numpy_step as ns
from tests.numpy_step import DT, NB

MODES = ('applied', 'negated', 'mass', 'no_arm', 'no_ancestors', 'model_mass')
XW_BODIES = 14


def body_centres(pr):
    """c_b = p_b + R_b com_b [..., 11, 3] of a preparation record: the centres of mass numpy_step's mass matrix uses."""
    return pr['p'] + np.einsum('...bij,bj->...bi', pr['R'], ns.model()['body_com'])


def generalised_force(pr, w, mode='applied'):
    """tau [..., 11] of the robot rows of w [..., >= 11, 6] from prep's R, p, axis and the model's anc, body_com."""
    assert mode in MODES, mode
    m = ns.model()
    w = np.asarray(w, dtype=np.float64)[..., :NB, :]
    F, T = w[..., :3], w[..., 3:]
    p, ax = pr['p'], pr['axis']
    d = body_centres(pr)[..., :, None, :] - p[..., None, :, :]                      # [..., body, joint, 3]
    if mode == 'no_arm':
        d = np.zeros_like(d)
    anc = np.eye(NB) if mode == 'no_ancestors' else m['anc']
    mom = np.cross(d, np.broadcast_to(F[..., :, None, :], d.shape)) + T[..., :, None, :]
    tau = np.einsum('...bki,...ki,bk->...k', mom, ax, anc)
    return -tau if mode == 'negated' else tau


def robot_term(pr, w, mode='applied'):
    """dt M^-1 tau [..., 11] (or the wrong term of a control)."""
    A = pr['M'] if mode == 'mass' else pr['Minv']
    return DT * np.einsum('...ij,...j->...i', A, generalised_force(pr, w, mode))


def object_terms(pr, w, dyn, mode='applied'):
    """(dt F / m, dt Iinv T), each [..., nobj, 3], of the object rows of w [..., 14, 6]; dyn [..., nobj, 8] the env's dynamics rows."""
    assert mode in MODES, mode
    nobj = pr['ovs'].shape[-2]
    w = np.asarray(w, dtype=np.float64)[..., NB:NB + nobj, :]
    if mode == 'negated':
        w = -w
    mass = (ns.default_dynamics(nobj) if mode == 'model_mass' else np.asarray(dyn, dtype=np.float64))[..., 0]
    A = pr['oIinv']
    if mode == 'mass':
        mass, A = 1.0 / mass, np.linalg.inv(A)
    return DT * w[..., :3] / mass[..., None], DT * np.einsum('...ij,...j->...i', A, w[..., 3:])


def add_to(pr, w, dyn, mode='applied'):
    """prep's record with the feature's terms added; a target whose rows are all zero keeps the record's own array."""
    w = np.asarray(w, dtype=np.float64)
    out = dict(pr)
    if (w[..., :NB, :] != 0).any():
        out['qds'] = pr['qds'] + robot_term(pr, w, mode)
    nobj = pr['ovs'].shape[-2]
    if (w[..., NB:NB + nobj, :] != 0).any():
        dv, dw = object_terms(pr, w, dyn, mode)
        out['ovs'], out['ows'] = pr['ovs'] + dv, pr['ows'] + dw
    return out


@contextlib.contextmanager
def applied(w, dyn=None, mode='applied'):
    """Within the block `numpy_step.prep` returns its own record with the wrench table w [..., 14, 6] applied (broadcasting against
    the state's leading dimensions); dyn [..., nobj, 8]: the env's dynamics rows (None: the rows prep is called with), and
    `numpy_actuators.unconstrained_velocities` adds the robot's term.  Nothing else of the record changes; with w all zero the
    record's own arrays come back."""
    assert mode in MODES, mode
    w = np.asarray(w, dtype=np.float64)
    prep0, uv0 = ns.prep, na.unconstrained_velocities

    def prep(state, dyn_arg, *a, **k):
        pr = prep0(state, dyn_arg, *a, **k)
        if not (w != 0).any():
            return pr
        return add_to(pr, w, dyn_arg if dyn is None else dyn, mode)

    def unconstrained_velocities(pr, qd, damping):
        out = uv0(pr, qd, damping)
        return out + robot_term(pr, w, mode) if (w[..., :NB, :] != 0).any() else out

    ns.prep, na.unconstrained_velocities = prep, unconstrained_velocities
    try:
        yield
    finally:
        ns.prep, na.unconstrained_velocities = prep0, uv0


def body_weights(nobj=3, dyn=None):
    """m g of the fourteen rows [14]: the model's robot bodies, then the objects (dyn [nobj, 8]: their rows; None: the model's);
    rows of absent objects 0."""
    out = np.zeros(XW_BODIES)
    out[:NB] = ns.model()['body_mass'] * ns.GRAVITY
    out[NB:NB + nobj] = (ns.default_dynamics(nobj) if dyn is None else np.asarray(dyn, dtype=np.float64))[:, 0] * ns.GRAVITY
    return out


def random_wrenches(N, seed, dyn=None, nobj=3):
    """w [N, 14, 6] float32: forces uniform within +-3 x the body's weight, torques within +-3 x weight x 0.05 m (dyn [N, nobj, 8]:
    the envs' own object rows)."""
    rng = np.random.default_rng(seed)
    wt = np.stack([body_weights(nobj, None if dyn is None else dyn[i]) for i in range(N)])          # [N, 14]
    w = rng.uniform(-3.0, 3.0, (N, XW_BODIES, 6)) * wt[:, :, None]
    w[:, :, 3:] *= 0.05
    return w.astype(np.float32)


def case_inputs(N, nobj=3, states=None):
    """The inputs of the one-step GPU test (tests/test_gpu_external_wrenches.py), shared with the reference's own tests: states
    [N, 61] from test_gpu_numpy_step.edge_states (which runs the device; `states`: recorded ones in their place, for the tests
    without one), per-env dynamics rows [N, nobj, 8] from its random_dynamics, the previous step's table and this step's
    [N, 14, 6] float32.  In both tables env 2 is all zero, env 3 has robot rows only, env 4 one object row (object 1) only."""
    from tests.test_gpu_numpy_step import edge_states, random_dynamics
    st, dyn = (edge_states(N, 3) if states is None else np.asarray(states, np.float32)[:N]), random_dynamics(N, 5, nobj)
    tables = []
    for seed in (61, 62):
        w = random_wrenches(N, seed, dyn.astype(np.float64), nobj)
        w[2] = 0.0
        w[3, NB:] = 0.0
        w[4, :NB + 1] = 0.0
        w[4, NB + 2:] = 0.0
        w[:, NB + nobj:] = 0.0
        tables.append(w)
    return st, dyn, tables[0], tables[1]


def prep_ceilings(pr, st, w, dyn):
    """The float32 ceilings of |device - numpy| of the three touched fields of the preparation record with the table w applied:
    qd* at numpy_torque.qds_ceiling with the generalised force in tau's place [N, 1]; v* and w* at test_gpu_numpy_step's
    1e-6 (1 + |v|) widened by the size of the added term, 1e-6 (1 + |v| + |added term|) [N, nobj, 1].  pr: numpy_step.prep's record
    WITHOUT the wrench."""
    from tests import numpy_torque as nt
    N, nobj = len(st), pr['ovs'].shape[-2]
    s = np.asarray(st, dtype=np.float64)
    ob = s[:, 22:22 + 13 * nobj].reshape(N, nobj, 13).copy()
    ob[pr['oob']] = 0.0
    dv, dw = object_terms(pr, w, dyn)
    n = lambda a: np.linalg.norm(a, axis=-1)[..., None]
    return (nt.qds_ceiling(pr, s[:, NB:2 * NB], generalised_force(pr, w)),
            1e-6 * (1 + n(ob[..., 7:10]) + n(dv)), 1e-6 * (1 + n(ob[..., 10:13]) + n(dw)))
