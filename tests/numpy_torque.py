"""The float64 reference of the step's joint torque inputs (rr_set_joint_torques), for the tests; a helper module: pytest does not
collect it.  tests/numpy_step.py is not edited: `applied(tau)` replaces its `prep` for the length of a `with` block by a wrapper that
adds DT * Minv @ tau to the returned `qds` -- the one place the feature acts, qd*' = qd* + dt M^-1 tau -- so that `numpy_step.step`
sees the torque; the motors, limit rows and contacts of that step act on top, unchanged.  tests/numpy_actuators.step (per-joint
motors: a joint with max_force 0 is torque controlled) forms its own qd* from prep's M^-1 and bias, so its
`unconstrained_velocities` is wrapped the same way for the same block.  Both are put back on exit.

`mode` states the wrong features the GPU test's negative controls are judged against, on the reference side:
  'negated'  -tau in tau's place;
  'mass'     M in the place of M^-1.
(The third control, a torque applied one step late, is the reference with the previous step's table: it needs no mode.)

`free_arm_rollout` is the step of an arm that no row touches -- motors off, no joint within the limit window, no robot contact --:
qd <- qd*', q <- q + dt qd.  tests/test_numpy_torque.py checks that `numpy_step.step` does exactly that for such a state."""
import contextlib

import numpy as np

from tests import numpy_actuators as na
from tests import numpy_step as ns
from tests.numpy_step import DT, NB

MODES = ('applied', 'negated', 'mass')
HOLD_STEPS = 50
HOLD_RATIO = 0.05
# three mid-range postures: every limited joint further than numpy_step.LIMIT_WINDOW from its limits, the arm bent (gravity loads the
# shoulder, elbow and wrist joints), the fingers half open; held there the arm touches neither the table nor the objects that settle on it
HOLD_POSTURES = np.array([[0.4, 0.5, -0.5, -1.2, 0.3, 0.8, 0.2, 0.6, -0.7, 0.6, -0.7],
                          [-0.9, -0.6, 0.8, 1.1, -0.4, -0.7, 0.5, 0.8, -0.8, 0.7, -0.9],
                          [1.2, 1.0, 0.2, 0.9, 1.0, 0.5, -0.6, 0.9, -0.6, 0.8, -0.8]])


def torque_term(pr, tau, mode='applied'):
    """dt M^-1 tau from a preparation record (float64; broadcasts over leading dimensions), or the wrong term of a control."""
    assert mode in MODES, mode
    tau = np.asarray(tau, dtype=np.float64)
    A = pr['M'] if mode == 'mass' else pr['Minv']
    return DT * np.einsum('...ij,...j->...i', A, -tau if mode == 'negated' else tau)


@contextlib.contextmanager
def applied(tau, mode='applied'):
    """Within the block `numpy_step.prep` returns its own record with `qds` replaced by qds + DT * Minv @ tau (tau [..., 11],
    broadcasting against the state's leading dimensions), and `numpy_actuators.unconstrained_velocities` adds the same term.  Nothing
    else of the record changes; with tau all zero the record's own arrays come back."""
    tau = np.asarray(tau, dtype=np.float64)
    prep0, uv0 = ns.prep, na.unconstrained_velocities

    def prep(*a, **k):
        pr = prep0(*a, **k)
        if not tau.any():
            return pr
        return dict(pr, qds=pr['qds'] + torque_term(pr, tau, mode))

    def unconstrained_velocities(pr, qd, damping):
        out = uv0(pr, qd, damping)
        return out + torque_term(pr, tau, mode) if tau.any() else out

    ns.prep, na.unconstrained_velocities = prep, unconstrained_velocities
    try:
        yield
    finally:
        ns.prep, na.unconstrained_velocities = prep0, uv0


def joint_terms(q, qd, damping=None):
    """M^-1 [..., 11, 11] and bias [..., 11] of numpy_step at (q, qd), and qd* under `damping` (None: the model's)."""
    q, qd = np.asarray(q, np.float64), np.asarray(qd, np.float64)
    M, _ = ns.mass_matrix_and_potential(q)
    b = ns.bias(q, qd)
    Minv = np.linalg.inv(M)
    d = ns.model()['body_damping'] if damping is None else damping
    return Minv, b, qd + DT * np.einsum('...ij,...j->...i', Minv, -b - d * qd)


def free_arm_step(q, qd, tau, damping=None):
    """One step of the free arm: (q', qd') = (q + dt qd*', qd*') with qd*' = qd* + dt M^-1 tau."""
    Minv, _, qds = joint_terms(q, qd, damping)
    qds = qds + DT * np.einsum('...ij,...j->...i', Minv, np.asarray(tau, np.float64))
    return np.asarray(q, np.float64) + DT * qds, qds


def free_arm_rollout(q0, steps, torque_of, damping=None):
    """`steps` free-arm steps from q0 [..., 11] at rest; torque_of(q, qd) gives the table of each step.  Returns q [steps + 1, ..., 11]."""
    q, qd = np.asarray(q0, np.float64), np.zeros_like(np.asarray(q0, np.float64))
    out = [q]
    for _ in range(steps):
        q, qd = free_arm_step(q, qd, torque_of(q, qd), damping)
        out.append(q)
    return np.stack(out)


def float32_bias(q, qd):
    """The torque table a float32 controller sets: numpy_step's bias at (q, qd), rounded to float32."""
    return ns.bias(q, qd).astype(np.float32).astype(np.float64)


def drift(qs):
    """Per leading row: the largest joint excursion from the start over a rollout q [steps + 1, ..., 11]."""
    return np.abs(qs - qs[0]).max(axis=(0, -1))


def qds_ceiling(pr, qd, tau):
    """tests/test_gpu_numpy_step.py's ceiling of |device - numpy| of qd*, 2e-4 + 2e-6 |qd| + 5e-5 bterm, with bterm taken over
    dt M^-1 (bias - tau): the argument given there -- float32 epsilon x the mass matrix's condition x the term's size -- applies to
    the added term unchanged.  pr: numpy_step.prep's record WITHOUT the torque; qd [..., 11]."""
    bterm = np.abs(DT * np.einsum('...ij,...j->...i', pr['Minv'], pr['bias'] - np.asarray(tau, np.float64))).max(-1, keepdims=True)
    return 2e-4 + 2e-6 * np.abs(np.asarray(qd, np.float64)).max(-1, keepdims=True) + 5e-5 * bterm
