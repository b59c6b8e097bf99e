"""CPU tests of the float64 reference the joint-space dynamics at candidate postures are checked against (tests/numpy_dynamics.py over
tests/numpy_step.py): three properties of the reference itself, and the negative controls -- wrong references that the ceilings of
tests/test_gpu_posture_dynamics.py must refuse on every row of that test's own inputs, at the shipped constants and at the cap of
1e-4 no constant may be raised above.

Smallest worst-ratio over a row at C_M = C_V = 2e-5 over the 1 202 rows of the three shapes, edge rows included (measured by this
file, which prints them; divide by 5 for the cap; in brackets what the issue reports for its own sample of 400 uniform postures):
M without the rotational inertias 5.0e4 (1e5) -- 1 / C_M: a diagonal entry that is rotational inertia alone is wrong by itself, and
the difference of the two matrices being positive semi-definite no entry can do more; bias without the Coriolis terms on the rows
with qd != 0 1.47e3 (1 600); the wrist body's mass + 1 %: gravity 9.5 (45; 24 on the straight-elbow rows); a fingertip body's mass
+ 1 %: gravity 44 (53), bias 11.3 (15).  All are above 5, so every control still misses the cap on every row (smallest 1.9 x)."""
import numpy as np
import pytest

from tests import numpy_dynamics as nd
from tests import numpy_step as ns


_rows = nd.all_rows


def test_inputs_are_what_the_issue_asks_for():
    lo, hi = nd.limits()
    for N, K in nd.SHAPES:
        q, qd, qdd = nd.inputs(N, K)
        assert q.shape == qd.shape == qdd.shape == (N, K, 11) and q.dtype == qd.dtype == qdd.dtype == np.float32
        kind = nd.edge_kind(N * K).reshape(N, K)
        assert (q >= lo.astype(np.float32) - 1e-6).all() and (q <= hi.astype(np.float32) + 1e-6).all()
        assert np.abs(qd[kind != 1]).max() <= 3 and np.abs(qdd).max() <= 10
        assert not qd[kind == 0].any()
        if (kind == 1).any():
            assert np.abs(qd[kind == 1]).max() > 3 and np.abs(qd[kind == 1]).max() <= 40
        if (kind == 2).any():
            assert not q[kind == 2][:, 3].any() and (q[kind == 2][:, 5] == np.float32(1e-7)).all()
        if (kind == 3).any():
            assert (q[kind == 3][:, 7:9] == lo[7:9].astype(np.float32)).all() and (q[kind == 3][:, 9:11] == hi[9:11].astype(np.float32)).all()
    # the largest shape has every kind of edge row
    assert set(nd.edge_kind(37 * 32)) == {-1, 0, 1, 2, 3}


def test_mass_matrix_is_symmetric_positive_definite():
    _, _, _, ref, _ = _rows()
    M = ref['mass_matrix']
    d = np.sqrt(np.einsum('rii->ri', M))
    assert (np.abs(M - M.transpose(0, 2, 1)) <= 1e-14 * d[:, :, None] * d[:, None, :]).all()
    assert np.linalg.eigvalsh(M).min() > 0
    # the two finger branches do not couple
    assert not M[:, 7:9, 9:11].any() and not M[:, 9:11, 7:9].any()
    assert np.abs(np.einsum('rij,rjk->rik', M, ref['mass_inverse']) - np.eye(11)).max() < 1e-9


def test_coriolis_terms_are_even_in_the_velocity():
    q, qd, _, ref, _ = _rows()
    q, qd = q[:200], qd[:200]
    G = ref['gravity'][:200]
    c_plus, c_minus = ref['bias'][:200] - G, ns.bias(q, -qd.astype(np.float64)) - G
    assert np.abs(c_plus - c_minus).max() <= 1e-12 * max(1.0, np.abs(c_plus).max())


def test_power_identity():
    """qd . C(q, qd) = 1/2 qd^T Mdot qd with Mdot = sum_k dM/dq_k qd_k from the complex-step derivative: the Coriolis terms do no work
    beyond the change of the kinetic energy."""
    q, qd, _, ref, _ = _rows()
    q, qd = q[:200].astype(np.float64), qd[:200].astype(np.float64)
    C = ref['bias'][:200] - ref['gravity'][:200]
    qc = ns._cs_points(q)
    Mdot = sum(ns.mass_matrix_and_potential(qc[k])[0].imag / ns.CS_H * qd[:, k, None, None] for k in range(ns.NB))
    lhs = np.einsum('ri,ri->r', qd, C)
    rhs = 0.5 * np.einsum('ri,rij,rj->r', qd, Mdot, qd)
    scale = np.einsum('ri,ri->r', np.abs(qd), np.abs(C)) + 1e-30
    assert (np.abs(lhs - rhs) <= 1e-10 * scale).all(), float((np.abs(lhs - rhs) / scale).max())


# control -> {field: the factor over the ceiling that the issue reports for it at C_M / C_V, on its own sample of 400 uniform postures}
REPORTED = {'no_rotational_inertia': dict(mass_matrix=1e5), 'no_coriolis': dict(bias=1600.0), 'wrist_mass_1pc': dict(gravity=45.0),
            'fingertip_mass_1pc': dict(gravity=53.0, bias=15.0)}


@pytest.mark.parametrize('control', sorted(REPORTED))
def test_negative_control_misses_the_ceiling_on_every_row(control):
    """Every wrong reference is outside the ceiling on EVERY row of the GPU test's inputs -- at the shipped constants and at the cap
    C_CAP = 1e-4 (x 5 wider) no constant may be raised above.  `no_coriolis` is judged on the rows with a velocity: at qd = 0 exactly
    the bias has no Coriolis term to leave out."""
    q, qd, qdd, ref, kind = _rows()
    scale = nd.scales(ref, qdd)
    wrong = nd.controls_of_all_rows()[control]
    rows = kind != 0 if control == 'no_coriolis' else np.ones(len(q), bool)
    assert nd.C_CAP / nd.C_M == nd.C_CAP / nd.C_V == 5.0
    for name, reported in REPORTED[control].items():
        r = nd.row_ratios(wrong[name], ref, scale, name)[rows]
        print(control, name, 'smallest worst-ratio over a row %.3g (on the sample of the issue: %.3g)' % (r.min(), reported), 'edge rows:',
              {nd.EDGE_KINDS[k]: float('%.3g' % r[kind[rows] == k].min()) for k in range(4) if (kind[rows] == k).any()})
        assert r.min() > 1.0, (control, name, float(r.min()))
        assert r.min() * nd.C_M / nd.C_CAP > 1.0, (control, name, float(r.min()))
