"""CPU tests (-m "not gpu") of the float64 reference of the signed-distance gradients: the committed differences
(tests/golden/signed_gradient.npz, written by tests/golden/make_signed_gradient.py) are reproducible, the header's formula restated in
float64 agrees with them on the items that are compared, four deliberately wrong evaluations do not, and enough items are compared."""
import numpy as np
import pytest

from tests import numpy_distance as nd
from tests import numpy_posture as npo
from tests import numpy_signed_gradient as nsg
from tests import numpy_step as ns

NOISE = 1e-7                  # m: the reference's d carries about 3e-8 m of qhull noise; a recomputed distance may differ from the file's by that
ROWS, PAIRS = (0, 5), tuple(range(0, 80, 8))       # the items that are recomputed: two rows x ten pairs
SUBSET = [(r, j) for r in range(16) for j in range(0, 80, 4)]      # the items the restatement is evaluated on: every fourth pair

_cache = {}


def _case_r():
    if 'r' not in _cache:
        st, po, pairs = npo.case_r_inputs()
        rows = npo.rows(st, po)
        _cache['r'] = (st, po, pairs, rows, nsg.witnesses(rows, pairs, SUBSET))
    return _cache['r']


def _file(tag):
    f = nsg.fixture()
    d0, dp, dm = f[tag + '_d0'], f[tag + '_dplus'], f[tag + '_dminus']
    cen, fwd, bwd = nsg.derivatives(d0, dp, dm, float(f['h']))
    return d0, cen, fwd, bwd, nsg.compared(d0, fwd, bwd)


def test_the_fixture_is_what_the_generator_says():
    f = nsg.fixture()
    assert float(f['h']) == nsg.H and float(f['smooth']) == nsg.SMOOTH and float(f['margin']) == nsg.MARGIN
    assert f['r_d0'].shape == (16, 80) and f['r_dplus'].shape == f['r_dminus'].shape == f['r_formula'].shape == (16, 80, 11)
    assert f['p_d0'].shape == (5, 7) and f['p_dplus'].shape == f['p_dminus'].shape == (5, 7, 11)
    assert f['r_cost_fd'].shape == (16, 11) and f['r_cost_rows'].shape == (16,) and f['r_cost_rows'].sum() >= 8
    # the undisturbed distances are the cases' own references
    assert np.abs(f['r_d0'] - npo.case_r()['d']).max() <= NOISE and np.abs(f['p_d0'] - nd.case(5)[2]['d']).max() <= NOISE
    # TOL_G: four times the restatement's largest error over the compared items of both cases
    err = max(float(np.abs(f[t + '_formula'] - _file(t)[1]).max(-1)[_file(t)[4]].max()) for t in ('r', 'p'))
    assert float(f['formula_error']) == pytest.approx(err, rel=1e-12) and float(f['tol_g']) == pytest.approx(4 * err, rel=1e-12)
    assert 1e-6 < float(f['tol_g']) < 4 * nsg.SMOOTH       # (a smooth item's central difference is within |fwd - bwd| / 2 of either one-sided one)
    # a static pair -- no robot shape on either side -- has no gradient at all
    st5, pairs5, _ = nd.case(5)
    static = (nsg.bodies(pairs5) < 0).all(1)
    assert static.any() and (f['p_dplus'][:, static] == f['p_d0'][:, static, None]).all() and (f['p_dminus'][:, static] == f['p_d0'][:, static, None]).all()


def test_recomputed_differences_match_the_file():
    st, po, pairs, rows, _ = _case_r()
    items = [(r, j) for r in ROWS for j in PAIRS]
    d0, dp, dm = nsg.differences(rows, pairs, items=items)
    f = nsg.fixture()
    r, j = np.array(items).T
    for name, mine in (('r_d0', d0), ('r_dplus', dp), ('r_dminus', dm)):
        assert np.isfinite(mine[r, j]).all() and np.abs(mine[r, j] - f[name][r, j]).max() <= NOISE, name


def test_float64_formula_against_the_differences():
    st, po, pairs, rows, W = _case_r()
    f = nsg.fixture()
    d0, cen, fwd, bwd, ok = _file('r')
    r, j = np.array(SUBSET).T
    g = nsg.formula_items(rows, pairs, SUBSET, W)
    assert np.abs(g - f['r_formula'][r, j]).max() <= 1e-9                 # the file's restatement is this one
    assert np.abs(W['s'] - d0[r, j]).max() <= NOISE and np.abs(np.linalg.norm(W['n'], axis=1) - 1).max() <= 1e-9
    assert np.abs(W['a'] - W['b'] - W['s'][:, None] * W['n']).max() <= 1e-6      # a - b = s n for both signs
    err = np.abs(g - cen[r, j]).max(-1)
    sel = ok[r, j]
    print('formula vs central differences on %d compared of %d items: max %.3g, 99 %% %.3g; on the others max %.3g; overlapping compared %d, max %.3g'
          % (sel.sum(), len(sel), err[sel].max(), np.quantile(err[sel], 0.99), err[~sel].max() if (~sel).any() else 0.0,
             (sel & (d0[r, j] < 0)).sum(), err[sel & (d0[r, j] < 0)].max()))
    assert err[sel].max() <= float(f['formula_error']) * (1 + 1e-9)
    # over the whole file: both cases, every compared item
    for tag in ('r', 'p'):
        d0, cen, fwd, bwd, ok = _file(tag)
        assert np.abs(f[tag + '_formula'] - cen).max(-1)[ok].max() <= float(f['tol_g']) / 4 * (1 + 1e-9)
    assert np.abs(_file('r')[1]).max() > 0.5                                # (gradients of the order of a lever, not of the tolerance)


@pytest.mark.parametrize('control', nsg.CONTROLS)
def test_controls_miss_the_differences(control):
    st, po, pairs, rows, W = _case_r()
    tol = float(nsg.fixture()['tol_g'])
    d0, cen, fwd, bwd, ok = _file('r')
    r, j = np.array(SUBSET).T
    present = np.repeat(np.asarray(st, dtype=np.float64)[:, :ns.NB], 4, axis=0)
    neighbour = np.roll(np.asarray(po, dtype=np.float64), 1, axis=1).reshape(16, ns.NB)
    g = nsg.formula_items(rows, pairs, SUBSET, W, control=control, present=present, neighbour=neighbour)
    err = np.abs(g - cen[r, j]).max(-1)[ok[r, j]]
    print('%s: misses the differences by %.3g at most (10 x TOL_G = %.3g), on %d of %d compared items by more than TOL_G'
          % (control, err.max(), 10 * tol, (err > tol).sum(), len(err)))
    assert err.max() >= 10 * tol


def test_enough_items_are_compared():
    for tag, overlapping in (('r', 10), ('p', 0)):
        d0, cen, fwd, bwd, ok = _file(tag)
        dec = np.abs(d0) >= nd.DECIDE
        print('case %s: %d decided, %d compared, overlapping compared %d' % (tag, dec.sum(), ok.sum(), (ok & (d0 < 0)).sum()))
        assert ok.sum() >= 0.9 * dec.sum() and (ok & (d0 < 0)).sum() >= overlapping
    # the cost: differences of the float64 hinge cost on the rows the fixture lists, formed from its own distances
    f = nsg.fixture()
    d0, dp, dm = f['r_d0'], f['r_dplus'], f['r_dminus']
    c = (nsg.cost(np.moveaxis(dp, -1, 1)) - nsg.cost(np.moveaxis(dm, -1, 1))) / (2 * nsg.H)
    assert np.array_equal(c, f['r_cost_fd'])
    rows_ok = (np.abs(d0 - nsg.MARGIN) >= nsg.NEAR_MARGIN).all(1) & (_file('r')[4] | ~(d0 < nsg.MARGIN)).all(1)
    assert np.array_equal(rows_ok, f['r_cost_rows'])
    # ... and they agree with the analytic sum over the restatement's gradients within TOL_G times the sum of the hinge terms
    an = nsg.cost_gradient(d0, f['r_formula'])
    bound = float(f['tol_g']) * np.maximum(nsg.MARGIN - d0, 0.0).sum(1) + 1e-9
    assert (np.abs(an - c).max(1) <= bound)[rows_ok].all(), (np.abs(an - c).max(1) / bound)[rows_ok]
