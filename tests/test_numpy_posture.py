"""CPU tests of the float64 reference of the posture clearance queries (tests/numpy_posture.py): conditions on the GPU tests' inputs,
from the reference alone -- enough decided items and decided nearest rows of both kinds, several winning pairs, a cull that culls,
negative controls that are far off -- and the reduction rule on synthetic arrays."""
import numpy as np

from tests import numpy_distance as nd
from tests import numpy_posture as npo


def test_inputs_of_case_r():
    st, po, pairs = npo.case_r_inputs()
    assert st.shape == (4, 61) and po.shape == (4, 4, 11) and po.dtype == np.float32 and po.flags.c_contiguous and pairs.shape == (80, 2)
    r = npo.rows(st, po)
    assert r.shape == (16, 61) and (r[:, :11] == po.reshape(16, 11)).all() and (r[5, 11:] == st[1, 11:]).all() and (r[15, 11:] == st[3, 11:]).all()


def test_case_r_decides_enough():
    """measured: 100 % of the items decided; 15 of 16 nearest rows (4 overlapping, 11 separated) over 9 winning pairs"""
    ref = npo.case_r()
    j, dec = npo.nearest(ref)
    m = npo.clearance(ref).min(axis=1)
    print('decided share', ref['decided'].mean(), 'rows', int(dec.sum()), 'overlapping', int((dec & (m == 0)).sum()), 'separated',
          int((dec & (m > 0)).sum()), 'pairs', len(set(j[dec].tolist())))
    assert ref['d'].shape == (16, 80) and ref['decided'].mean() >= 0.9
    assert dec.sum() >= 12 and (dec & (m == 0)).sum() >= 2 and (dec & (m > 0)).sum() >= 5
    assert len(set(j[dec].tolist())) >= 5


def test_case_r_with_a_cull():
    """measured at max_distance = 0.05: 15 of 16 nearest rows over 7 winning pairs, about 1 100 culled items"""
    ref = npo.case_r(max_distance=0.05)
    j, dec = npo.nearest(ref)
    print('rows', int(dec.sum()), 'pairs', len(set(j[dec].tolist())), 'culled', int(ref['culled'].sum()))
    assert dec.sum() >= 12 and len(set(j[dec].tolist())) >= 5 and ref['culled'].sum() >= 500
    st, po, pairs = npo.case_r_inputs()
    direct = nd.reference(npo.rows(st, po)[:2], pairs, max_distance=0.05)           # the derived cull is numpy_distance's own
    for k in ('culled', 'decided', 'expect', 'd', 'gap'):
        assert (direct[k] == ref[k][:2]).all(), k


def test_negative_controls_are_far_off():
    """measured: neighbour's posture 1.39 m, neighbour env's postures 1.54 m, posture ignored 1.81 m; the smallest of the four
    variants of numpy_distance (first_64_vertices_only) 0.025 m"""
    ref = npo.case_r()
    for c in npo.CONTROLS:
        err = nd.control_error(ref, npo.case_r(control=c))
        print(c, err)
        assert err > 0.01, (c, err)
    for v in nd.VARIANTS:
        err = nd.control_error(ref, npo.case_r(variant=v))
        print(v, err)
        assert err > 0.01, (v, err)


def test_grid_case_decides_enough():
    """measured: 134 of 134"""
    ref = npo.grid_case()
    print('grid decided', int(ref['decided'].sum()))
    assert ref['d'].shape == (134, 1) and ref['decided'].sum() >= 120


def _ref(d, gap=None, culled=None, decided=None):
    d = np.asarray(d, dtype=np.float64)
    return dict(d=d, gap=d - 0.01 if gap is None else np.asarray(gap, dtype=np.float64), culled=np.zeros(d.shape, bool) if culled is None else np.asarray(culled),
                decided=np.abs(d) >= nd.DECIDE if decided is None else np.asarray(decided))


def test_nearest_on_synthetic_rows():
    j, dec = npo.nearest(_ref([[0.3, 0.1, 0.2],            # one strict minimum
                               [0.3, -0.02, -0.05],        # two overlapping pairs tie at 0: the lower index
                               [0.1, 0.1004, 0.5],         # two within a millimetre: undecided
                               [0.3, 0.0005, 0.2],         # the minimum is itself undecided (nearer than 1 mm to touching)
                               [-0.0002, -0.05, 0.2]]))    # the tie at 0 holds an undecided item
    assert j[:2].tolist() == [1, 1] and dec.tolist() == [True, True, False, False, False]
    # a culled pair takes part with its sphere gap
    j, dec = npo.nearest(_ref([[0.30, 0.20]], gap=[[0.10, 0.15]], culled=[[True, False]], decided=[[True, True]]))
    assert j.tolist() == [0] and dec.tolist() == [True]


def test_reduction_rule_on_synthetic_rows():
    nan, inf = np.nan, np.inf
    d = np.array([[0.0, 0.0, 0.1], [0.2, 0.0, 0.0], [nan, 0.3, 0.3], [0.3, nan, 0.1], [nan, nan, nan], [inf, inf, 5.0], [inf, nan, inf]])
    assert npo.first_minimum(d).tolist() == [0, 1, 1, 2, 0, 2, 0]
    clean = np.random.default_rng(5).uniform(0, 1, size=(3, 4, 7)).astype(np.float32)
    assert (npo.first_minimum(clean) == clean.argmin(-1)).all() and npo.first_minimum(clean).shape == (3, 4)
