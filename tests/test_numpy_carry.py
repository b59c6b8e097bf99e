"""CPU tests of the float64 reference of the posture queries with carried objects (tests/numpy_carry.py): the reference alone -- a
carried object keeps its pose in its link's frame, its distance to its own link does not depend on the joints, the committed
differences are what the reference computes -- and the conditions on the fixture that tests/test_gpu_carry.py leans on."""
import numpy as np

from tests import numpy_carry as nc
from tests import numpy_distance as nd
from tests import numpy_posture as npo
from tests import numpy_signed_gradient as nsg
from tests import numpy_step as ns
from tests.golden import make_carry


def _align(q, like):
    return q * np.where((q * like).sum(-1, keepdims=True) < 0, -1.0, 1.0)


def test_inputs():
    st, po, links, given = nc.inputs()
    assert st.shape == (5, 61) and st.dtype == np.float32 and po.shape == (5, 3, 11) and po.dtype == np.float32 and po.flags.c_contiguous
    assert links.tolist() == [[-1, -1, -1], [8, -1, -1], [10, 4, -1], [8, 8, 8], [-1, -1, 8]] and given.shape == (5, 3, 7)
    lim = ns.model()['body_limits']
    assert (po >= lim.min(1).astype(np.float32)).all() and (po <= lim.max(1).astype(np.float32)).all()
    assert np.abs(po - st[:, None, :11]).max() <= 0.5 + 1e-6 and np.abs(po - st[:, None, :11]).max() > 0.4
    assert len(nc.seven_pairs()) == 7 and len(nc.two_pairs()) == 2 and 7 % 4 != 0
    mv = nc.moved_posture()
    assert mv.shape == (5, 1, 11) and (np.abs(mv[:, 0, 1] - st[:, 1]) >= 0.3).all() and (np.delete(mv[:, 0], 1, axis=1) == np.delete(st[:, :11], 1, axis=1)).all()
    # the body that carries: link 8 hangs on body 6, finger_01 on body 8, link 4 on body 3; the masks follow
    mA, mB = nc.masks(links, nc.seven_pairs(), nc.K)
    anc = ns.model()['anc']
    assert mA.shape == (15, 7, 11) and not np.delete(mA[:3], 5, axis=1).any() and (mA[:3, 5] == anc[4]).all() and (mA[3, 0] == anc[6]).all() and (mA[6, 1] == anc[8]).all() and (mA[6, 4] == anc[3]).all()
    assert (mB[9, 6] == anc[6]).all() and (mA[9, 6] == anc[6]).all() and (mA[12, 6] == anc[6]).all() and not mB[12, 6].any() and (mB[3, 2] == anc[7]).all()


def test_a_carried_object_keeps_its_pose_in_its_link():
    st, po, links, _ = nc.inputs()
    rel = nc.reference_rel()
    rows = nc.carried_rows(st, po, links, rel)
    assert rows.dtype == np.float64 and rows.shape == (15, 61) and (rows[:, :11] == po.reshape(15, 11)).all()
    back = nc.rel_in_link(rows, links, nc.K).reshape(5, 3, 3, 7)
    err = 0.0
    for e, o in zip(*np.nonzero(links >= 0)):
        for k in range(3):
            err = max(err, np.abs(back[e, k, o, :3] - rel[e, o, :3]).max(), np.abs(_align(back[e, k, o, 3:], rel[e, o, 3:]) - rel[e, o, 3:]).max())
    print('carried poses in their links over the K rows: off by %.3g' % err)
    assert err <= 1e-12
    # a free object's columns are the state's, bit for bit; the given pose of env 4 has nothing to do with the state's
    plain = npo.rows(st.astype(np.float64), po.astype(np.float64))
    for e, o in zip(*np.nonzero(links < 0)):
        assert (rows[3 * e:3 * e + 3, 22 + 13 * o:29 + 13 * o] == plain[3 * e:3 * e + 3, 22 + 13 * o:29 + 13 * o]).all()
    assert np.abs(rows[12:, 48:51] - plain[12:, 48:51]).max() > 0.05
    # captured at the attach posture, the carried rows at that posture are the state's own
    own = nc.carried_rows(st, st[:, None, :11], links, rel)
    cap = nc.CAPTURED.astype(bool)
    assert np.abs(own[cap, 22:25] - st[cap, 22:25]).max() <= 1e-12 and np.abs(own[cap, 35:38] - st[cap, 35:38]).max() <= 1e-12


def test_the_distance_to_its_own_link_does_not_depend_on_the_joints():
    """(cube, link 8's shape) in envs 1 and 3, whose cube link 8 carries: the central differences vanish -- to the reference's noise,
    about 3e-8 m in d (numpy_signed_gradient.H's comment) over 2 H = 2e-3 rad: 3e-5 m/rad --, and without the attachment they do not."""
    st, po, links, _ = nc.inputs()
    rel = nc.reference_rel()
    pair = nc.own_link_pair()
    items = [(3, 0), (9, 0)]
    d0, dp, dm = nc.differences(st, po, links, rel, pair, items)
    cen = nsg.derivatives(d0, dp, dm)[0]
    free = nc.differences(st, po, np.full_like(links, -1), rel, pair, items)
    cfree = nsg.derivatives(*free)[0]
    print('carried by its own link: |central| %.3g; free: %.3g' % (np.abs(cen[[3, 9], 0]).max(), np.abs(cfree[[3, 9], 0]).max()))
    assert np.abs(cen[[3, 9], 0]).max() <= 3e-5 and np.abs(cfree[[3, 9], 0]).max() > 0.05


def test_the_fixture_decides_enough():
    """measured: 54 items with an attached shape, 38 separated and 16 overlapping decided, none undecided; every row's nearest pair decided"""
    st, po, links, _ = nc.inputs()
    ref = nc.reference()
    att = nc.attached_items(links, nc.seven_pairs(), nc.K)
    dec = ref['decided']
    sep, ov, und = int((att & dec & (ref['d'] > 0)).sum()), int((att & dec & (ref['d'] < 0)).sum()), int((att & ~dec).sum())
    j, rowdec = npo.nearest(ref)
    print('attached items', int(att.sum()), 'separated', sep, 'overlapping', ov, 'undecided', und, 'decided rows', rowdec.reshape(5, 3).sum(1).tolist())
    assert att.sum() == 54 and not att[:3].any() and att[3].tolist() == [True, True, True, True, False, False, True] and att[12].tolist() == [False] * 6 + [True]
    assert sep >= 10 and ov >= 10 and und <= 0.1 * att.sum()
    assert (rowdec.reshape(5, 3).sum(1) >= 1).all()                      # a decided nearest / deepest row per attachment pattern
    # the deepest pair by the signed distance too (what signed_distance reduces): strictly deepest by a millimetre
    srt = np.sort(ref['d'], 1)
    assert ((srt[:, 1] - srt[:, 0] >= nd.DECIDE).reshape(5, 3).sum(1) >= 1).all()
    # the carried objects move: with the attachments ignored the reference is off by centimetres on most attached items
    plain = nd.reference(npo.rows(st, po), nc.seven_pairs())
    off = np.abs(plain['d'] - ref['d'])
    print('attachments ignored: off by more than 1 cm on %d of %d attached items, nowhere else by more than %.3g' % ((off[att] > 0.01).sum(), att.sum(), off[~att].max()))
    assert (off[att] > 0.01).sum() >= 30 and off[~att].max() == 0.0
    # "it moves": (cube, table) of env 1 at the moved posture against the cube left where it was
    mv = nc.moved_posture()
    a = nc.reference(pairs=nc.two_pairs(), postures=mv)['d'][1, 0]
    b = nd.reference(npo.rows(st, mv), nc.two_pairs())['d'][1, 0]
    print('(cube, table) of env 1 at the moved posture: carried %.4f m, left behind %.4f m' % (a, b))
    assert abs(a - b) > 0.01 and abs(a) >= nd.DECIDE and abs(b) >= nd.DECIDE


def test_the_committed_differences():
    g = nc.golden()
    st, po, links, _ = nc.inputs()
    pairs = nc.seven_pairs()
    att = nc.attached_items(links, pairs, nc.K)
    assert g['d0'].shape == (15, 7) and g['dplus'].shape == (15, 7, 11) and (np.isnan(g['d0']) == ~att).all()
    assert np.abs(g['d0'] - nc.reference()['d'])[att].max() <= 1e-12
    # one item recomputed: (cube, finger_00) of env 2's second row, the cube on finger_01
    d0, dp, dm = nc.differences(st, po, links, nc.reference_rel(), pairs, [(7, 2)])
    assert max(abs(d0[7, 2] - g['d0'][7, 2]), np.abs(dp[7, 2] - g['dplus'][7, 2]).max(), np.abs(dm[7, 2] - g['dminus'][7, 2]).max()) <= 1e-9
    # the float64 formula with the carried masks against the differences: tol_g is four times their largest disagreement
    ok, err, items = make_carry.formula_error(g['d0'], g['dplus'], g['dminus'])
    print('%d compared items (%d overlapping): formula against differences %.3g m/rad, tol_g %.3g' % (ok.sum(), (ok & (g['d0'] < 0)).sum(), err.max(), float(g['tol_g'])))
    assert ok.sum() >= 40 and (ok & (g['d0'] < 0)).sum() >= 10 and abs(4 * err.max() - float(g['tol_g'])) <= 1e-9 and float(g['tol_g']) <= 1e-5
    # ... and with the carried objects' masks left out (the original kernel's rule) the formula is far off
    mA, mB = nsg.masks(pairs)
    rows = nc.carried_rows(st, po, links, nc.reference_rel())
    W = nsg.witnesses(rows, pairs, items)
    r, j = np.array([i[0] for i in items]), np.array([i[1] for i in items])
    cen = nsg.derivatives(g['d0'], g['dplus'], g['dminus'])[0]
    wrong = np.abs(nsg.formula(rows[r, :11], W['a'], W['b'], W['n'], mA[j], mB[j]) - cen[r, j]).max(-1)
    assert (wrong > 0.01).sum() >= 20
