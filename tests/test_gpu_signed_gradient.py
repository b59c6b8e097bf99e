"""GPU tests (-m gpu) of the joint gradients of the signed distance (rr_signed_gradient, include/realrobot.h): byte equality of the five
RR_SD_* buffers with rr_signed_distance, the gradients against the header's formula in float64 on the device's own records, against
CENTRAL FINITE DIFFERENCES of the float64 reference (tests/golden/signed_gradient.npz: qhull on the Minkowski difference, no GJK, no
Jacobian), the cost sums, the fixed cases, bit identity, that the query has no effect on the simulation, and the API.

Tolerances.  TOL_G, device against the differences on the compared items (decided and smooth, both read off the reference alone), is
the fixture's: four times the float64 formula's own largest disagreement with the differences.  TOL_F, device against the float64
formula on the device's OWN a, b and n, is four times MEASURED_F, the largest such difference the MI355X showed on the first run of
test_formula_on_the_device_record (float32 frames against float64 ones, a lever of about a metre).  The cost sums are held to the
rounding of a float32 sum of Q terms, (Q + 4) 2^-24 times the sum of the terms' magnitudes."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model
from tests import numpy_distance as nd
from tests import numpy_posture as npo
from tests import numpy_signed_gradient as nsg

pytestmark = pytest.mark.gpu

U = np.uint32
MEASURED_F = 1.09e-7          # m/rad: the largest |device - float64 formula on the device's record| of test_formula_on_the_device_record on the MI355X
                              # (8.33e-8 in case 5, 2.99e-8 on case R's deepest rows, 1.09e-7 over case R's 1280 pair rows)
TOL_F = 4 * MEASURED_F
MARGIN = np.float32(nsg.MARGIN)
GRAD = ('gradient', 'cost', 'cost_gradient')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _same(x, y, keys=None):
    return all((_bits(x[k]) == _bits(y[k])).all() for k in (keys or x))


def _env(N, nobj=3):
    return BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)


def _sd_bytes(env):
    return [env.signed_buffer(i, host=True).tobytes() for i in range(5)]


def _pointers(env, call='rr_signed_gradient_buffer', count=3):
    out = []
    for w in range(count):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(getattr(env.L, call)(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def _sum_tol(terms, axis):
    """the rounding of a float32 sum of Q products (the terms along `axis`) in any fixed order: (Q + 4) half-ulps of the sum of the magnitudes"""
    terms = np.asarray(terms, dtype=np.float64)
    return (terms.shape[axis] + 4) * 2.0 ** -24 * np.abs(terms).sum(axis) + 1e-30


_device = {}


def _case5():
    """(state, pairs, the gradient query's result at the present state, the RR_SD_* bytes behind it and behind rr_signed_distance)"""
    st, pairs, _ = nd.case(5)
    if '5' not in _device:
        env = _env(5)
        env.state = st
        env.set_distance_pairs(pairs)
        env.signed_distance(host=True)
        plain = _sd_bytes(env)
        env.signed_distance(np.zeros((5, 2, 11), np.float32), host=True)           # (other rows in between: the gradient call has to write them all)
        out = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
        _device['5'] = (out, _sd_bytes(env), plain)
        env.close()
    return (st, pairs) + _device['5']


def _case_r():
    """case R: (state, postures, pairs, the result of the posture query [4, 4, ...], of four present-state queries with posture k
    written into the state [4, 4, ...], and the two sets of RR_SD_* bytes)"""
    st, po, pairs = npo.case_r_inputs()
    if 'R' not in _device:
        env = _env(4)
        env.state = st
        env.set_distance_pairs(pairs)
        env.signed_distance(po, host=True)
        plain = _sd_bytes(env)
        env.signed_distance(host=True)
        out = _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True))
        mine = _sd_bytes(env)
        rows = npo.rows(st, po).reshape(4, 4, 61)
        per = []
        for k in range(4):
            env.state = np.ascontiguousarray(rows[:, k])
            per.append(_copy(env.signed_distance_gradient(margin=MARGIN, host=True)))
        env.close()
        _device['R'] = (out, {key: np.stack([p[key] for p in per], 1) for key in per[0]}, mine, plain)
    return (st, po, pairs) + _device['R']


def test_sd_buffers_equal_the_existing_query_byte_for_byte():
    for name, (mine, plain) in (('5', _case5()[3:5]), ('R', _case_r()[5:7])):
        for i, (x, y) in enumerate(zip(mine, plain)):
            if name == 'R' and i == 4:
                continue                                                           # (RR_SD_POINTS: a posture query writes none; the present-state query in between did)
            assert len(x) == len(y) > 0 and x == y, (name, nat.SD_FIELDS[i])
    out = _case5()[2]
    assert set(out) >= set(GRAD) | {'pair_gradient', 'pair_distance', 'pair_normal', 'distance', 'pair'}
    assert out['gradient'].shape == (5, 11) and out['cost'].shape == (5,) and out['cost_gradient'].shape == (5, 11) and out['pair_gradient'].shape == (5, 7, 11)
    r = _case_r()[3]
    assert r['gradient'].shape == (4, 4, 11) and r['cost'].shape == (4, 4) and r['cost_gradient'].shape == (4, 4, 11) and 'pair_gradient' not in r


def test_formula_on_the_device_record():
    """pair_gradient and gradient against the float64 formula on the device's own a, b, n and the float64 frames of numpy_step.forward."""
    st, pairs, out = _case5()[:3]
    mA, mB = nsg.masks(pairs)
    g64 = nsg.formula(st[:, None, :11], out['pair_point_a'], out['pair_point_b'], out['pair_normal'], mA[None], mB[None])
    e5 = float(np.abs(out['pair_gradient'] - g64).max())
    rows = np.arange(5)
    assert (_bits(out['gradient']) == _bits(out['pair_gradient'][rows, out['pair']])).all()           # the deepest row carries that pair's gradient
    st, po, pairs, r, per = _case_r()[:5]
    mA, mB = nsg.masks(pairs)
    g64 = nsg.formula(po, r['point_a'], r['point_b'], r['normal'], mA[r['pair']], mB[r['pair']])
    er = float(np.abs(r['gradient'] - g64).max())
    g64 = nsg.formula(po[:, :, None, :], per['pair_point_a'], per['pair_point_b'], per['pair_normal'], mA[None, None], mB[None, None])
    ep = float(np.abs(per['pair_gradient'] - g64).max())
    print('device against the float64 formula on its own record: case 5 %.3g, case R deepest %.3g, case R all pairs %.3g (TOL_F %.3g); largest |g| %.3g'
          % (e5, er, ep, TOL_F, np.abs(per['pair_gradient']).max()))
    assert np.abs(per['pair_gradient']).max() > 0.5
    assert max(e5, er, ep) <= TOL_F


def test_against_the_differences():
    f = nsg.fixture()
    tol = float(f['tol_g'])
    # the present state: every pair's gradient on the compared items of case 5
    out = _case5()[2]
    cen, fwd, bwd = nsg.derivatives(f['p_d0'], f['p_dplus'], f['p_dminus'])
    ok5 = nsg.compared(f['p_d0'], fwd, bwd)
    e5 = np.abs(out['pair_gradient'] - cen).max(-1)
    print('case 5: %d compared items, device against the differences %.3g (TOL_G %.3g)' % (ok5.sum(), e5[ok5].max(), tol))
    # case R: the deepest pair's gradient on the rows whose deepest pair the reference decides and compares; every pair's gradient
    # (present-state queries with the posture written into the state) on all compared items
    st, po, pairs, r, per = _case_r()[:5]
    d0 = f['r_d0']
    cen, fwd, bwd = nsg.derivatives(d0, f['r_dplus'], f['r_dminus'])
    ok = nsg.compared(d0, fwd, bwd)
    m = d0.min(1)
    S = d0 < (m + nd.DECIDE)[:, None]
    jstar = S.argmax(1)
    rowdec = (S.sum(1) == 1) & ok[np.arange(16), jstar]
    pair = r['pair'].reshape(16)
    assert rowdec.sum() >= 8 and (pair[rowdec] == jstar[rowdec]).all()
    er = np.abs(r['gradient'].reshape(16, 11) - cen[np.arange(16), jstar]).max(-1)
    ep = np.abs(per['pair_gradient'].reshape(16, 80, 11) - cen).max(-1)
    print('case R: %d decided rows, deepest gradient against the differences %.3g; %d compared items, every pair %.3g (overlapping %d: %.3g)'
          % (rowdec.sum(), er[rowdec].max(), ok.sum(), ep[ok].max(), (ok & (d0 < 0)).sum(), ep[ok & (d0 < 0)].max()))
    # the cost's gradient against differences of the float64 cost, on the fixture's rows: each pair's gradient may be off by TOL_G,
    # each hinge term by the device's distance error (1e-6 m, generous) times a gradient of at most 1
    cfd, crow = f['r_cost_fd'], f['r_cost_rows']
    ec = np.abs(r['cost_gradient'].reshape(16, 11) - cfd).max(-1)
    bound = tol * np.maximum(nsg.MARGIN - d0, 0.0).sum(1) + 1e-6 * (d0 < nsg.MARGIN).sum(1)
    print('case R: cost gradient against the differences on %d rows: %.3g, worst error / bound %.3g' % (crow.sum(), ec[crow].max(), (ec[crow & (bound > 0)] / bound[crow & (bound > 0)]).max()))
    assert e5[ok5].max() <= tol
    assert er[rowdec].max() <= tol and ep[ok].max() <= tol
    assert (ec <= bound)[crow].all()


def test_cost_sums():
    """cost and cost_gradient at margin 0.05 against float64 sums over the device's own signed values and gradients."""
    out = _case5()[2]
    per = _case_r()[4]
    for name, o in (('5', out), ('R', per)):
        d, g = o['pair_distance'].astype(np.float64), o['pair_gradient'].astype(np.float64)
        c = np.maximum(np.float64(MARGIN) - d, 0.0)
        assert (c > 0).sum() >= 5
        eC = np.abs(o['cost'] - nsg.cost(d, np.float64(MARGIN)))
        eG = np.abs(o['cost_gradient'] - nsg.cost_gradient(d, g, np.float64(MARGIN)))
        tC, tG = _sum_tol(0.5 * c * c, -1), _sum_tol(c[..., None] * g, -2)
        print('case %s: cost error %.3g (worst / bound %.3g), cost gradient error %.3g (worst / bound %.3g), largest cost %.3g'
              % (name, eC.max(), (eC / tC).max(), eG.max(), (eG / tG).max(), o['cost'].max()))
        assert (eC <= tC).all() and (eG <= tG).all() and o['cost'].max() > 1e-4
    # the posture form carries the rows of the present-state form, bit for bit
    r = _case_r()[3]
    assert _same(r, per, keys=GRAD)


def test_fixed_cases():
    n = nd.names()
    st = nd.states(5, 36)
    pairs = np.array([(n['lbr_iiwa_link_6'], n['table']), (n['skin_00'], n['cube']), (n['finger_01'], n['lbr_iiwa_link_3']), (n['cube'], n['table'])], np.int32)
    body = nsg.bodies(pairs)
    assert body[0].tolist() == [5, -1] and body[3].tolist() == [-1, -1]
    env = _env(5)
    env.state = st
    env.set_distance_pairs(pairs)
    out = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    pg = out['pair_gradient']
    # zero columns, as +0.0 bits: the joints behind a forearm link, every joint of a pair of an object and a static shape, the pad
    assert not _bits(pg[:, 0, 6:]).any() and np.abs(pg[:, 0, :6]).max() > 0.05
    assert not _bits(pg[:, 3]).any()
    assert not _bits(env.signed_gradient_buffer('pair_gradient', host=True)[..., 11]).any() and not _bits(env.signed_gradient_buffer('gradient', host=True)[..., 11]).any()
    # a joint that moves both shapes of a robot pair: column 0 turns the whole arm about the vertical through both
    # (n . (a_k x (a - b)) = 0 in exact arithmetic; each half is a float32 sum of six products below 1: four ulps of 1 each)
    assert np.abs(pg[:, 2, 0]).max() <= 8 * 2.0 ** -23 and np.abs(pg[:, 2, 3:]).max() > 0.01
    # margin 0 counts penetrations only
    zero = _copy(env.signed_distance_gradient(margin=0.0, host=True))
    d, g = zero['pair_distance'].astype(np.float64), zero['pair_gradient'].astype(np.float64)
    assert (_bits(zero['pair_gradient']) == _bits(pg)).all()
    apart = (d >= 0).all(1)
    print('margin 0: %d of 5 rows without a penetration; costs %s' % (apart.sum(), zero['cost']))
    assert not _bits(zero['cost'][apart]).any() and not _bits(zero['cost_gradient'][apart]).any()
    assert (np.abs(zero['cost'] - nsg.cost(d, 0.0)) <= _sum_tol(0.5 * np.minimum(d, 0.0) ** 2, -1)).all()
    assert (np.abs(zero['cost_gradient'] - nsg.cost_gradient(d, g, 0.0)) <= _sum_tol(np.minimum(d, 0.0)[..., None] * g, -2)).all()
    # status 2: with a cull the culled pairs report the gradient of the sphere gap -- the formula on the sphere points, which is the
    # formula on the sphere centres (a lever along n adds nothing)
    env.set_distance_pairs(pairs, 0.25)
    cul = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    is2 = cul['pair_status'] == 2
    assert is2.sum() >= 3 and (is2 & (body[None, :, 0] >= 0)).sum() >= 2
    sph = np.array(load_model()['shape_sphere'], dtype=np.float64)
    mA, mB = nsg.masks(pairs)
    nn = cul['pair_normal'].astype(np.float64)
    ca, cb = cul['pair_point_a'] + sph[pairs[:, 0], 3][None, :, None] * nn, cul['pair_point_b'] - sph[pairs[:, 1], 3][None, :, None] * nn
    g64 = nsg.formula(st[:, None, :11], ca, cb, nn, mA[None], mB[None])
    print('status 2: %d items, gradient of the sphere gap off by %.3g' % (is2.sum(), np.abs(cul['pair_gradient'] - g64)[is2].max()))
    assert np.abs(cul['pair_gradient'] - g64)[is2].max() <= TOL_F
    assert (_bits(cul['pair_gradient'])[~is2] == _bits(pg)[~is2]).all()
    # status 4: the cube moved along the reported normal until it touches the finger pad (a gap of half a micrometre): +0.0 in every column
    env.set_distance_pairs(pairs)
    e = int(np.argmin(np.where(out['pair_status'][:, 1] == 0, out['pair_distance'][:, 1], np.inf)))      # the env whose pad is nearest its cube
    assert out['pair_status'][e, 1] == 0
    touch = st.copy().astype(np.float64)
    touch[e, 22:25] += (out['pair_distance'][e, 1] - 5e-7) * out['pair_normal'][e, 1].astype(np.float64)
    env.state = touch.astype(np.float32)
    t = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    print('status 4: env %d, pair 1: status %d, distance %.3g (from %.3g)' % (e, t['pair_status'][e, 1], t['pair_distance'][e, 1], out['pair_distance'][e, 1]))
    assert t['pair_status'][e, 1] == 4 and not _bits(t['pair_gradient'][e, 1]).any() and np.abs(pg[e, 1]).max() > 0.01
    # ... and it takes part in the cost with c = margin and no gradient
    others = np.delete(np.arange(4), 1)
    d, g = t['pair_distance'][e].astype(np.float64), t['pair_gradient'][e].astype(np.float64)
    assert abs(t['cost'][e] - nsg.cost(d, np.float64(MARGIN))) <= _sum_tol(0.5 * np.maximum(MARGIN - d, 0) ** 2, -1)
    assert (np.abs(t['cost_gradient'][e] - nsg.cost_gradient(d[others], g[others], np.float64(MARGIN))) <= _sum_tol(np.maximum(MARGIN - d, 0)[:, None] * g, -2)).all()
    env.close()


def test_determinism_and_independence():
    import torch
    st, po, pairs, first, per = _case_r()[:5]
    env = _env(4)
    env.state = st
    env.set_distance_pairs(pairs)
    assert _same(first, _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True)))               # another handle, another call
    assert _same(first, _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True)))
    # a CUDA torch tensor read in place against the staged host tensor
    t = torch.from_numpy(po).cuda()
    torch.cuda.synchronize()
    dev = {key: torch.from_dlpack(v) for key, v in env.signed_distance_gradient(t, margin=MARGIN).items()}
    env.sync()
    for key, v in dev.items():
        assert v.is_cuda and tuple(v.shape) == first[key].shape and (_bits(v.cpu().numpy()) == _bits(first[key])).all(), key
    # a posture query at the envs' own joints against the present-state query
    own = np.ascontiguousarray(st[:, None, :11])
    at_own, present = _copy(env.signed_distance_gradient(own, margin=MARGIN, host=True)), _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    for key in GRAD:
        assert (_bits(at_own[key][:, 0]) == _bits(present[key])).all(), key
    # a permuted pair table: permuted pair_gradient rows; the deepest gradient follows where the minimum is strict
    perm = np.random.default_rng(3).permutation(80)
    inv = np.argsort(perm)
    env.set_distance_pairs(pairs[perm])
    shuffled = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    assert (_bits(shuffled['pair_gradient'][:, inv]) == _bits(present['pair_gradient'])).all()
    srt = np.sort(present['pair_distance'], -1)
    strict = srt[..., 0] < srt[..., 1]
    assert strict.any() and (_bits(shuffled['gradient'][strict]) == _bits(present['gradient'][strict])).all()
    d, g = shuffled['pair_distance'].astype(np.float64), shuffled['pair_gradient'].astype(np.float64)          # (another order of the same terms)
    assert (np.abs(shuffled['cost_gradient'] - present['cost_gradient']) <= 2 * _sum_tol(np.maximum(MARGIN - d, 0)[..., None] * g, -2)).all()
    env.close()
    # the grid case: N = 67, K = 2, one pair (three waves of a workgroup without a pair) against the same items at N = 1
    st, po, pairs = npo.grid_inputs()
    big = _env(67)
    big.state = st
    big.set_distance_pairs(pairs)
    wide = np.float32(0.5)                                                                                # (a margin that many of these pad-to-cube distances are inside)
    grid = _copy(big.signed_distance_gradient(po, margin=wide, host=True))
    big.close()
    c = np.maximum(wide - grid['distance'], np.float32(0))                                              # one pair: the sums have one term
    assert grid['gradient'].shape == (67, 2, 11) and (grid['cost_gradient'] == -(c[..., None] * grid['gradient'])).all() and (grid['cost'] == np.float32(0.5) * c * c).all()
    one = _env(1)
    one.set_distance_pairs(pairs)
    for e in (0, 33, 66):
        one.state = st[e:e + 1]
        single = _copy(one.signed_distance_gradient(po[e:e + 1], margin=wide, host=True))
        for key in GRAD + ('distance', 'normal'):
            assert (_bits(single[key][0]) == _bits(grid[key][e])).all(), (e, key)
    one.close()
    assert np.abs(grid['gradient']).max() > 0.05 and (grid['cost'] > 0).sum() >= 20


def test_no_effect_on_the_simulation():
    """N = 8: 20 steps with a gradient call between every two steps give the state bytes of 20 steps without."""
    from real_robots_amd.distributed import synthetic_actions
    a, b = _env(8), _env(8)
    a.reset()
    b.reset()
    po = np.ascontiguousarray(nd.states(24, 121)[:, :11].reshape(8, 3, 11))
    b.set_distance_pairs(npo.robot_pairs())
    for t in range(20):
        cmd = synthetic_actions(list(range(8)), t)
        a.step(cmd)
        b.step(cmd)
        if t == 7:
            before = [b.host(f).tobytes() for f in (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS)]
            b.signed_distance_gradient(po, margin=MARGIN, host=True)
            b.signed_distance_gradient(margin=MARGIN)
            assert before == [b.host(f).tobytes() for f in (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS)]
        else:
            b.signed_distance_gradient(po if t % 2 else None, margin=MARGIN, host=(t % 4 == 0))
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    for f in (nat.F_STATE, nat.F_ERRFLAGS, nat.F_TOUCH):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    assert (b.signed_gradient_buffer('cost', host=True) != 0).any()
    a.close()
    b.close()


def test_refusals_and_buffer_life():
    import torch
    N = 5
    env = _env(N)
    L = env.L
    good = np.ascontiguousarray(nd.states(N * 2, 122)[:, :11].reshape(N, 2, 11))
    # an empty pair table is refused, by the library and by the binding
    for args in ((None, 0, 0, 0.0), (good.ctypes.data, 2, 0, 0.0)):
        assert L.rr_signed_gradient(env.h, *args) == -1 and 'rr_signed_gradient: the pair table is empty' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.signed_distance_gradient()
    before = _pointers(env)
    assert [n for _, n in before] == [0, 0, 0] and all(p for p, _ in before) and len({p for p, _ in before}) == 3
    sd = _pointers(env, 'rr_signed_buffer', 5)
    n = nd.names()
    p3 = np.array([(n['skin_00'], n['cube']), (n['finger_01'], n['tomato']), (n['lbr_iiwa_link_6'], n['table'])], np.int32)
    env.set_distance_pairs(p3)
    assert [x for _, x in _pointers(env)] == [0, 0, N * 3 * 48]                                         # before the first query K' counts as 0
    KM, QM = nat.PC_MAX_POSTURES, nat.DIST_MAX
    env.sync()
    for (p, _), count in zip(before, (N * KM * 12, N * KM * 12, N * QM * 12)):                          # zero-filled over the whole allocation
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (count,), '<i4', env)).any().item()
    env.state = nd.states(N, 123)
    present = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    assert [x for _, x in _pointers(env)] == [N * 48, N * 48, N * 3 * 48]
    pg = env.signed_gradient_buffer('pair_gradient', host=True).copy()
    first = _copy(env.signed_distance_gradient(good, margin=MARGIN, host=True))
    sizes = [N * 2 * 48, N * 2 * 48, N * 3 * 48]
    assert [x for _, x in _pointers(env)] == sizes
    assert [x for _, x in _pointers(env, 'rr_signed_buffer', 5)] == [N * 2 * 48, N * 2 * 16, N * 2 * 3 * 4, N * 2 * 3 * 4, N * 3 * 48]
    assert env.signed_gradient_buffer('pair_gradient', host=True).tobytes() == pg.tobytes()              # a posture query leaves RR_SG_PAIR_GRADIENT untouched
    # refused calls: RR_EINVAL (-1), the cause named, pointers and sizes unchanged
    cases = [((None, 2, 0, 0.0), 'null postures with n_postures 2'), ((good.ctypes.data, 0, 0, 0.0), 'n_postures 0'), ((good.ctypes.data, 33, 0, 0.0), 'n_postures 33'),
             ((good.ctypes.data, -1, 1, 0.0), 'n_postures -1'), ((None, 0, 0, float('nan')), 'margin'), ((None, 0, 0, float('inf')), 'margin'),
             ((good.ctypes.data, 2, 0, -1e-3), 'margin')]
    for args, word in cases:
        assert L.rr_signed_gradient(env.h, *args) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_signed_gradient' in msg and word in msg, msg
        assert _pointers(env) == list(zip([p for p, _ in before], sizes))
    env.set_distance_pairs(p3, 0.04)                                                                     # a cull in force below the margin
    assert L.rr_signed_gradient(env.h, None, 0, 0, 0.05) == -1 and 'max_distance' in L.rr_last_error().decode()
    assert _pointers(env) == list(zip([p for p, _ in before], sizes))
    assert L.rr_signed_gradient(env.h, None, 0, 0, 0.04) == 0
    env.set_distance_pairs(p3)
    p, x = C.c_void_p(), C.c_size_t()
    for which in (3, -1):
        assert L.rr_signed_gradient_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_signed_gradient_buffer' in L.rr_last_error().decode()
    assert L.rr_signed_gradient_copy_to_host(env.h, 0, pg.ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.signed_gradient_buffer('deepest')
    with pytest.raises(ValueError):
        env.signed_distance_gradient(good[:, :, :9])
    assert _same(first, _copy(env.signed_distance_gradient(good, margin=MARGIN, host=True))) and _same(present, _copy(env.signed_distance_gradient(margin=MARGIN, host=True)))
    # DLPack views from torch, both forms
    for arg, host in ((None, present), (good, first)):
        dev = {key: torch.from_dlpack(v) for key, v in env.signed_distance_gradient(arg, margin=MARGIN).items()}
        env.sync()
        assert set(dev) == set(host)
        for key, v in dev.items():
            assert v.is_cuda and tuple(v.shape) == host[key].shape and (_bits(v.cpu().numpy()) == _bits(host[key])).all(), key
    # pointers stay across K and Q and beside the sibling's buffers; the sizes follow
    k5 = np.ascontiguousarray(nd.states(N * 5, 125)[:, :11].reshape(N, 5, 11))
    env.set_distance_pairs('collision')
    assert env.signed_distance_gradient(k5, margin=MARGIN, host=True)['cost_gradient'].shape == (N, 5, 11)
    after = _pointers(env)
    assert [p for p, _ in after] == [p for p, _ in before] and [x for _, x in after] == [N * 5 * 48, N * 5 * 48, N * 92 * 48]
    assert [p for p, _ in _pointers(env, 'rr_signed_buffer', 5)] == [p for p, _ in sd]
    env.set_distance_pairs([])
    assert L.rr_signed_gradient(env.h, None, 0, 0, 0.0) == -1 and [p for p, _ in _pointers(env)] == [p for p, _ in before]
    env.close()
