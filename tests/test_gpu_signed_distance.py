"""GPU tests (-m gpu) of the signed-distance queries (rr_signed_distance, include/realrobot.h): penetration depth, direction, witness
points and bound of overlapping hulls against the float64 reference (tests/numpy_penetration.py: qhull on the Minkowski difference),
the separated and culled items against tests/numpy_distance.py, the negative controls, bit identity between calls, batch sizes,
tables, tensors, forks and the two forms of the query, that the query has no effect on the simulation, and the API.

Tolerances.  Separated and culled items are held to every bound of numpy_distance.compare with tests/test_gpu_distance.py's TOL.
Overlapping items are held to TOL_SD, by the same protocol: MEASURED is the largest |-signed - exact depth| over the decided
overlapping items (|depth| >= 1 mm) of test 1 on the MI355X, measured against the float64 reference, never against the device, and
TOL_SD is four times that (the factor covers other seeds and compiler versions).  It must stay below a tenth of the smallest error a
negative control shows (0.45 mm: face_normals_only in case 5); test_negative_controls asserts it.
profiles/signed_distance_bench.json carries both figures."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_collide as ncol
from tests import numpy_distance as nd
from tests import numpy_penetration as pen
from tests import numpy_posture as npo
from tests.test_gpu_distance import TOL as TOL_DIST

pytestmark = pytest.mark.gpu

U = np.uint32
MEASURED = 6.52e-8            # m: the largest |-signed - exact| over the 53 decided overlapping items of test 1 on the MI355X (4.59e-8 in case 1, 6.52e-8 in case 5, 5.69e-8 in case R)
TOL_SD = 4 * MEASURED
RECORD = ('distance', 'bound', 'point_a', 'point_b', 'normal', 'status', 'body_a', 'body_b')      # the deepest record without the pair index
PER_PAIR = ('pair_distance', 'pair_status', 'pair_iterations', 'pair_expansions')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _same(x, y, rows=None, keys=None):
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    return all((_bits(sel(x[k])) == _bits(sel(y[k]))).all() for k in (keys or x))


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _report(where, fig, fails):
    print(where, {k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in fig.items()}, fails)


def _env(N, nobj=3):
    return BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)


def _item_cols(out):
    """the per-pair records of a present-state result under the names numpy_distance.compare / numpy_penetration.compare read"""
    return dict(distance=out['pair_distance'], lower=out['pair_bound'], bound=out['pair_bound'], point_a=out['pair_point_a'], point_b=out['pair_point_b'],
                normal=out['pair_normal'], status=out['pair_status'], expansions=out['pair_expansions'])


_device = {}


def _present(name):
    """(state, pairs, reference, device result) of the present-state cases '1' and '5': the device is asked once per process."""
    st, pairs, ref = nd.case(int(name))
    if name not in _device:
        env = _env(len(st))
        env.state = st
        env.set_distance_pairs(pairs)
        _device[name] = _copy(env.signed_distance(host=True))
        env.close()
    return st, pairs, ref, _device[name]


def _case_r():
    """(state, postures, pairs, reference [16 rows], the posture query's result [4, 4, ...], the per-pair records [16, 80, ...] of four
    present-state queries with posture k written into the state)."""
    st, po, pairs = npo.case_r_inputs()
    if 'R' not in _device:
        env = _env(4)
        env.state = st
        env.set_distance_pairs(pairs)
        query = _copy(env.signed_distance(po, host=True))
        rows = npo.rows(st, po).reshape(4, 4, 61)
        per = []
        for k in range(4):
            env.state = np.ascontiguousarray(rows[:, k])
            per.append(_copy(env.signed_distance(host=True)))
        env.close()
        rec = {key: np.stack([p[key] for p in per], 1) for key in per[0]}                                # [4, 4, ...]
        _device['R'] = (query, {key: v.reshape((16,) + v.shape[2:]) for key, v in rec.items()})
    return (st, po, pairs, npo.case_r()) + _device['R']


def _well_formed(out, pairs):
    """what holds on EVERY row of a clean run, decided or not: out is a result with the leading axes flattened to R rows"""
    R, Q = out['pair_distance'].shape
    rows = np.arange(R)
    assert out['pair'].dtype == np.int32 and (out['pair'] >= 0).all() and (out['pair'] < Q).all()
    assert (out['pair'] == npo.first_minimum(out['pair_distance'])).all()                              # the first minimum of the device's own row
    assert (_bits(out['distance']) == _bits(out['pair_distance'][rows, out['pair']])).all()
    assert (out['status'] == out['pair_status'][rows, out['pair']]).all()
    body = np.array([ncol.body_id(s) for s in ncol.shapes()])
    assert (out['body_a'] == body[pairs[out['pair'], 0]]).all() and (out['body_b'] == body[pairs[out['pair'], 1]]).all()
    st, it, ex = out['pair_status'], out['pair_iterations'], out['pair_expansions']
    assert np.isin(st, (0, 1, 2, 3, 4, 5)).all() and it.max() <= 32 and ex.max() <= 32
    assert (it[st == 2] == 0).all() and (it[st != 2] >= 1).all() and (ex[np.isin(st, (0, 2, 3))] == 0).all() and (ex[np.isin(st, (1, 5))] >= 1).all()
    neg = out['pair_distance'] < 0
    assert np.isin(st[neg], (1, 5)).all() and (out['pair_distance'][st == 4] == 0).all()
    if 'pair_point_a' in out:                                                                          # the deepest row carries that pair's record, bit for bit
        for key, col in (('bound', 'pair_bound'), ('point_a', 'pair_point_a'), ('point_b', 'pair_point_b'), ('normal', 'pair_normal')):
            assert (_bits(out[key]) == _bits(out[col][rows, out['pair']])).all(), key


def _judge(where, cols, ref, pairs, flat, records=True):
    """per-pair records [R, Q, ...] against float64: the overlapping items by numpy_penetration.compare and TOL_SD; the others, with
    test_gpu_distance's TOL, by every bound of numpy_distance.compare in the present-state cases (records) and by status and distance
    -- what the posture form delivers per pair -- in case R"""
    fig, fails = pen.compare(cols, ref, pairs, TOL_SD)
    _report(where + ' overlapping', fig, fails)
    dec = ref['decided']
    if records:
        fig2, fails2 = nd.compare(cols, dict(ref, decided=dec & (ref['expect'] != 1)), TOL_DIST, pairs)
    else:
        sep = dec & (ref['expect'] == 0)
        fig2 = dict(separated=int(sep.sum()), status_mismatches=int((np.asarray(cols['status'])[sep] != 0).sum()),
                    distance_error=float(np.abs(np.asarray(cols['distance'], dtype=np.float64) - ref['d'])[sep].max()))
        fails2 = ['status_mismatches %d > 0' % fig2['status_mismatches']] * (fig2['status_mismatches'] > 0) + \
                 ['distance_error %.3g > %.3g' % (fig2['distance_error'], TOL_DIST)] * (not fig2['distance_error'] <= TOL_DIST)
    _report(where + ' apart', fig2, fails2)
    assert (np.asarray(cols['status'])[dec] != 3).all()
    _well_formed(flat, pairs)
    return fig, fails + fails2


@pytest.mark.parametrize('name', ('1', '5'))
def test_against_float64_present_state(name):
    """case(1): N = 1, the 92 collision pairs (9 overlapping decided items); case(5): N = 5, seven pairs (4)."""
    st, pairs, ref, out = _present(name)
    N, Q = len(st), len(pairs)
    assert out['pair_distance'].shape == (N, Q) and out['pair_point_a'].shape == (N, Q, 3) and out['distance'].shape == (N,) and out['normal'].shape == (N, 3)
    assert out['pair_status'].dtype == np.uint8 and out['pair_expansions'].dtype == np.uint8 and out['status'].dtype == np.int32
    fig, fails = _judge('case ' + name, _item_cols(out), ref, pairs, out)
    assert fig['overlapping'] == {'1': 9, '5': 4}[name]
    assert not fails, fails


def test_against_float64_case_r():
    """N = 4, K = 4, the 80 robot pairs (40 overlapping decided items): the posture query's distances and statuses, and the full
    records of the same 16 rows from present-state queries with the postures written into the state."""
    st, po, pairs, ref, query, rec = _case_r()
    assert query['pair_distance'].shape == (4, 4, 80) and query['distance'].shape == (4, 4) and query['point_a'].shape == (4, 4, 3)
    assert 'pair_point_a' not in query
    flat = {k: v.reshape((16,) + v.shape[2:]) for k, v in query.items()}
    for key in PER_PAIR:                                                                               # the two forms agree bit for bit
        assert (_bits(flat[key]) == _bits(rec[key])).all(), key
    assert _same(flat, rec, keys=RECORD + ('pair',))
    fig, fails = _judge('case R', _item_cols(rec), ref, pairs, rec, records=False)
    assert fig['overlapping'] == 40
    assert not fails, fails
    _well_formed(flat, pairs)


def test_grid_case():
    """N = 67, K = 2, one pair: 134 workgroups, three waves of each without a pair."""
    st, po, pairs = npo.grid_inputs()
    ref = npo.grid_case()
    env = _env(67)
    env.state = st
    env.set_distance_pairs(pairs)
    out = _copy(env.signed_distance(po, host=True))
    env.close()
    assert out['pair_distance'].shape == (67, 2, 1) and (out['pair'] == 0).all()
    flat = {k: v.reshape((134,) + v.shape[2:]) for k, v in out.items()}
    _well_formed(flat, pairs)
    dec, sd, status = ref['decided'], flat['pair_distance'].astype(np.float64), flat['pair_status']
    sep, over = dec & (ref['d'] > 0), dec & (ref['d'] < 0)
    print('grid: decided %d, separated %d, overlapping %d' % (dec.sum(), sep.sum(), over.sum()))
    assert (status[sep] == 0).all() and (status[over] == 1).all()
    assert np.abs(sd - ref['d'])[sep].max() <= TOL_DIST
    if over.any():
        assert np.abs(sd - ref['d'])[over].max() <= TOL_SD
    assert _same({k: flat[k] for k in RECORD}, {'distance': flat['pair_distance'][:, 0], 'bound': flat['bound'], 'point_a': flat['point_a'], 'point_b': flat['point_b'],
                                                'normal': flat['normal'], 'status': flat['pair_status'][:, 0].astype(np.int32), 'body_a': flat['body_a'], 'body_b': flat['body_b']})


@pytest.mark.parametrize('control', pen.CONTROLS)
def test_negative_controls(control):
    """Each wrong restatement, and the face-normals-only search, disagrees with the device's depth by the control's own error, far
    above TOL_SD, in every case where the control applies."""
    from tests.test_numpy_penetration import APPLIES
    smallest = min(pen.control_error(name, c) for c in pen.CONTROLS for name in APPLIES[c])
    assert TOL_SD < 0.1 * smallest, (TOL_SD, smallest)
    for name in APPLIES[control]:
        ref, pairs = pen.case(name)
        rows, cols = pen.overlapping(ref)
        depth = -(_present(name)[3]['pair_distance'] if name != 'R' else _case_r()[5]['pair_distance'])[rows, cols].astype(np.float64)
        err, disagree = pen.control_error(name, control), float(np.abs(depth - pen.control_depths(name, control)).max())
        print('%s case %s: control error %.3g, device against control %.3g' % (control, name, err, disagree))
        assert disagree > TOL_SD and abs(disagree - err) <= TOL_SD and TOL_SD < 0.1 * err


def test_bit_identity():
    import torch
    st, po, pairs, ref, first, _ = _case_r()
    env = _env(4)
    env.state = st
    env.set_distance_pairs(pairs)
    assert _same(first, _copy(env.signed_distance(po, host=True)))                                     # another handle, another call
    assert _same(first, _copy(env.signed_distance(po, host=True)))
    # a CUDA torch tensor read in place against the staged host tensor
    t = torch.from_numpy(po).cuda()
    torch.cuda.synchronize()
    view = env.signed_distance(t)
    dev = {key: torch.from_dlpack(v) for key, v in view.items()}
    env.sync()
    for key, v in dev.items():
        assert v.is_cuda and tuple(v.shape) == first[key].shape and (_bits(v.cpu().numpy()) == _bits(first[key])).all(), key
    # a posture query at the envs' own joints against the present-state query
    own = np.ascontiguousarray(st[:, None, :11])
    at_own, present = _copy(env.signed_distance(own, host=True)), _copy(env.signed_distance(host=True))
    for key in PER_PAIR + RECORD + ('pair',):
        assert (_bits(at_own[key][:, 0]) == _bits(present[key])).all(), key
    # against rr_closest_points / rr_posture_clearance where the hulls do not overlap
    cp, pc = _copy(env.closest_points(host=True)), _copy(env.posture_clearance(po, host=True))
    both = (cp['status'] != 1) & np.isin(present['pair_status'], (0, 2, 3))
    assert both.sum() >= 200 and np.abs(cp['distance'].astype(np.float64) - present['pair_distance'])[both].max() <= TOL_DIST
    bothk = (pc['pair_status'] != 1) & np.isin(first['pair_status'], (0, 2, 3))
    assert bothk.sum() >= 1000 and np.abs(pc['pair_distance'].astype(np.float64) - first['pair_distance'])[bothk].max() <= TOL_DIST
    dec = ref['decided'].reshape(4, 4, 80)
    assert (first['pair_status'][dec] == pc['pair_status'][dec]).all() and (first['pair_distance'][dec & (pc['pair_status'] == 1)] < 0).all()
    # sd_pair's first half is rr_dist.inc's dist_pair restated: the same bits, and the same full record where both write one
    assert (_bits(cp['distance']) == _bits(present['pair_distance']))[both].all()
    assert (_bits(pc['pair_distance']) == _bits(first['pair_distance']))[bothk].all()
    points, sd_points = env.distance_buffer(0, host=True), env.signed_buffer('points', host=True)      # RR_DIST_POINTS, RR_SD_POINTS: [4, 80, 12]
    assert points.shape == sd_points.shape == (4, 80, 12) and (_bits(points) == _bits(sd_points))[both].all()
    # a permuted pair table: permuted columns, permuted back
    perm = np.random.default_rng(3).permutation(80)
    inv = np.argsort(perm)
    env.set_distance_pairs(pairs[perm])
    shuffled = _copy(env.signed_distance(po, host=True))
    for key in PER_PAIR:
        assert (_bits(shuffled[key][..., inv]) == _bits(first[key])).all(), key
    srt = np.sort(first['pair_distance'], -1)
    strict = srt[..., 0] < srt[..., 1]
    assert strict.sum() >= 8 and (shuffled['pair'][strict] == inv[first['pair'][strict]]).all() and _same(shuffled, first, rows=strict, keys=RECORD)
    env.close()
    # N = 5 inside N = 67 (the present state, seven pairs), and forks
    s5, p7, _, five = _present('5')
    N = 67
    s67 = nd.states(N, 117)
    s67[10:15] = s5
    big = _env(N)
    big.state = s67
    big.set_distance_pairs(p7)
    full = _copy(big.signed_distance(host=True))
    assert _same({k: v[10:15] for k, v in full.items()}, five)
    src = np.full(N, -1, np.int32)
    src[[3, 8, 66]] = [20, 12, 14]
    big.fork(src)
    forked = _copy(big.signed_distance(host=True))
    for d, s in ((3, 20), (8, 12), (66, 14)):
        assert _same({k: v[d] for k, v in forked.items()}, {k: v[s] for k, v in full.items()}), (d, s)
    assert _same(forked, full, rows=np.setdiff1d(np.arange(N), [3, 8, 66]))
    big.close()


def _pointers(env, call='rr_signed_buffer', count=5):
    out = []
    for w in range(count):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(getattr(env.L, call)(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_no_effect_on_the_simulation():
    """Queries of both forms between steps leave the state, the preparation record, the error flags, the RR_DIST_* and RR_PC_* buffers
    and every later step bit-identical to those of a twin that never asked."""
    from real_robots_amd.distributed import synthetic_actions
    a, b = _env(8), _env(8)
    a.reset()
    b.reset()
    pairs = npo.robot_pairs()
    po = np.ascontiguousarray(nd.states(24, 121)[:, :11].reshape(8, 3, 11))
    for env in (a, b):
        env.set_distance_pairs(pairs, 0.25)
    for t in range(30):
        cmd = synthetic_actions(list(range(8)), t)
        a.step(cmd, render=(t == 29))
        b.step(cmd, render=(t == 29))
        if t == 12:
            for env in (a, b):
                env.closest_points()
                env.posture_clearance(po)
            before = [b.host(f).tobytes() for f in (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS)] + \
                     [b.distance_buffer(w, host=True).tobytes() for w in range(2)] + [b.posture_buffer(w, host=True).tobytes() for w in range(4)]
            b.signed_distance()
            b.signed_distance(po, host=True)
            after = [b.host(f).tobytes() for f in (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS)] + \
                    [b.distance_buffer(w, host=True).tobytes() for w in range(2)] + [b.posture_buffer(w, host=True).tobytes() for w in range(4)]
            assert before == after
        elif t % 3 == 0:
            b.signed_distance(po if t % 2 else None, host=(t % 4 == 0))
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    for f in (nat.F_ERRFLAGS, nat.F_TOUCH, nat.F_RGB, nat.F_DEPTH, nat.F_STATE):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert (b.signed_buffer('signed', host=True) != 0).any()
    a.close()
    b.close()


def test_api():
    import torch
    N = 5
    env = _env(N)
    L = env.L
    good = np.ascontiguousarray(nd.states(N * 2, 122)[:, :11].reshape(N, 2, 11))
    pcs = _pointers(env, 'rr_posture_buffer', 4)
    # an empty pair table is refused, by the library and by the binding, for both forms
    for args in ((None, 0, 0), (good.ctypes.data, 2, 0)):
        assert L.rr_signed_distance(env.h, *args) == -1 and 'rr_signed_distance: the pair table is empty' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.signed_distance()
    before = _pointers(env)
    assert [n for _, n in before] == [0, 0, 0, 0, 0] and all(p for p, _ in before) and len({p for p, _ in before}) == 5
    n = nd.names()
    p3 = np.array([(n['skin_00'], n['cube']), (n['finger_01'], n['tomato']), (n['lbr_iiwa_link_6'], n['table'])], np.int32)
    env.set_distance_pairs(p3)
    assert [x for _, x in _pointers(env)] == [0, 0, 0, 0, N * 3 * 48]                                  # before the first query K' counts as 0
    # zero-filled before the first query, over the whole allocation
    KM, QM = nat.PC_MAX_POSTURES, nat.DIST_MAX
    env.sync()
    for (p, _), count in zip(before, (N * KM * 12, N * KM * 4, N * KM * QM, N * KM * QM, N * QM * 12)):
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (count,), '<i4', env)).any().item()
    env.state = nd.states(N, 123)
    present = _copy(env.signed_distance(host=True))
    assert [x for _, x in _pointers(env)] == [N * 48, N * 16, N * 3 * 4, N * 3 * 4, N * 3 * 48]
    points = env.signed_buffer('points', host=True).copy()
    assert not _bits(points[..., 11]).any() and not _bits(env.signed_buffer('deepest', host=True)[..., 11]).any()      # the pad column is +0.0
    first = _copy(env.signed_distance(good, host=True))
    sizes = [N * 2 * 48, N * 2 * 16, N * 2 * 3 * 4, N * 2 * 3 * 4, N * 3 * 48]
    assert [x for _, x in _pointers(env)] == sizes
    assert env.signed_buffer('points', host=True).tobytes() == points.tobytes()                         # a posture query leaves RR_SD_POINTS untouched
    raw = env.signed_buffer('status', host=True)
    assert ((raw & 255) == first['pair_status']).all() and (((raw >> 8) & 255) == first['pair_iterations']).all() and ((raw >> 16) == first['pair_expansions']).all()
    # refused calls: RR_EINVAL (-1), the cause named, nothing changes
    for args, word in (((None, 2, 0), 'null postures with n_postures 2'), ((None, -1, 1), 'null postures with n_postures -1'), ((good.ctypes.data, 0, 0), 'n_postures 0'),
                       ((good.ctypes.data, 33, 0), 'n_postures 33'), ((good.ctypes.data, -1, 1), 'n_postures -1')):
        assert L.rr_signed_distance(env.h, *args) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_signed_distance' in msg and word in msg, msg
        assert _pointers(env) == list(zip([p for p, _ in before], sizes))
    p, x = C.c_void_p(), C.c_size_t()
    for which in (5, -1):
        assert L.rr_signed_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_signed_buffer' in L.rr_last_error().decode()
    assert L.rr_signed_copy_to_host(env.h, 0, points.ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    for bad in (good[:, :, :9], good.astype(np.float64), np.zeros((N, 33, 11), np.float32), good[:4]):
        with pytest.raises(ValueError):
            env.signed_distance(bad)
    with pytest.raises(ValueError):
        env.signed_buffer('nearest')
    assert _same(first, _copy(env.signed_distance(good, host=True))) and _same(present, _copy(env.signed_distance(host=True)))
    # DLPack views from torch, both forms
    for arg, host in ((None, present), (good, first)):                                                 # (a later call rewrites the buffers in place)
        dev = {key: torch.from_dlpack(v) for key, v in env.signed_distance(arg).items()}
        env.sync()
        assert set(dev) == set(host)
        for key, v in dev.items():
            assert v.is_cuda and tuple(v.shape) == host[key].shape and (_bits(v.cpu().numpy()) == _bits(host[key])).all(), key
    # pointers stay across K and Q and beside the other queries' buffers; the sizes follow
    k5 = np.ascontiguousarray(nd.states(N * 5, 125)[:, :11].reshape(N, 5, 11))
    env.set_distance_pairs('collision')
    assert env.signed_distance(k5, host=True)['pair_distance'].shape == (N, 5, 92)
    after = _pointers(env)
    assert [p for p, _ in after] == [p for p, _ in before] and [x for _, x in after] == [N * 5 * 48, N * 5 * 16, N * 5 * 92 * 4, N * 5 * 92 * 4, N * 92 * 48]
    assert [p for p, _ in _pointers(env, 'rr_posture_buffer', 4)] == [p for p, _ in pcs]
    env.set_distance_pairs([])
    assert L.rr_signed_distance(env.h, None, 0, 0) == -1 and [p for p, _ in _pointers(env)] == [p for p, _ in before]
    env.close()


def test_non_finite_posture():
    """A NaN posture in one (env, k): the call returns, the stream syncs, every other row is bit for bit the clean run's, and the bad
    row stays well-formed (no loop bound depends on data)."""
    st, po, pairs, _, clean, _ = _case_r()
    env = _env(4)
    env.state = st
    env.set_distance_pairs(pairs)
    bad = po.copy()
    bad[2, 1, 3] = np.nan
    out = _copy(env.signed_distance(bad, host=True))
    env.sync()
    env.close()
    others = np.ones((4, 4), bool)
    others[2, 1] = False
    assert _same(out, clean, rows=others)
    assert 0 <= out['pair'][2, 1] < 80 and np.isin(out['pair_status'][2, 1], (0, 1, 2, 3, 4, 5)).all()
    assert out['pair_iterations'][2, 1].max() <= 32 and out['pair_expansions'][2, 1].max() <= 32
    assert out['status'][2, 1] == out['pair_status'][2, 1, out['pair'][2, 1]]
