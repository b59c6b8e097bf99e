"""GPU tests (-m gpu) of the clearance queries at candidate postures (rr_posture_clearance, include/realrobot.h): the four device
buffers against the independent float64 reference (tests/numpy_posture.py: numpy_distance on the substituted state rows, and the
nearest pair where the reference alone decides it); the negative controls; rr_closest_points on a twin handle that is written and
queried posture by posture; bit-identity between calls, K, batch sizes, host and device tensors, permuted tables and forks; the grid
and the limits; the cull; that the query has no effect on the simulation; the API; non-finite input.

Tolerance, by the protocol of tests/test_gpu_distance.py.  TOL bounds |distance - exact| on every DECIDED separated item
(|exact| >= 1 mm) and, through numpy_distance.compare, the nearest records.  It is four times the largest |distance - exact| measured
on the MI355X over the decided items of test 1 (MEASURED; the factor covers other seeds and compiler versions), measured against
numpy_distance.reference, never against the device, and it must stay below a tenth of the smallest error a negative control shows
(test_negative_controls asserts it).  profiles/posture_clearance_bench.json carries the figure."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_collide as ncol
from tests import numpy_distance as nd
from tests import numpy_posture as npo

pytestmark = pytest.mark.gpu

U = np.uint32
MEASURED = 2.12e-7            # m: the largest |distance - exact| over the decided items of test 1 (case R: 1280 of 1280 decided) on the MI355X
TOL = 4 * MEASURED
RECORD = ('distance', 'lower', 'point_a', 'point_b', 'normal', 'status', 'body_a', 'body_b')      # the nearest record without the pair index


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _same(x, y, rows=None, keys=None):
    """two results of posture_clearance(host=True), bit for bit (on the rows given: an index into the leading axes)"""
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    return all((_bits(sel(x[k])) == _bits(sel(y[k]))).all() for k in (keys or x))


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _flat(out):
    """the leading [N, K] of every column flattened to R = N * K rows"""
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in out.items()}


def _report(where, fig, fails):
    print(where, {k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in fig.items()}, fails)


def _env(N, nobj=3):
    return BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)


_device = {}


def _case_r(max_distance=None):
    """(state, postures, pairs, reference, device result [N, K, ...]) of case R: the device is asked once per process."""
    st, po, pairs = npo.case_r_inputs()
    if max_distance not in _device:
        env = _env(4)
        env.state = st
        env.set_distance_pairs(pairs, max_distance)
        _device[max_distance] = _copy(env.posture_clearance(po, host=True))
        env.close()
    return st, po, pairs, npo.case_r(max_distance), _device[max_distance]


def _well_formed(out, pairs):
    """what holds on EVERY row of a clean run, decided or not"""
    f = _flat(out)
    R, Q = f['pair_distance'].shape
    rows = np.arange(R)
    assert f['pair'].dtype == np.int32 and (f['pair'] >= 0).all() and (f['pair'] < Q).all()
    assert (_bits(f['distance']) == _bits(f['pair_distance'][rows, f['pair']])).all()                  # the record's distance is that pair's, bit for bit
    assert (f['pair'] == npo.first_minimum(f['pair_distance'])).all() and (f['pair'] == f['pair_distance'].argmin(-1)).all()      # the first argmin of the device's own row
    assert (f['status'] == f['pair_status'][rows, f['pair']]).all()
    body = np.array([ncol.body_id(s) for s in ncol.shapes()])
    assert (f['body_a'] == body[pairs[f['pair'], 0]]).all() and (f['body_b'] == body[pairs[f['pair'], 1]]).all()
    assert np.isin(f['pair_status'], (0, 1, 2, 3)).all() and f['pair_iterations'].max() <= 32
    assert (f['pair_iterations'][f['pair_status'] == 2] == 0).all() and (f['pair_iterations'][f['pair_status'] != 2] >= 1).all()


def test_against_float64_case_r():
    """N = 4, K = 4, the 80 robot pairs of the collision table: random postures over random object poses and the arranged ones."""
    st, po, pairs, ref, out = _case_r()
    assert out['pair_distance'].shape == (4, 4, 80) and out['pair_status'].shape == (4, 4, 80) and out['pair_status'].dtype == np.uint8
    assert out['distance'].shape == (4, 4) and out['point_a'].shape == (4, 4, 3) and out['pair'].shape == (4, 4) and out['status'].dtype == np.int32
    fig, fails = npo.compare(_flat(out), ref, TOL, pairs)
    _report('case R', fig, fails)
    assert not fails, fails
    assert fig['decided'] >= 0.9 * fig['items'] and fig['decided_rows'] >= 12
    _well_formed(out, pairs)
    env = _env(4)
    env.state = st
    env.set_distance_pairs(pairs)
    env.posture_clearance(po)
    assert not _bits(env.posture_buffer('nearest', host=True)[..., 11]).any()                         # the pad column is +0.0
    raw = env.posture_buffer('status', host=True)
    assert raw.shape == (4, 4, 80) and ((raw & 255) == out['pair_status']).all() and ((raw >> 8) == out['pair_iterations']).all()
    env.close()


@pytest.mark.parametrize('control', npo.CONTROLS + nd.VARIANTS)
def test_negative_controls(control):
    """A reference with the neighbour's posture, the neighbour env's postures or the present joints, and each deliberately wrong
    restatement of numpy_distance, disagrees with the device, by far more than TOL."""
    st, po, pairs, ref, out = _case_r()
    var = npo.case_r(control=control) if control in npo.CONTROLS else npo.case_r(variant=control)
    fig, fails = npo.compare(_flat(out), var, TOL, pairs)
    err = nd.control_error(ref, var)
    _report(control, dict(fig, control_error=err), fails)
    assert fails, control
    assert TOL < 0.1 * err, (TOL, err)


def test_against_closest_points_on_a_written_twin():
    """What a user did before: per posture k, write_state(joint_pos) on a twin handle and closest_points().  The two kernels run one
    pair search (dist_pair, csrc/rr_dist.inc) on the same frames, so every one of the 1 280 items, decided or not, has
    rr_closest_points' distance bits, iterations and status."""
    st, po, pairs, ref, out = _case_r()
    twin = _env(4)
    twin.state = st
    twin.set_distance_pairs(pairs)
    rows = npo.rows(st, po).reshape(4, 4, 61)
    cp = []
    for k in range(4):
        twin.write_state(np.ascontiguousarray(rows[:, k]), np.ones(4, np.uint8), joint_pos=True)
        cp.append(_copy(twin.closest_points(host=True)))
    twin.close()
    dist, status, iters = (np.stack([c[key] for c in cp], 1) for key in ('distance', 'status', 'iterations'))      # [N, K, Q]
    dec = ref['decided'].reshape(4, 4, 80)
    assert (out['pair_status'][dec] == status[dec]).all()
    assert np.abs(out['pair_distance'].astype(np.float64) - dist)[dec].max() <= 2 * TOL
    jstar, rowdec = npo.nearest(ref)
    assert (dist.reshape(16, 80).argmin(-1)[rowdec] == out['pair'].reshape(16)[rowdec]).all() and (out['pair'].reshape(16)[rowdec] == jstar[rowdec]).all()
    assert dist.size == 1280 and (_bits(out['pair_distance']) == _bits(dist)).all()
    assert (iters == out['pair_iterations']).all() and (status == out['pair_status']).all()


def test_bit_identity_of_calls_postures_batches_tensors_tables_and_forks():
    import torch
    st, po, pairs, ref, first = _case_r()
    env = _env(4)
    env.state = st
    env.set_distance_pairs(pairs)
    assert _same(first, _copy(env.posture_clearance(po, host=True)))                                 # another handle, another call
    assert _same(first, _copy(env.posture_clearance(po, host=True)))
    for k in range(4):                                                                               # posture k of K = 4 == the same posture alone
        alone = _copy(env.posture_clearance(np.ascontiguousarray(po[:, k:k + 1]), host=True))
        assert _same({key: v[:, 0] for key, v in alone.items()}, {key: v[:, k] for key, v in first.items()}), k
    # a CUDA torch tensor read in place against the staged host tensor
    t = torch.from_numpy(po).cuda()
    torch.cuda.synchronize()
    view = env.posture_clearance(t)
    dev = {key: torch.from_dlpack(v) for key, v in view.items()}
    env.sync()
    for key, v in dev.items():
        assert v.is_cuda and tuple(v.shape) == first[key].shape and (_bits(v.cpu().numpy()) == _bits(first[key])).all(), key
    # a permuted pair table: permuted columns; the winner's record where the row's minimum is strict
    perm = np.random.default_rng(3).permutation(80)
    inv = np.argsort(perm)
    env.set_distance_pairs(pairs[perm])
    shuffled = _copy(env.posture_clearance(po, host=True))
    for key in ('pair_distance', 'pair_status', 'pair_iterations'):
        assert (_bits(shuffled[key]) == _bits(first[key][..., perm])).all(), key
    srt = np.sort(first['pair_distance'], -1)
    strict = srt[..., 0] < srt[..., 1]
    assert strict.sum() >= 8 and (shuffled['pair'][strict] == inv[first['pair'][strict]]).all()
    assert _same(shuffled, first, rows=strict, keys=RECORD)
    env.close()
    # env 66 of a 67-env handle against a 1-env handle; forks
    N = 67
    s67 = nd.states(N, 117)
    p67 = np.ascontiguousarray(nd.states(N * 4, 118)[:, :11].reshape(N, 4, 11))
    s67[66], p67[66] = st[0], po[0]
    p67[3], p67[8], p67[30] = p67[20], p67[20], p67[66]
    big = _env(N)
    big.state = s67
    big.set_distance_pairs(pairs)
    full = _copy(big.posture_clearance(p67, host=True))
    assert _same({key: v[66] for key, v in full.items()}, {key: v[0] for key, v in first.items()})
    lone = _env(1)
    lone.state = st[:1]
    lone.set_distance_pairs(pairs)
    assert _same({key: v[0] for key, v in _copy(lone.posture_clearance(po[:1], host=True)).items()}, {key: v[66] for key, v in full.items()})
    lone.close()
    src = np.full(N, -1, np.int32)
    src[[3, 8, 30]] = [20, 20, 66]
    big.fork(src)
    forked = _copy(big.posture_clearance(p67, host=True))
    for d, s in ((3, 20), (8, 20), (30, 66)):
        assert _same({key: v[d] for key, v in forked.items()}, {key: v[s] for key, v in full.items()}), (d, s)
    assert _same(forked, full, rows=np.setdiff1d(np.arange(N), [3, 8, 30]))
    big.close()


def test_grid_and_limits():
    """N = 67, K = 2 with one pair against float64 (134 workgroups, a one-pair table: three waves of a workgroup have no pair); K = 32
    at N = 1 with two pairs: every row equals that posture alone."""
    st, po, pairs = npo.grid_inputs()
    ref = npo.grid_case()
    assert ref['decided'].sum() >= 120
    env = _env(67)
    env.state = st
    env.set_distance_pairs(pairs)
    out = _copy(env.posture_clearance(po, host=True))
    env.close()
    assert out['pair_distance'].shape == (67, 2, 1) and (out['pair'] == 0).all()
    fig, fails = npo.compare(_flat(out), ref, TOL, pairs)
    _report('grid', fig, fails)
    assert not fails, fails
    _well_formed(out, pairs)
    n = nd.names()
    two = np.array([(n['finger_01'], n['mustard']), (n['skin_00'], n['cube'])], np.int32)
    p32 = np.ascontiguousarray(nd.states(32, 119)[:, :11].reshape(1, 32, 11))
    one = _env(1)
    one.state = nd.states(1, 120)
    one.set_distance_pairs(two)
    allk = _copy(one.posture_clearance(p32, host=True))
    assert allk['pair_distance'].shape == (1, 32, 2) and len(np.unique(allk['distance'])) >= 16
    for k in range(32):
        alone = _copy(one.posture_clearance(np.ascontiguousarray(p32[:, k:k + 1]), host=True))
        assert _same({key: v[:, 0] for key, v in alone.items()}, {key: v[:, k] for key, v in allk.items()}), k
    _well_formed(allk, two)
    one.close()


def test_cull():
    """max_distance = 5 cm on case R: decided far items have status 2, no iterations and the reference's sphere gap; near items are
    bit for bit those of the call without a cull; the nearest pair is the reference's on decided rows."""
    st, po, pairs, ref, out = _case_r(0.05)
    plain = _case_r()[4]
    fig, fails = npo.compare(_flat(out), ref, TOL, pairs)
    _report('cull', fig, fails)
    assert not fails, fails
    assert fig['decided_rows'] >= 12
    far = out['pair_status'] == 2
    cul = (ref['decided'] & ref['culled']).reshape(far.shape)
    assert cul.sum() >= 500 and far[cul].all() and (out['pair_iterations'][cul] == 0).all()
    assert np.abs(out['pair_distance'].astype(np.float64) - ref['gap'].reshape(far.shape))[cul].max() <= nd.GAP_TOL
    for key in ('pair_distance', 'pair_status', 'pair_iterations'):
        assert (_bits(out[key])[~far] == _bits(plain[key])[~far]).all(), key
    _well_formed(out, pairs)


def test_no_effect_on_the_simulation():
    """40 steps with a query (K = 3) after each leave contact counts, state, touch, error flags, a rendered frame and the checkpoint
    bit-identical to 40 steps without, and the buffers of an interleaved closest_points() too."""
    from real_robots_amd.distributed import synthetic_actions
    a, b = _env(8), _env(8)
    a.reset()
    b.reset()
    pairs = npo.robot_pairs()
    a.set_distance_pairs(pairs, 0.25)
    b.set_distance_pairs(pairs, 0.25)
    po = np.ascontiguousarray(nd.states(24, 121)[:, :11].reshape(8, 3, 11))
    for t in range(40):
        cmd = synthetic_actions(list(range(8)), t)
        a.step(cmd, render=(t == 39))
        b.step(cmd, render=(t == 39))
        b.posture_clearance(po, host=(t % 2 == 0))
        if t % 13 == 5:
            a.closest_points()
            b.closest_points()
            b.posture_clearance(po)
            for w in range(2):
                assert a.distance_buffer(w, host=True).tobytes() == b.distance_buffer(w, host=True).tobytes(), (t, w)
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    for f in (nat.F_ERRFLAGS, nat.F_TOUCH, nat.F_RGB, nat.F_DEPTH, nat.F_STATE):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert (b.posture_buffer('nearest', host=True)[..., 0] > 0).any()
    a.close()
    b.close()


def _buffers(env):
    out = []
    for w in range(4):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_posture_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_api():
    import torch
    N = 5
    env = _env(N)
    L = env.L
    good = np.ascontiguousarray(nd.states(N * 2, 122)[:, :11].reshape(N, 2, 11))
    # an empty pair table is refused, by the library and by the binding
    assert L.rr_posture_clearance(env.h, good.ctypes.data, 2, 0) == -1 and 'pair table is empty' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.posture_clearance(good)
    before = _buffers(env)
    assert [n for _, n in before] == [0, 0, 0, 0] and all(p for p, _ in before) and len({p for p, _ in before}) == 4
    n = nd.names()
    p3 = np.array([(n['skin_00'], n['cube']), (n['finger_01'], n['tomato']), (n['lbr_iiwa_link_6'], n['table'])], np.int32)
    env.set_distance_pairs(p3)
    assert [x for _, x in _buffers(env)] == [0, 0, 0, 0]                                             # before the first query K counts as 0
    for w, name in enumerate(nat.PC_FIELDS):
        assert env.posture_buffer(name, host=True).shape[:2] == (N, 0) and env.posture_buffer(w).shape[:2] == (N, 0)
    # zero-filled before the first query, over the whole allocation
    whole = (N * nat.PC_MAX_POSTURES * 12, N * nat.PC_MAX_POSTURES * 4, N * nat.PC_MAX_POSTURES * nat.DIST_MAX, N * nat.PC_MAX_POSTURES * nat.DIST_MAX)
    env.sync()
    for (p, _), count in zip(before, whole):
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (count,), '<i4', env)).any().item()
    env.state = nd.states(N, 123)
    first = _copy(env.posture_clearance(good, host=True))
    assert [x for _, x in _buffers(env)] == [N * 2 * 48, N * 2 * 16, N * 2 * 3 * 4, N * 2 * 3 * 4]
    # refused calls: RR_EINVAL (-1), the cause named, nothing changes
    for args, word in (((None, 2, 0), 'null postures'), ((good.ctypes.data, 0, 0), 'n_postures 0'), ((good.ctypes.data, 33, 0), 'n_postures 33'),
                       ((good.ctypes.data, -1, 1), 'n_postures -1')):
        assert L.rr_posture_clearance(env.h, *args) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_posture_clearance' in msg and word in msg, msg
    p, x = C.c_void_p(), C.c_size_t()
    for which in (4, -1):
        assert L.rr_posture_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_posture_buffer' in L.rr_last_error().decode()
    assert L.rr_posture_copy_to_host(env.h, 0, first['distance'].ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    for bad in (good[:, :, :9], good.astype(np.float64), np.zeros((N, 33, 11), np.float32), good[:4]):
        with pytest.raises(ValueError):
            env.posture_clearance(bad)
    with pytest.raises(ValueError):
        env.posture_buffer('points')
    assert [x for _, x in _buffers(env)] == [N * 2 * 48, N * 2 * 16, N * 2 * 3 * 4, N * 2 * 3 * 4]
    got = {name: env.posture_buffer(name, host=True) for name in nat.PC_FIELDS}
    assert (_bits(got['nearest'][..., 0]) == _bits(first['distance'])).all() and (got['id'][..., 1] == first['pair']).all()
    assert (_bits(got['distance']) == _bits(first['pair_distance'])).all()
    # the query works after reset, state = ... and restore
    ck = env.checkpoint()
    env.reset()
    after_reset = _copy(env.posture_clearance(good, host=True))
    assert np.isfinite(after_reset['pair_distance']).all() and not _same(after_reset, first)
    env.state = nd.states(N, 123)
    assert _same(first, _copy(env.posture_clearance(good, host=True)))
    env.state = nd.states(N, 124)
    env.restore(ck)
    assert _same(first, _copy(env.posture_clearance(good, host=True)))
    # pointers stay across K and Q; the sizes follow
    k5 = np.ascontiguousarray(nd.states(N * 5, 125)[:, :11].reshape(N, 5, 11))
    env.set_distance_pairs('collision')
    assert env.posture_clearance(k5, host=True)['pair_distance'].shape == (N, 5, 92)
    after = _buffers(env)
    assert [p for p, _ in after] == [p for p, _ in before] and [x for _, x in after] == [N * 5 * 48, N * 5 * 16, N * 5 * 92 * 4, N * 5 * 92 * 4]
    env.set_distance_pairs([])
    assert L.rr_posture_clearance(env.h, good.ctypes.data, 2, 0) == -1 and [p for p, _ in _buffers(env)] == [p for p, _ in before]
    env.close()


def test_non_finite_posture_and_object_pose():
    """A NaN posture in one (env, k), then a NaN object pose in one env: the call returns, the stream syncs, every other row is bit
    for bit the clean run's, and the bad rows stay well-formed (the loop bounds do not depend on data)."""
    st, po, pairs, _, clean = _case_r()
    env = _env(4)
    env.state = st
    env.set_distance_pairs(pairs)
    bad = po.copy()
    bad[2, 1, 3] = np.nan
    out = _copy(env.posture_clearance(bad, host=True))
    env.sync()
    others = np.ones((4, 4), bool)
    others[2, 1] = False
    assert _same(out, clean, rows=others)
    assert 0 <= out['pair'][2, 1] < 80 and np.isin(out['pair_status'][2, 1], (0, 1, 2, 3)).all() and out['pair_iterations'][2, 1].max() <= 32
    assert out['status'][2, 1] == out['pair_status'][2, 1, out['pair'][2, 1]]
    nanst = st.copy()
    nanst[1, 22:29] = np.nan
    env.write_state(nanst, np.array([0, 1, 0, 0], np.uint8), obj_pose=True)
    out = _copy(env.posture_clearance(po, host=True))
    env.sync()
    env.close()
    assert _same(out, clean, rows=[0, 2, 3])
    assert (out['pair'][1] >= 0).all() and (out['pair'][1] < 80).all() and np.isin(out['pair_status'][1], (0, 1, 2, 3)).all() and out['pair_iterations'][1].max() <= 32
