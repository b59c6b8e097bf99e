"""GPU tests (-m gpu) of the swept clearance along joint-space segments (rr_swept_clearance, include/realrobot.h) on the committed
fixture (tests/golden/swept_clearance.npz: N = 3, K = 8, 18 pairs, the float64 profile of every pair at 65 uniform t; safety 0.01,
tolerance 1e-3): the guarantees against the profiles, tightness of the stop, the statuses by class, the hit record against
posture_clearance at q_stop bit for bit, the reach table against float64, bit-identity between calls, permutations, batch sizes and
input paths, no effect on the simulation, a non-finite row.

TOL_D is the distance tolerance of tests/test_gpu_posture_query.py (four times the largest |distance - exact| measured there against
the float64 reference): the device's lower bound is a float32 number at float32 frames, so a guarantee is held to safety - TOL_D.
Measured on the MI355X (each test prints its figures before it judges): the smallest profile - safety over the samples the device
declares free is +6.08e-4 m; the largest float64 distance of a reported pair at q_stop is 1.00e-4 m inside safety + tolerance; the
reach table is at most 0.97 ulp above float64; steps and evaluations are the float64 restatement's row for row (at most 31 steps)."""
import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_distance as nd
from tests import numpy_sweep as sw
from tests.test_gpu_posture_query import TOL as TOL_D

pytestmark = pytest.mark.gpu

ROWS = [(e, k) for e in range(3) for k in range(8)]
KEYS = ('fraction', 'q_stop', 'status', 'pair', 'steps', 'evaluations', 'distance', 'lower', 'point_a', 'point_b', 'normal', 'pair_free_until')


def _env(N):
    return BatchedREALRobotEnv(N, objects=3, width=64, height=64)


def _bytes(env):
    return [env.sweep_buffer(w, host=True).tobytes() for w in range(len(nat.SW_FIELDS))]


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _fixture_env(N=3, envs=None):
    f = sw.fixture()
    env = _env(N)
    env.state = f['states'][:N] if envs is None else f['states'][envs]
    env.set_distance_pairs(f['pairs'])
    return env


_dev = {}


def _device():
    """The device's answer on the fixture, asked once per process: (columns, the four buffers' bytes)."""
    if not _dev:
        f = sw.fixture()
        env = _fixture_env()
        out = _copy(env.swept_clearance(f['segments'], f['safety'], f['tolerance'], host=True))
        _dev.update(out=out, bytes=_bytes(env))
        env.close()
    return _dev['out'], _dev['bytes']


def _classes():
    f = sw.fixture()
    return {(e, k): sw.classify(f['profile'][e, k], f['segments'][e, k].astype(np.float64), f['safety']) for e, k in ROWS}


def test_returns_every_column_well_formed():
    out, _ = _device()
    f = sw.fixture()
    Q = len(f['pairs'])
    assert set(out) == set(KEYS)
    assert out['fraction'].shape == (3, 8) and out['q_stop'].shape == (3, 8, 11) and out['pair_free_until'].shape == (3, 8, Q)
    assert out['point_a'].shape == out['point_b'].shape == out['normal'].shape == (3, 8, 3)
    assert np.isin(out['status'], (0, 1, 3)).all() and (out['steps'] >= 1).all() and (out['steps'] <= nat.SW_MAX_STEPS).all()
    assert ((out['pair'] >= 0) & (out['pair'] < Q))[out['status'] != 0].all() and (out['pair'][out['status'] == 0] == -1).all()
    assert (out['evaluations'] >= Q).all() and (out['evaluations'] <= out['steps'] * Q).all()
    assert ((out['pair_free_until'] >= 0) & (out['pair_free_until'] <= 1)).all()
    assert ((out['fraction'] >= 0) & (out['fraction'] <= 1)).all()
    # q_stop is q(fraction) of a stopped row: the posture of the last step
    seg = f['segments']
    stopped = out['status'] != 0
    q = np.float32(seg[:, :, 0]) + out['fraction'][..., None] * (seg[:, :, 1] - seg[:, :, 0])
    assert np.abs(q - out['q_stop'])[stopped].max() <= 4e-7


def test_conservative_against_the_profiles():
    out, _ = _device()
    f = sw.fixture()
    worst, bad = np.inf, 0
    for e, k in ROWS:
        res = dict(free=out['pair_free_until'][e, k], fraction=out['fraction'][e, k])
        n, slack = sw.violations(res, f['profile'][e, k], f['safety'], slack=TOL_D)
        worst, bad = min(worst, slack), bad + n
    print('smallest profile - safety over the samples the device covers: %.4g m (must exceed -%.3g); violated samples: %d' % (worst, TOL_D, bad))
    assert bad == 0 and worst > -TOL_D


def test_tight_where_it_stops():
    out, _ = _device()
    f = sw.fixture()
    env = _fixture_env()
    worst = -np.inf
    for e, k in ROWS:
        if out['status'][e, k] != 1:
            continue
        j = int(out['pair'][e, k])
        env.set_distance_pairs(f['pairs'][j:j + 1])
        po = np.ascontiguousarray(np.broadcast_to(out['q_stop'][e, k], (3, 1, 11)), dtype=np.float32)
        gjk = int(env.posture_clearance(po, host=True)['status'][e, 0])
        if gjk not in (0, 1):
            continue
        d = max(float(nd.reference(np.concatenate([out['q_stop'][e, k], f['states'][e, 11:]])[None].astype(np.float64), f['pairs'][j:j + 1])['d'][0, 0]), 0.0)
        worst = max(worst, d - f['safety'] - f['tolerance'])
        assert d <= f['safety'] + f['tolerance'] + TOL_D, (e, k, j, d)
    env.close()
    print('largest float64 distance of a reported pair at q_stop minus (safety + tolerance): %.4g m (at most %.3g)' % (worst, TOL_D))
    assert worst > -np.inf


def test_status_by_class():
    out, _ = _device()
    cls = _classes()
    for (e, k), c in cls.items():
        st, fr = int(out['status'][e, k]), float(out['fraction'][e, k])
        if 'long' not in c:
            assert st != 3, (e, k)
        if 'free' in c:
            assert st == 0 and fr == 1.0 and out['pair'][e, k] == -1, (e, k, st, fr)
            assert not np.concatenate([out[x][e, k].ravel() for x in ('distance', 'lower', 'point_a', 'point_b', 'normal')]).view(np.uint32).any()
        if 'tunnel' in c:
            assert st == 1 and 0.0 < fr < 1.0, (e, k, st, fr)
        if 'start_in_collision' in c:
            assert st == 1 and fr == 0.0 and out['steps'][e, k] == 1, (e, k, st, fr)
    print('steps', out['steps'].tolist(), 'evaluations', out['evaluations'].tolist(), 'status', out['status'].tolist())


def test_hit_record_is_posture_clearance_at_q_stop():
    out, raw = _device()
    f = sw.fixture()
    hit = np.frombuffer(raw[nat.SW_FIELDS.index('hit')], np.uint32).reshape(3, 8, 12)
    env = _fixture_env()
    po = np.ascontiguousarray(out['q_stop'])
    seen = 0
    for j in sorted(set(out['pair'][out['status'] != 0].tolist())):
        env.set_distance_pairs(f['pairs'][j:j + 1])
        env.posture_clearance(po)
        near = env.posture_buffer('nearest', host=True).view(np.uint32)
        m = (out['status'] != 0) & (out['pair'] == j)
        assert (near[m] == hit[m]).all(), j
        seen += int(m.sum())
    env.close()
    assert seen == int((out['status'] != 0).sum()) >= 12


def test_reach_table():
    env = _env(1)
    got = env.sweep_reach()
    env.close()
    ref = sw.reach_table()
    assert got.shape == ref.shape and got.dtype == np.float32
    up = got.astype(np.float64) - ref
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print('reach - float64: min %.3g, max %.3g ulp' % (up.min(), (up / ulp).max()))
    assert (up >= 0).all() and (up <= 2 * ulp).all() and ((got == 0) == (ref == 0)).all()


def test_determinism_and_independence():
    import torch
    out, raw = _device()
    f = sw.fixture()
    seg, s, t = f['segments'], f['safety'], f['tolerance']
    env = _fixture_env()
    env.swept_clearance(seg, s, t)
    assert _bytes(env) == raw                                                   # two calls (another handle, the device road of the views)
    dev = torch.as_tensor(seg, device='cuda:0')
    env.swept_clearance(dev, s, t)
    env.sync()
    assert _bytes(env) == raw                                                   # a device tensor read in place
    pk = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    got = _copy(env.swept_clearance(np.ascontiguousarray(seg[:, pk]), s, t, host=True))
    for key in KEYS:
        assert got[key].tobytes() == np.ascontiguousarray(out[key][:, pk]).tobytes(), key      # rows permuted along K
    env.close()
    pe = [2, 0, 1]
    env = _fixture_env(envs=pe)
    got = _copy(env.swept_clearance(np.ascontiguousarray(seg[pe]), s, t, host=True))
    for key in KEYS:
        assert got[key].tobytes() == np.ascontiguousarray(out[key][pe]).tobytes(), key          # ... and along the envs
    env.close()
    env = _fixture_env(N=1)
    got = _copy(env.swept_clearance(np.ascontiguousarray(seg[:1, :1]), s, t, host=True))
    for key in KEYS:
        assert got[key].tobytes() == np.ascontiguousarray(out[key][:1, :1]).tobytes(), key      # row 0 at N = 1, K = 1
    env.close()


def test_no_effect_on_the_simulation():
    """Steps with a swept query after each leave the state, the preparation record, the error flags, the buffers of the other queries
    and the next steps' outputs bit-identical to those of a twin that never asked."""
    from real_robots_amd.distributed import synthetic_actions
    f = sw.fixture()
    a, b = _env(3), _env(3)
    po = np.ascontiguousarray(f['segments'][:, :2, 0])
    for env in (a, b):
        env.reset()
        env.set_distance_pairs(f['pairs'])
        env.closest_points()
        env.posture_clearance(po)
    for t in range(12):
        cmd = synthetic_actions(list(range(3)), t)
        a.step(cmd)
        b.step(cmd)
        b.swept_clearance(f['segments'], f['safety'], f['tolerance'], host=(t % 2 == 0))
        for fld in (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS, nat.F_JOINTS, nat.F_TOUCH, nat.F_OBJ_POSE, nat.F_CONTACT_COUNT):
            assert a.host(fld).tobytes() == b.host(fld).tobytes(), (t, fld)
    for w in range(2):
        assert a.distance_buffer(w, host=True).tobytes() == b.distance_buffer(w, host=True).tobytes(), w
    for w in range(4):
        assert a.posture_buffer(w, host=True).tobytes() == b.posture_buffer(w, host=True).tobytes(), w
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert (b.sweep_buffer('id', host=True)[..., 2] >= 1).all()
    a.close()
    b.close()


def test_non_finite_row_leaves_the_loop():
    out, _ = _device()
    f = sw.fixture()
    seg = f['segments'].copy()
    seg[1, 2, 1, 3] = np.nan
    seg[2, 6, 0, 0] = np.inf
    env = _fixture_env()
    got = _copy(env.swept_clearance(seg, f['safety'], f['tolerance'], host=True))
    env.sync()
    env.close()
    for e, k in ((1, 2), (2, 6)):
        assert got['steps'][e, k] <= nat.SW_MAX_STEPS and got['status'][e, k] in (0, 1, 3), (e, k, got['steps'][e, k], got['status'][e, k])
    others = np.ones((3, 8), bool)
    others[1, 2] = others[2, 6] = False
    for key in KEYS:
        assert np.ascontiguousarray(got[key][others]).tobytes() == np.ascontiguousarray(out[key][others]).tobytes(), key
