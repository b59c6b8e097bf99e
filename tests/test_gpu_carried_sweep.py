"""GPU tests (-m gpu) of the swept clearance with carried objects (rr_carried_sweep, include/realrobot.h) on the committed fixture
(tests/golden/carried_sweep.npz: N = 4, K = 8, 18 pairs, the float64 profile of every pair at 65 uniform t with the carried objects
moving; safety 0.01, tolerance 1e-3; env 0 nothing attached, env 1 the cube on the gripper base captured, env 2 the cube on a finger
link and the tomato on a mid-arm link given, env 3 all three on the gripper base captured): the guarantees against the profiles,
tightness of the stop, the statuses by class, the float64 restatement row for row, the hit record against posture_clearance at q_stop
bit for bit, the free env and the forwarding against swept_clearance byte for byte, determinism, input paths, no effect on the
simulation, non-finite input, the refusals.

SLACK is the larger of the distance tolerance of tests/test_gpu_posture_query.py and four times tests/test_gpu_carry.py's MEASURED_D:
the project's own ceilings for a float32 record on free and on carried items.  Every test prints its figures before it judges.
Measured on the MI355X: the smallest profile - safety over the samples the device declares free is +6.08e-4 m; the largest float64
distance of a reported pair at q_stop, the object carried there, is 1.16e-5 m inside safety + tolerance; status, pair, steps and
evaluations are the float64 restatement's row for row (at most 38 steps)."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_carried_sweep as cs
from tests import numpy_distance as nd
from tests import numpy_sweep as sw
from tests.test_gpu_carry import MEASURED_D
from tests.test_gpu_posture_query import TOL as TOL_D

pytestmark = pytest.mark.gpu

SLACK = max(TOL_D, 4 * MEASURED_D)
KEYS = ('fraction', 'q_stop', 'status', 'pair', 'steps', 'evaluations', 'distance', 'lower', 'point_a', 'point_b', 'normal', 'pair_free_until')
N, K = cs.N, cs.K


def _env(n=N):
    return BatchedREALRobotEnv(n, objects=3, width=64, height=64)


def _bytes(env):
    return [env.sweep_buffer(w, host=True).tobytes() for w in range(len(nat.SW_FIELDS))]


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _plain_env():
    f = cs.fixture()
    env = _env()
    env.state = f['states']
    env.set_distance_pairs(f['pairs'])
    return env


def _attach(env):
    """The fixture's attachments: envs 0, 1, 3 captured from the state (env 0 has none), env 2 given."""
    f = cs.fixture()
    env.attach_objects(f['links'], env_mask=cs.CAPTURED)
    env.attach_objects(f['links'], rel_pose=f['rel_given'], env_mask=1 - cs.CAPTURED)


def _fixture_env():
    env = _plain_env()
    _attach(env)
    return env


_dev = {}


def _device():
    """The device's answer on the fixture, asked once per process: (columns, the four buffers' bytes)."""
    if not _dev:
        f = cs.fixture()
        env = _fixture_env()
        out = _copy(env.carried_sweep(f['segments'], f['safety'], f['tolerance'], host=True))
        _dev.update(out=out, bytes=_bytes(env))
        env.close()
    return _dev['out'], _dev['bytes']


def test_returns_every_column_well_formed():
    out, _ = _device()
    f = cs.fixture()
    Q = len(f['pairs'])
    assert set(out) == set(KEYS)
    assert out['fraction'].shape == (N, K) and out['q_stop'].shape == (N, K, 11) and out['pair_free_until'].shape == (N, K, Q)
    assert out['point_a'].shape == out['point_b'].shape == out['normal'].shape == (N, K, 3)
    assert np.isin(out['status'], (0, 1, 3)).all() and (out['steps'] >= 1).all() and (out['steps'] <= nat.SW_MAX_STEPS).all()
    assert ((out['pair'] >= 0) & (out['pair'] < Q))[out['status'] != 0].all() and (out['pair'][out['status'] == 0] == -1).all()
    assert (out['evaluations'] >= Q).all() and (out['evaluations'] <= out['steps'] * Q).all()
    assert ((out['pair_free_until'] >= 0) & (out['pair_free_until'] <= 1)).all()
    assert ((out['fraction'] >= 0) & (out['fraction'] <= 1)).all()
    seg = f['segments']
    stopped = out['status'] != 0
    q = np.float32(seg[:, :, 0]) + out['fraction'][..., None] * (seg[:, :, 1] - seg[:, :, 0])
    assert np.abs(q - out['q_stop'])[stopped].max() <= 4e-7


def test_conservative_against_the_profiles():
    out, _ = _device()
    f = cs.fixture()
    worst, bad = np.inf, 0
    for e, k in cs.ROWS:
        res = dict(free=out['pair_free_until'][e, k], fraction=out['fraction'][e, k])
        n, slack = sw.violations(res, f['profile'][e, k], f['safety'], slack=SLACK)
        worst, bad = min(worst, slack), bad + n
    print('smallest profile - safety over the samples the device covers: %.4g m (must exceed -%.3g); violated samples: %d; largest step count %d'
          % (worst, SLACK, bad, out['steps'].max()))
    assert bad == 0 and worst > -SLACK


def test_tight_where_it_stops():
    out, _ = _device()
    f = cs.fixture()
    worst, seen = -np.inf, 0
    for e, k in cs.ROWS:
        if out['status'][e, k] != 1:
            continue
        j = int(out['pair'][e, k])
        d = float(cs.lower_bounds(f['states'][e], out['q_stop'][e, k], f['pairs'][j:j + 1], f['links'][e], f['rel'][e])[0])
        worst, seen = max(worst, d - f['safety'] - f['tolerance']), seen + 1
    print('largest float64 distance of a reported pair at q_stop, the object carried there, minus (safety + tolerance): %.4g m (at most %.3g) over %d rows'
          % (worst, SLACK, seen))
    assert seen >= 16 and worst <= SLACK


def test_status_by_class():
    out, _ = _device()
    f = cs.fixture()
    cls = cs.classes()
    print('status', out['status'].tolist(), 'pair', out['pair'].tolist(), 'steps', out['steps'].tolist(), 'evaluations', out['evaluations'].tolist())
    seen = 0
    for (e, k), c in cls.items():
        st, fr = int(out['status'][e, k]), float(out['fraction'][e, k])
        assert st != 3, (e, k)
        if 'free' in c:
            assert st == 0 and fr == 1.0 and out['pair'][e, k] == -1, (e, k, st, fr)
            assert not np.concatenate([out[x][e, k].ravel() for x in ('distance', 'lower', 'point_a', 'point_b', 'normal')]).view(np.uint32).any()
        if 'tunnel' in c:
            assert st == 1 and 0.0 < fr < 1.0, (e, k, st, fr)
        if 'start_in_collision' in c:
            assert st == 1 and fr == 0.0 and out['steps'][e, k] == 1, (e, k, st, fr)
        if 'carried_hits_arm_free' in c:
            assert st == 1 and fr < 1.0 and cs.carried_pairs(f['pairs'], f['links'][e])[out['pair'][e, k]], (e, k, st, fr, out['pair'][e, k])
            seen += 1
    assert seen >= 6


def test_decides_as_the_float64_restatement_row_for_row():
    out, _ = _device()
    f = cs.fixture()
    got = np.stack([out['status'], out['pair'], out['steps'], out['evaluations']], -1)
    print('device {status, pair, steps, evaluations} differ from the restatement on rows', np.argwhere((got != f['restated']).any(-1)).tolist())
    assert (got == f['restated']).all()


def test_hit_record_is_posture_clearance_at_q_stop():
    out, raw = _device()
    f = cs.fixture()
    hit = np.frombuffer(raw[nat.SW_FIELDS.index('hit')], np.uint32).reshape(N, K, 12)
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
    assert seen == int((out['status'] != 0).sum()) >= 16


def test_free_env_and_forwarding_are_swept_clearance_byte_for_byte():
    out, raw = _device()
    f = cs.fixture()
    seg, s, t = f['segments'], f['safety'], f['tolerance']
    twin = _plain_env()                                                           # never attached
    want = _copy(twin.swept_clearance(seg, s, t, host=True))
    want_raw = _bytes(twin)
    for key in KEYS:                                                              # env 0 has no attachment on the attached handle
        assert out[key][0].tobytes() == want[key][0].tobytes(), key
    assert (out['status'][1:] != want['status'][1:]).any()                        # ... and the carried envs do differ
    got = _copy(twin.carried_sweep(seg, s, t, host=True))                         # a handle that never attached: the call forwards
    assert _bytes(twin) == want_raw and all(got[k].tobytes() == want[k].tobytes() for k in KEYS)
    twin.close()
    env = _fixture_env()
    env.carried_sweep(seg, s, t)
    assert _bytes(env) == raw
    env.detach_objects()                                                          # the unmasked detach: forwarding again
    env.carried_sweep(seg, s, t)
    assert _bytes(env) == want_raw
    env.swept_clearance(seg, s, t)
    assert _bytes(env) == want_raw
    env.close()


def test_determinism_permutations_and_input_paths():
    import torch
    out, raw = _device()
    f = cs.fixture()
    seg, s, t = f['segments'], f['safety'], f['tolerance']
    env = _fixture_env()
    env.carried_sweep(seg, s, t)
    assert _bytes(env) == raw                                                   # two calls (another handle, the device road of the views)
    dev = torch.as_tensor(seg, device='cuda:0')
    env.carried_sweep(dev, s, t)
    env.sync()
    assert _bytes(env) == raw                                                   # a device tensor read in place
    pk = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    got = _copy(env.carried_sweep(np.ascontiguousarray(seg[:, pk]), s, t, host=True))
    for key in KEYS:
        assert got[key].tobytes() == np.ascontiguousarray(out[key][:, pk]).tobytes(), key      # rows permuted along K
    got = _copy(env.carried_sweep(np.ascontiguousarray(seg[:, :1]), s, t, host=True))
    for key in KEYS:
        assert got[key].tobytes() == np.ascontiguousarray(out[key][:, :1]).tobytes(), key      # K = 1: a row does not depend on its neighbours
    env.close()


def test_no_effect_on_the_simulation():
    """Steps with a carried sweep after each leave the state, the preparation record, the error flags, the buffers of the other queries
    and the next steps' outputs bit-identical to those of a twin that attached and never asked."""
    from real_robots_amd.distributed import synthetic_actions
    f = cs.fixture()
    a, b = _env(), _env()
    po = np.ascontiguousarray(f['segments'][:, :2, 0])
    for env in (a, b):
        env.reset()
        env.set_distance_pairs(f['pairs'])
        env.attach_objects({'cube': 'base'})
        env.closest_points()
        env.posture_clearance(po)
    for t in range(8):
        cmd = synthetic_actions(list(range(N)), t)
        a.step(cmd)
        b.step(cmd)
        b.carried_sweep(f['segments'], f['safety'], f['tolerance'], host=(t % 2 == 0))
        for fld in (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS, nat.F_JOINTS, nat.F_TOUCH, nat.F_OBJ_POSE, nat.F_CONTACT_COUNT):
            assert a.host(fld).tobytes() == b.host(fld).tobytes(), (t, fld)
    for w in range(2):
        assert a.distance_buffer(w, host=True).tobytes() == b.distance_buffer(w, host=True).tobytes(), w
    for w in range(4):
        assert a.posture_buffer(w, host=True).tobytes() == b.posture_buffer(w, host=True).tobytes(), w
    la, ra = a.attachments()
    lb, rb = b.attachments()
    assert (la == lb).all() and ra.tobytes() == rb.tobytes()
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert (b.sweep_buffer('id', host=True)[..., 2] >= 1).all()
    a.close()
    b.close()


def test_non_finite_input_leaves_the_loop():
    """A bounded-loop check: every loop bound of the kernel is a constant or Q, so a non-finite segment row or table row ends within the
    step cap, and no other env sees it."""
    out, _ = _device()
    f = cs.fixture()
    seg = f['segments'].copy()
    seg[1, 2, 1, 3] = np.nan
    seg[2, 6, 0, 0] = np.inf
    st = f['states'].copy()
    st[3, 22:29] = np.nan                                                         # env 3's cube has no pose when it is captured
    env = _env()
    env.state = st
    env.set_distance_pairs(f['pairs'])
    _attach(env)
    rel = env.attachments()[1]
    assert not np.isfinite(rel[3, 0]).all() and np.isfinite(rel[:3]).all()
    got = _copy(env.carried_sweep(seg, f['safety'], f['tolerance'], host=True))
    env.sync()
    env.close()
    bad = np.zeros((N, K), bool)
    bad[1, 2] = bad[2, 6] = True
    bad[3] = True
    print('non-finite rows: status', got['status'][bad].tolist(), 'steps', got['steps'][bad].tolist())
    assert (got['steps'][bad] <= nat.SW_MAX_STEPS).all() and np.isin(got['status'][bad], (0, 1, 3)).all()
    for key in KEYS:
        assert np.ascontiguousarray(got[key][~bad]).tobytes() == np.ascontiguousarray(out[key][~bad]).tobytes(), key


def test_refusals_leave_the_buffers_untouched():
    f = cs.fixture()
    env = _env()
    L = env.L
    good = np.ascontiguousarray(f['segments'][:, :2])
    call = lambda ptr, k, s, t: L.rr_carried_sweep(env.h, ptr, k, 0, s, t)
    env.state = f['states']
    for attached in (False, True):
        env.set_distance_pairs([])
        before = _bytes(env)                                                        # (in the second pass: what the first pass's queries left, in the empty table's layout)
        assert call(good.ctypes.data, 2, 0.0, 1e-3) == -1 and 'rr_carried_sweep' in L.rr_last_error().decode() and 'pair table is empty' in L.rr_last_error().decode()
        with pytest.raises(ValueError):
            env.carried_sweep(good)
        assert _bytes(env) == before
        env.set_distance_pairs(f['pairs'])
        if attached:
            _attach(env)
        env.carried_sweep(good, 0.01, 1e-3)
        first = _bytes(env)
        nan, inf = float('nan'), float('inf')
        for args, word in (((None, 2, 0.0, 1e-3), 'null segments'), ((good.ctypes.data, 0, 0.0, 1e-3), 'n_segments 0'), ((good.ctypes.data, 33, 0.0, 1e-3), 'n_segments 33'),
                           ((good.ctypes.data, 2, -1e-3, 1e-3), 'safety'), ((good.ctypes.data, 2, nan, 1e-3), 'safety'), ((good.ctypes.data, 2, inf, 1e-3), 'safety'),
                           ((good.ctypes.data, 2, 0.0, 5e-7), 'tolerance'), ((good.ctypes.data, 2, 0.0, nan), 'tolerance'), ((good.ctypes.data, 2, 0.0, 0.0), 'tolerance')):
            assert call(*args) == -1, word
            msg = L.rr_last_error().decode()
            assert 'rr_carried_sweep' in msg and word in msg, msg
            assert _bytes(env) == first, word                                       # a refusal writes nothing and launches nothing
        env.set_distance_pairs(f['pairs'], 0.05)                                    # a cull below safety + tolerance
        before = _bytes(env)
        assert call(good.ctypes.data, 2, 0.05, 1e-3) == -1 and 'max_distance' in L.rr_last_error().decode() and 'rr_carried_sweep' in L.rr_last_error().decode()
        assert _bytes(env) == before
        env.set_distance_pairs(f['pairs'])
        assert call(good.ctypes.data, 2, 0.01, 1e-3) == 0 and _bytes(env) == first
        for bad in (good[:, :, :, :9], good.astype(np.float64), good[:3]):
            with pytest.raises(ValueError):
                env.carried_sweep(bad)
        assert _bytes(env) == first
    # swept_clearance keeps refusing on the attached handle, and names the call that does not
    assert L.rr_swept_clearance(env.h, good.ctypes.data, 2, 0, 0.01, 1e-3) == -1 and 'rr_carried_sweep' in L.rr_last_error().decode()
    assert _bytes(env) == first
    p, x = C.c_void_p(), C.c_size_t()
    nat.check(L.rr_sweep_buffer(env.h, 0, C.byref(p), C.byref(x)))
    assert x.value == N * 2 * 48
    env.close()
