"""GPU tests (-m gpu) of the device-side state writes and reads (rr_write_state / rr_read_state, rr_write.inc):
* read_state() is the state, and only a further call refreshes it;
* the device road equals the host calls bit for bit -- rr_reset, rr_set_object_poses, rr_set_state, reset + teleport in one call --
  right behind the call and five steps later, images included;
* every column group alone under a mask, with NaN in everything the call must not use (other columns, unmasked rows, objects the
  handle does not have); uint8 and bool masks;
* an identity write keeps the run bit for bit (contact history included), RR_W_FRESH drops the history;
* a frozen env stays frozen without RR_W_FRESH; the host path; refused calls change nothing; reset() with a device mask.
70 envs: a partial second workgroup of 64, and masks with set and clear bytes on both sides of env 64 and in the tail.  Every
comparison is bitwise.  The handles are warmed up once (60 steps, the run of tests/test_gpu_fork.py, which has contact history) and
every test starts from that checkpoint."""

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions

pytestmark = pytest.mark.gpu

N, T0 = 70, 60
ALL4 = dict(joint_pos=True, joint_vel=True, obj_pose=True, obj_vel=True)
_cache = {}


def _cmds():
    if 'cm' not in _cache:
        _cache['cm'] = [synthetic_actions(range(N), t, seed=5).astype(np.float32) for t in range(T0 + 8)]
    return _cache['cm']


def _handles(objects):
    """(A, B, checkpoint after the warm-up, the state at step 30) for handles with `objects` objects, made once"""
    if objects not in _cache:
        A, B = (BatchedREALRobotEnv(N, objects=objects, width=64, height=64) for _ in range(2))
        st30 = None
        for t in range(T0):
            for e in (A, B):
                e.step(_cmds()[t], render=(t % 7 == 0))
            if t == 29:
                st30 = A.state
        ck = A.checkpoint()
        assert np.array_equal(ck, B.checkpoint())
        assert A.host(nat.F_CONTACT_COUNT).max() > 0        # (the run has contact history to keep or to drop)
        _cache[objects] = (A, B, ck, st30)
    return _cache[objects]


@pytest.fixture
def pair():
    A, B, ck, st30 = _handles(3)
    A.restore(ck)
    B.restore(ck)
    return A, B, st30


def teardown_module(module):
    for v in _cache.values():
        if isinstance(v, tuple):
            v[0].close()
            v[1].close()
    _cache.clear()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _mask(dtype=np.uint8):
    """seeded; set and clear bytes on both sides of env 64 and in the tail; as uint8 the set bytes are any non-zero value"""
    rng = np.random.default_rng(11)
    m = rng.random(N) < 0.5
    m[[1, 62, 64, 68]] = True
    m[[0, 63, 65, 69]] = False
    if dtype == np.uint8:
        return (m * rng.integers(1, 256, N)).astype(np.uint8)
    return m


def _everything(env):
    return dict(state=env.state, touch=env.host(nat.F_TOUCH), count=env.host(nat.F_CONTACT_COUNT), errflags=env.host(nat.F_ERRFLAGS),
                timestep=env.host(nat.F_TIMESTEP), joints=env.host(nat.F_JOINTS), obj_pose=env.host(nat.F_OBJ_POSE),
                contacts=[env.contacts(i) for i in range(env.N)])


def _images(env):
    return dict(rgb=env.host(nat.F_RGB), depth=env.host(nat.F_DEPTH), mask=env.host(nat.F_MASK))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_equal(a, b, label, envs=None):
    """dicts of _everything / _images: bitwise equal (for the envs `envs`: all)"""
    sel = np.arange(N) if envs is None else np.asarray(envs)
    for k in a:
        if k == 'contacts':
            for i in sel:
                assert np.array_equal(_bits(a[k][i]), _bits(b[k][i])), (label, k, i)
        else:
            bad = np.flatnonzero([not np.array_equal(_bits(a[k][i]), _bits(b[k][i])) for i in sel])
            assert bad.size == 0, (label, k, sel[bad])


def _five_steps(A, B, label):
    for t in range(5):
        for e in (A, B):
            e.step(_cmds()[T0 + t], render=(t == 2))
    _assert_equal(_everything(A), _everything(B), label + ': five steps later')
    _assert_equal(_images(A), _images(B), label + ': images')
    assert (B.host(nat.F_ERRFLAGS) == 0).all()


def _poses(state, rng, nobj=3):
    """finite, plausible object poses [N, nobj, 7] near those of `state`: moved a few centimetres and lifted, any orientation"""
    p = np.empty((N, nobj, 7), np.float32)
    for o in range(nobj):
        p[:, o, :3] = state[:, 22 + 13 * o:25 + 13 * o] + rng.uniform(-0.03, 0.03, (N, 3)).astype(np.float32) + np.array([0, 0, 0.05], np.float32)
        q = rng.normal(size=(N, 4))
        p[:, o, 3:] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return p


def _pose_tensor(poses, mask):
    """NaN everywhere but in the pose columns of the masked envs"""
    T = np.full((N, 61), np.nan, np.float32)
    on = np.asarray(mask) != 0
    for o in range(poses.shape[1]):
        T[on, 22 + 13 * o:29 + 13 * o] = poses[on, o]
    return T


def test_read_state_is_the_state_until_the_next_read(pair):
    import torch
    _, B, _ = pair
    view = torch.from_dlpack(B.read_state())
    B.sync()
    first = view.clone().cpu().numpy()
    assert first.shape == (N, 61) and first.dtype == np.float32
    B.step(_cmds()[T0])
    B.sync()
    assert np.array_equal(_bits(view.clone().cpu().numpy()), _bits(first))       # a step does not refresh the buffer
    B.read_state()
    B.sync()
    second = view.clone().cpu().numpy()
    st = B.state
    assert np.array_equal(_bits(second), _bits(st)) and not np.array_equal(second, first)
    B.restore(_handles(3)[2])
    assert np.array_equal(_bits(B.state), _bits(first))


@pytest.mark.parametrize('what', ['reset', 'poses', 'set_state', 'reset_poses'])
def test_the_device_road_equals_the_host_calls(pair, what):
    A, B, st30 = pair
    mh = _mask()
    md = _dev(mh)
    poses = _poses(A.state, np.random.default_rng(3))
    if what == 'reset':
        A.reset(mh)
        nat.check(B.L.rr_write_state(B.h, None, md.data_ptr(), nat.W_RESET, 1))
    elif what == 'poses':
        A.set_object_poses(poses, mh)
        B.write_state(_dev(_pose_tensor(poses, mh)), md, obj_pose=True)
    elif what == 'set_state':
        A.state = st30
        B.write_state(_dev(st30), None, fresh=True, **ALL4)
    else:
        A.reset(mh)
        A.set_object_poses(poses, mh)
        B.write_state(_dev(_pose_tensor(poses, mh)), md, reset=True, obj_pose=True)
    _assert_equal(_everything(A), _everything(B), what)
    _five_steps(A, B, what)


def _expected(old, T, on, parts, nobj):
    exp = old.copy()
    cols = []
    if parts & nat.W_JOINT_POS:
        cols += list(range(0, 11))
    if parts & nat.W_JOINT_VEL:
        cols += list(range(11, 22))
    for o in range(nobj):
        if parts & nat.W_OBJ_POSE:
            cols += list(range(22 + 13 * o, 29 + 13 * o))
        if parts & nat.W_OBJ_VEL:
            cols += list(range(29 + 13 * o, 35 + 13 * o))
        elif parts & nat.W_OBJ_POSE:
            exp[on, 29 + 13 * o:35 + 13 * o] = 0.0
    cols = np.array(cols)
    exp[np.ix_(on, cols)] = T[np.ix_(on, cols)]
    return exp, cols


@pytest.mark.parametrize('objects', [3, 1])
def test_parts_and_mask_with_nan_in_everything_else(objects):
    _, B, ck, _ = _handles(objects)
    B.restore(ck)
    old, before = B.state, _everything(B)
    on = _mask(bool)
    rng = np.random.default_rng(29)
    # finite, plausible new values for every column: joints and velocities nudged, objects moved and turned
    new = old + rng.uniform(-0.02, 0.02, old.shape).astype(np.float32)
    new[:, 11:22] = rng.uniform(-0.3, 0.3, (N, 11)).astype(np.float32)
    pz = _poses(old, rng)
    for o in range(3):
        new[:, 22 + 13 * o:29 + 13 * o] = pz[:, o]
        new[:, 29 + 13 * o:35 + 13 * o] = rng.uniform(-0.2, 0.2, (N, 6)).astype(np.float32)
    flags = {nat.W_JOINT_POS: dict(joint_pos=True), nat.W_JOINT_VEL: dict(joint_vel=True), nat.W_OBJ_POSE: dict(obj_pose=True),
             nat.W_OBJ_VEL: dict(obj_vel=True), nat.W_OBJ_POSE | nat.W_OBJ_VEL: dict(obj_pose=True, obj_vel=True)}
    for parts, kw in flags.items():
        exp, cols = _expected(old, new, on, parts, objects)
        T = np.full((N, 61), np.nan, np.float32)
        T[np.ix_(on, cols)] = new[np.ix_(on, cols)]
        assert np.isnan(T[~on]).all() and np.isnan(T[:, 22 + 13 * objects:]).all() and np.isfinite(exp).all()
        Td = _dev(T)
        for dtype in (np.uint8, bool):
            B.restore(ck)
            B.write_state(Td, _dev(_mask(dtype)), **kw)
            after = _everything(B)
            assert np.array_equal(_bits(after['state']), _bits(exp)), (parts, dtype, np.argwhere(_bits(after['state']) != _bits(exp))[:4])
            for k in ('count', 'contacts', 'timestep', 'errflags', 'touch'):
                _assert_equal({k: after[k]}, {k: before[k]}, (parts, dtype))
            assert np.array_equal(after['joints'][~on], before['joints'][~on]) and np.array_equal(after['obj_pose'][~on], before['obj_pose'][~on])
        B.step(_cmds()[T0])
        assert (B.host(nat.F_ERRFLAGS) == 0).all(), parts


def test_identity_write_keeps_the_run_and_fresh_drops_the_history(pair):
    import torch
    A, B, _ = pair
    copy = torch.from_dlpack(B.read_state()).clone()
    B.write_state(copy, None, **ALL4)
    _assert_equal(_everything(A), _everything(B), 'identity')
    _five_steps(A, B, 'identity')
    B.restore(_handles(3)[2])
    assert B.host(nat.F_CONTACT_COUNT).max() > 0
    B.write_state(copy, None, fresh=True, **ALL4)
    assert (B.host(nat.F_CONTACT_COUNT) == 0).all() and (B.host(nat.F_ERRFLAGS) == 0).all() and (B.host(nat.F_TOUCH) == 0).all()
    assert all(len(B.contacts(i)) == 0 for i in range(N))
    assert (B.host(nat.F_TIMESTEP) == T0).all()             # the clock is not part of the clean-up


def test_a_frozen_env_stays_frozen_without_fresh(pair):
    A, B, _ = pair
    k, others = 64, np.delete(np.arange(N), 64)
    s0 = A.state
    bad = s0.copy()
    bad[k, 3] = np.nan
    A.state = s0                                            # (rr_set_state is a fresh start for every env: A takes the same one)
    B.state = bad
    for e in (A, B):
        e.step(_cmds()[T0])
    assert B.host(nat.F_ERRFLAGS)[k] & 1
    _assert_equal(_everything(A), _everything(B), 'poisoned', others)
    row = np.full((N, 61), np.nan, np.float32)
    row[k] = s0[k]
    m = np.zeros(N, np.uint8)
    m[k] = 1
    rd, md = _dev(row), _dev(m)
    clock = B.host(nat.F_TIMESTEP)[k]
    B.write_state(rd, md, **ALL4)
    assert B.host(nat.F_ERRFLAGS)[k] & 1 and np.array_equal(_bits(B.state[k]), _bits(s0[k]))
    for e in (A, B):
        e.step(_cmds()[T0 + 1])
    assert B.host(nat.F_ERRFLAGS)[k] & 1 and B.host(nat.F_TIMESTEP)[k] == clock       # still frozen: not stepped
    assert np.array_equal(_bits(B.state[k]), _bits(s0[k]))
    _assert_equal(_everything(A), _everything(B), 'frozen', others)
    B.write_state(rd, md, fresh=True, **ALL4)
    assert B.host(nat.F_ERRFLAGS)[k] == 0
    for e in (A, B):
        e.step(_cmds()[T0 + 2])
    assert B.host(nat.F_ERRFLAGS)[k] == 0 and B.host(nat.F_TIMESTEP)[k] == clock + 1
    assert not np.array_equal(B.state[k], s0[k]) and np.isfinite(B.state[k]).all()
    _assert_equal(_everything(A), _everything(B), 'thawed', others)


def test_host_path_equals_device_path(pair):
    A, B, _ = pair
    mh, on = _mask(), _mask(bool)
    old = A.state
    rng = np.random.default_rng(31)
    T = np.full((N, 61), np.nan, np.float32)
    T[on, :11] = old[on, :11] + rng.uniform(-0.02, 0.02, (int(on.sum()), 11)).astype(np.float32)
    for o in range(3):
        T[on, 29 + 13 * o:35 + 13 * o] = rng.uniform(-0.2, 0.2, (int(on.sum()), 6)).astype(np.float32)
    A.write_state(T, mh, joint_pos=True, obj_vel=True)
    B.write_state(_dev(T), _dev(mh), joint_pos=True, obj_vel=True)
    ea = _everything(A)
    _assert_equal(ea, _everything(B), 'host path')
    exp, _ = _expected(old, T, on, nat.W_JOINT_POS | nat.W_OBJ_VEL, 3)
    assert np.array_equal(_bits(ea['state']), _bits(exp))
    _five_steps(A, B, 'host path')


def test_refused_calls_change_nothing(pair):
    _, B, st30 = pair
    before = _everything(B)
    sd, md = _dev(st30), _dev(_mask())
    for state, parts, dev in ((sd.data_ptr(), 64, 1), (sd.data_ptr(), 15 | 128, 1), (sd.data_ptr(), 0, 1), (None, nat.W_OBJ_POSE, 1),
                              (None, nat.W_RESET | nat.W_JOINT_VEL, 1), (st30.ctypes.data, 1 << 31, 0), (None, nat.W_JOINT_POS, 0)):
        rc = B.L.rr_write_state(B.h, state, md.data_ptr() if dev else None, parts, dev)
        assert rc == -1, (parts, rc)                        # RR_EINVAL
        assert b'rr_write_state' in B.L.rr_last_error()
        with pytest.raises(nat.NativeError):
            nat.check(rc)
    _assert_equal(_everything(B), before, 'refused')
    B.step(_cmds()[T0])
    A = _handles(3)[0]
    A.step(_cmds()[T0])
    _assert_equal(_everything(A), _everything(B), 'refused: the next step')       # (the look-ahead was not dropped either way: same run)


def test_reset_with_a_device_mask(pair):
    import torch
    A, B, _ = pair
    mh = _mask()
    A.reset(mh)
    B.reset(_dev(mh))
    _assert_equal(_everything(A), _everything(B), 'reset, uint8')
    A.reset(_mask(bool))
    B.reset(_dev(_mask(bool)))
    assert _dev(_mask(bool)).dtype == torch.bool
    _assert_equal(_everything(A), _everything(B), 'reset, bool')
    _five_steps(A, B, 'reset')
