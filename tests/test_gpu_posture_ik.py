"""GPU tests (-m gpu) of the inverse kinematics at candidate targets (rr_posture_ik, include/realrobot.h) against the float64
restatement of its algorithm (tests/numpy_pik.py): that what a row REPORTS is true of the posture it returns (closed loop), that its
status is honest, that it lands where the float64 iteration lands, the round trip with posture_kinematics / posture_clearance, row
independence and determinism, hostile rows, no effect on the simulation, the buffers and the refusals.

Shapes: N = 3 with K = 5 (15 rows: one ragged wave) and N = 5 with K = 32 (160 rows: 2.5 waves); the fixture is numpy_pik.fixture, whose
conditions tests/test_numpy_pik.py checks.

Bounds of the closed loop, from the 5e-6 per coordinate or quaternion component that tests/test_gpu_kinematic_obs.py grants this float32
chain: position error sqrt(3) x 5e-6 -> 1e-5 m; orientation error angle 2 x 2 x 5e-6 -> 2e-5 rad; residual: their sum, 3e-5.

One RR_EINVAL of the header is not provoked here: a model without the 17 URDF links needs another compiled model.  That a refused
first call allocates nothing is not observable through the ABI; what is observable is checked: behind the refusals the buffers report
K = 0 and are zero over their whole allocation."""
import ctypes as C
import functools

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model
from tests import numpy_pik as npk
from tests.test_gpu_kinematic_obs import POINT_LINKS
from tests.test_numpy_pik import CONFIGS, FINGER_LINK, FINGER_LOCAL

pytestmark = pytest.mark.gpu

U = np.uint32
ARM = 7
TOL_POS, TOL_ANG, TOL_RES = 1e-5, 2e-5, 3e-5
TOL_Q = 1e-3
LIM = np.array(load_model()['body_limits'], np.float32)[:ARM]
PI32 = np.float32(np.pi)
LINK3, LINK3_LOCAL = 3, (0.0, 0.05, 0.1)
# the closed loop's cases: the four configurations, and the point on link_3
CASES = CONFIGS + [('link_3', LINK3, LINK3_LOCAL, False, True)]
KEYS = ('posture', 'residual', 'position_error', 'orientation_error', 'status', 'iterations')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U) if a.dtype.itemsize == 4 else a


def _same(a, b, rows=None):
    return all((_bits(a[k] if rows is None else a[k][rows]) == _bits(b[k] if rows is None else b[k][rows])).all() for k in KEYS)


def _env(N, objects=3):
    return BatchedREALRobotEnv(N, objects=objects, width=64, height=64)


def _points(env, name):
    """Sets the case's points and returns the index of the solved one: the fresh handle's point, or eight points with the solved one
    at index 7."""
    if name == 'finger_point':
        local = np.full((8, 3), 0.01, np.float32)
        local[7] = FINGER_LOCAL
        assert POINT_LINKS[7] == FINGER_LINK
        env.set_kinematic_points(POINT_LINKS, local)
        return 7
    if name == 'link_3':
        local = np.full((8, 3), 0.01, np.float32)
        local[7] = LINK3_LOCAL
        env.set_kinematic_points(POINT_LINKS[:7] + [LINK3], local)
        return 7
    return 0


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The fixture of a case and the float64 restatement's result on it at the cap of 64, computed once."""
    _, link, local, position_only, clamp = next(c for c in CASES if c[0] == name)
    targets, seeds, _ = npk.fixture(link, local)
    ref = npk.solve(targets.reshape(-1, 7), seeds.reshape(-1, 11), link, local, max_iterations=npk.FIX_MAX_ITERATIONS,
                    position_only=position_only, clamp=clamp)
    for a in (targets, seeds) + tuple(ref.values()):
        a.setflags(write=False)
    return targets, seeds, ref


@pytest.mark.parametrize('name,link,local,position_only,clamp', CASES)
def test_closed_loop_status_and_landing(name, link, local, position_only, clamp):
    """Measured on MI355X (160 rows per case; the bounds: 1e-5 m, 2e-5 rad, 3e-5 and, for the landing, 1e-3 rad):

        case            position (m)  angle (rad)  residual   status 0 / 1   |q - q64|inf (rad)   update counts
        full_clamped    1.77e-07      1.47e-07     1.71e-07   155 / 5        1.19e-06             equal on 160 rows
        full_wrapped    2.23e-07      1.68e-07     2.07e-07   157 / 3        1.55e-06             equal on 160 rows
        position_only   1.83e-07      1.79e-07     1.83e-07   158 / 2        7.95e-07             equal on 160 rows
        finger_point    1.44e-07      1.34e-07     1.52e-07   154 / 6        1.32e-06             equal on 160 rows
        link_3          6.09e-08      1.07e-07     1.07e-07   160 / 0        1.93e-07             equal on 160 rows

    The largest difference in update counts between the device and the float64 restatement is 0 in every case."""
    targets, seeds, ref = _reference(name)
    N, K = targets.shape[:2]
    env = _env(N)
    point = _points(env, name)
    out = env.posture_ik(targets, seeds, point=point, max_iterations=npk.FIX_MAX_ITERATIONS, position_only=position_only, clamp=clamp, host=True)
    assert [out[k].shape for k in KEYS] == [(N, K, 11)] + [(N, K)] * 5
    assert [out[k].dtype for k in KEYS] == [np.float32] * 4 + [np.int32] * 2
    assert not env.posture_ik_buffer('result', host=True)[..., 3].view(U).any()                        # the fourth value is +0.0
    q, st, it = out['posture'].reshape(-1, 11), out['status'].reshape(-1), out['iterations'].reshape(-1)
    # ---- closed loop: the float64 forward kinematics of the REPORTED posture reproduces the reported errors
    fin = st != 2
    assert fin.all()
    e64 = npk.errors(q.astype(np.float64), targets.reshape(-1, 7), link, local)
    res64 = e64['position_error'] if position_only else e64['full']
    d_pos = np.abs(out['position_error'].reshape(-1) - e64['position_error'])[fin].max()
    d_ang = np.abs(out['orientation_error'].reshape(-1) - e64['orientation_error'])[fin].max()
    d_res = np.abs(out['residual'].reshape(-1) - res64)[fin].max()
    # ---- it lands where DLS lands
    clear = (ref['status'] == 0) & (ref['iterations'] <= npk.CLEAR_CUT)
    same_count = it == ref['iterations']
    d_q = np.abs(q.astype(np.float64) - ref['posture']).max(-1)
    d_q_max = d_q[same_count].max() if same_count.any() else 0.0
    d_it = int(np.abs(it - ref['iterations']).max())
    print('%s: closed loop position %.3g m, angle %.3g rad, residual %.3g; status 0 / 1 / 2: %d / %d / %d; clear-cut rows %d of %d; '
          'same update count on %d rows, there |q - q64|inf <= %.3g rad; largest difference in update counts %d'
          % (name, d_pos, d_ang, d_res, (st == 0).sum(), (st == 1).sum(), (st == 2).sum(), clear.sum(), len(st), same_count.sum(), d_q_max, d_it))
    assert d_pos <= TOL_POS and d_ang <= TOL_ANG and d_res <= TOL_RES, (d_pos, d_ang, d_res)
    # ---- status is honest
    small = out['residual'].reshape(-1) < np.float32(1e-3)
    assert ((st == 0) == (small & (position_only | (e64['cos'] > 0)))).all()
    assert ((st == 0) | (st == 1)).all() and (it >= 0).all() and (it <= npk.FIX_MAX_ITERATIONS).all() and (it[st == 1] == npk.FIX_MAX_ITERATIONS).all()
    if clamp:
        assert (q[:, :ARM] >= LIM[:, 0]).all() and (q[:, :ARM] <= LIM[:, 1]).all()
    else:
        assert (q[:, :ARM] > -PI32).all() and (q[:, :ARM] <= PI32).all()
    assert (_bits(q[:, ARM:]) == _bits(seeds.reshape(-1, 11)[:, ARM:])).all()                          # the fingers: the seed's bits
    if name == 'link_3':
        assert (_bits(q[:, 3:]) == _bits(seeds.reshape(-1, 11)[:, 3:])).all() and (it > 0).any()      # joints 3..6 do not move link_3
        assert (np.abs(q[:, :3] - seeds.reshape(-1, 11)[:, :3]).max(-1) > 0)[it > 0].all()
    assert (st[clear] == 0).all()
    assert d_q_max <= TOL_Q, d_q_max
    env.close()


def test_round_trip_with_the_siblings():
    """Targets from posture_kinematics(q*), seeds q*: status 0 without an update, the posture q*'s bits; the device view feeds
    posture_clearance and posture_kinematics in place and gives what a host copy of it gives."""
    from tests import numpy_posture as npo
    N, K = 3, 5
    env = _env(N)
    env.set_distance_pairs(npo.robot_pairs(), 0.25)
    rng = np.random.default_rng(3)
    lim = np.array(load_model()['body_limits'], np.float64)
    qs = rng.uniform(lim.min(1), lim.max(1), (N, K, 11)).astype(np.float32)
    qs[..., :ARM] = np.clip(qs[..., :ARM], LIM[:, 0], LIM[:, 1])
    pk = env.posture_kinematics(qs, host=True)
    targets = np.ascontiguousarray(np.concatenate([pk['point_pos'][:, :, 0], pk['link_pose'][:, :, nat.EE_LINK, 3:]], -1))
    out = env.posture_ik(targets, qs, host=True)
    assert not out['status'].any() and not out['iterations'].any() and (out['residual'] < 1e-5).all()
    assert (_bits(out['posture']) == _bits(qs)).all()
    # seeds a little off: the device view of the solution, in place, against a host copy of it
    seeds = qs.copy()
    seeds[..., :ARM] = np.clip(seeds[..., :ARM] + rng.uniform(-0.2, 0.2, (N, K, ARM)).astype(np.float32), LIM[:, 0], LIM[:, 1])
    view = env.posture_ik(targets, seeds, max_iterations=64)
    host_copy = env.posture_ik_buffer('posture', host=True)
    assert (host_copy != qs).any()
    pc_dev = env.posture_clearance(view['posture'], host=True)
    pk_dev = env.posture_kinematics(view['posture'], host=True)
    pc_host = env.posture_clearance(host_copy, host=True)
    pk_host = env.posture_kinematics(host_copy, host=True)
    for k in pc_dev:
        assert pc_dev[k].tobytes() == pc_host[k].tobytes(), k
    for k in pk_dev:
        assert pk_dev[k].tobytes() == pk_host[k].tobytes(), k
    assert env.posture_ik_buffer('posture', host=True).tobytes() == host_copy.tobytes()                # the queries did not write it
    conv = env.posture_ik_buffer('info', host=True)[..., 0] == 0
    assert conv.mean() >= 0.8
    assert np.abs(pk_dev['point_pos'][:, :, 0] - targets[..., :3])[conv].max() < 1.1e-3                # the tool is where it was asked to be
    env.close()


def test_row_independence_and_determinism():
    import torch
    targets, seeds, _ = _reference('full_clamped')
    N, K = targets.shape[:2]
    env = _env(N)
    kw = dict(max_iterations=npk.FIX_MAX_ITERATIONS)
    first = env.posture_ik(targets, seeds, host=True, **kw)
    assert _same(first, env.posture_ik(targets, seeds, host=True, **kw))                               # a second call
    rng = np.random.default_rng(11)
    perm = rng.permutation(N * K)
    shuffled = env.posture_ik(np.ascontiguousarray(targets.reshape(-1, 7)[perm].reshape(N, K, 7)),
                              np.ascontiguousarray(seeds.reshape(-1, 11)[perm].reshape(N, K, 11)), host=True, **kw)
    for k in KEYS:
        rows = first[k].reshape((N * K,) + first[k].shape[2:])
        assert (_bits(shuffled[k].reshape(rows.shape)) == _bits(rows[perm])).all(), k
    # the device path: the bits of the staged host arrays
    t_dev, s_dev = torch.from_numpy(np.array(targets)).cuda(), torch.from_numpy(np.array(seeds)).cuda()
    torch.cuda.synchronize()
    view = env.posture_ik(t_dev, s_dev, **kw)
    dev = {k: torch.from_dlpack(v) for k, v in view.items()}
    env.sync()
    for k in KEYS:
        assert dev[k].is_cuda and tuple(dev[k].shape) == first[k].shape and (_bits(dev[k].cpu().numpy()) == _bits(first[k])).all(), k
    # next to rows of NaNs
    bad_t, bad_s = np.array(targets), np.array(seeds)
    bad_t[1, 7] = np.nan
    bad_s[3, 30] = np.nan
    others = np.ones((N, K), bool)
    others[1, 7] = others[3, 30] = False
    got = env.posture_ik(bad_t, bad_s, host=True, **kw)
    assert _same(got, first, others) and got['status'][1, 7] == 2 and got['status'][3, 30] == 2
    env.close()
    # another N and another K: rows (e, 3 .. 7) of envs 1 .. 3
    env = _env(3)
    sub = env.posture_ik(np.ascontiguousarray(targets[1:4, 3:8]), np.ascontiguousarray(seeds[1:4, 3:8]), host=True, **kw)
    for k in KEYS:
        assert (_bits(sub[k]) == _bits(first[k][1:4, 3:8])).all(), k
    # seeds=None: the env's present joints as the seed, and in no other way
    st = env.state
    st[:, :11] = seeds[1:4, 0]
    st[:, 11:22] = 0.5
    env.state = st
    present = env.read_state()
    env.sync()
    q_now = np.ascontiguousarray(torch.from_dlpack(present).cpu().numpy()[:, None, :11].repeat(5, 1))
    assert (_bits(q_now[:, 0]) == _bits(seeds[1:4, 0])).all()
    t5 = np.ascontiguousarray(targets[1:4, :5])
    assert _same(env.posture_ik(t5, None, host=True, **kw), env.posture_ik(t5, q_now, host=True, **kw))
    assert env.state.tobytes() == st.tobytes()
    env.close()


def test_hostile_rows():
    targets, seeds, _ = _reference('full_clamped')
    t, s = np.array(targets[:3, :5]), np.array(seeds[:3, :5])
    env = _env(3)
    first = env.posture_ik(t, s, host=True)
    t[0, 1, 2] = np.nan
    s[0, 3, 4] = np.inf
    t[1, 2, 3:] = 0.0
    t[2, 4, :3] = (5.0, 0.0, 0.5)
    hostile = [(0, 1), (0, 3), (1, 2), (2, 4)]
    others = np.ones((3, 5), bool)
    for e, k in hostile:
        others[e, k] = False
    for clamp in (True, False):
        ref = first if clamp else env.posture_ik(np.array(targets[:3, :5]), np.array(seeds[:3, :5]), clamp=False, host=True)
        got = env.posture_ik(t, s, clamp=clamp, host=True)                                            # (the call returns success)
        assert [int(got['status'][e, k]) for e, k in hostile] == [2, 2, 2, 1], clamp
        assert np.isfinite(got['residual'][2, 4]) and got['residual'][2, 4] > 3.0 and got['iterations'][2, 4] == 32
        assert np.isfinite(got['posture'][2, 4]).all()
        assert _same(got, ref, others), clamp
    # position only: the quaternion is ignored by the solve -- a zero quaternion is no obstacle
    got = env.posture_ik(t, s, position_only=True, host=True)
    assert [int(got['status'][e, k]) for e, k in hostile] == [2, 2, int(got['residual'][1, 2] >= np.float32(1e-3)), 1]
    assert np.isfinite(got['residual'][1, 2])
    env.close()


def _buffers(env):
    out = []
    for w in range(len(nat.PIK_FIELDS)):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_posture_ik_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_no_effect_on_the_simulation():
    """A handle that asks between steps and a twin that does not: state, observations, preparation record, checkpoint and the
    ik() / get_plan() results stay equal bit for bit over the following steps; the buffers of rr_ik / rr_plan_macro and of the sibling
    queries written before a call are unchanged behind it; the pointers stay, `bytes` follows K."""
    import torch
    from real_robots_amd.distributed import synthetic_actions
    from tests import numpy_posture as npo
    N = 4
    a, b = _env(N), _env(N)
    targets, seeds, _ = _reference('full_clamped')
    t3, s3 = np.ascontiguousarray(targets[:N, :3]), np.ascontiguousarray(seeds[:N, :3])
    t_dev, s_dev = torch.from_numpy(t3).cuda(), torch.from_numpy(s3).cuda()
    torch.cuda.synchronize()
    macro = np.random.default_rng(2).uniform(-0.3, 0.3, (N, 2, 2)).astype(np.float32)
    ik_t = np.ascontiguousarray(targets[:N, 9])
    for env in (a, b):
        env.reset()
        env.set_distance_pairs(npo.robot_pairs(), 0.25)
        for t in range(10):
            env.step(synthetic_actions(list(range(N)), t))
        env.plan_macro(macro)
    b.posture_clearance(s3)
    b.posture_kinematics(s3)
    before = ([b.posture_buffer(w, host=True).tobytes() for w in range(len(nat.PC_FIELDS))],
              [b.posture_kinematics_buffer(w, host=True).tobytes() for w in range(len(nat.PK_FIELDS))], [b.get_plan(e).tobytes() for e in range(N)])
    b.posture_ik(t3, s3)
    ptrs = _buffers(b)
    assert [n for _, n in ptrs] == [N * 3 * 44, N * 3 * 16, N * 3 * 8] and len({p for p, _ in ptrs}) == 3
    b.posture_ik(t_dev, None, position_only=True)
    b.posture_ik(np.ascontiguousarray(targets[:N, :7]), None, point=0, max_iterations=5, clamp=False)
    assert _buffers(b) == [(p, n // 3 * 7) for p, n in ptrs]                                           # another K: the same pointers
    after = ([b.posture_buffer(w, host=True).tobytes() for w in range(len(nat.PC_FIELDS))],
             [b.posture_kinematics_buffer(w, host=True).tobytes() for w in range(len(nat.PK_FIELDS))], [b.get_plan(e).tobytes() for e in range(N)])
    assert before == after
    for t in range(10, 12):                                                                           # the following two steps
        cmd = synthetic_actions(list(range(N)), t)
        a.step(cmd)
        b.step(cmd)
        b.posture_ik(t_dev, s_dev)
    for f in (nat.F_STATE, nat.F_JOINTS, nat.F_TOUCH, nat.F_OBJ_POSE, nat.F_PREP, nat.F_ERRFLAGS, nat.F_CONTACT_COUNT):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    qa, ra = a.ik(ik_t)
    qb, rb = b.ik(ik_t)
    assert qa.tobytes() == qb.tobytes() and ra.tobytes() == rb.tobytes()
    assert all(a.get_plan(e).tobytes() == b.get_plan(e).tobytes() for e in range(N))
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    a.step_plan()
    b.step_plan()
    assert a.host(nat.F_STATE).tobytes() == b.host(nat.F_STATE).tobytes()
    a.close()
    b.close()


def test_refusals_and_buffers():
    import torch
    N = 5
    env = _env(N, objects=2)
    L = env.L
    targets, seeds, _ = _reference('full_clamped')
    t2, s2 = np.ascontiguousarray(targets[:, :2]), np.ascontiguousarray(seeds[:, :2])
    nan, inf = float('nan'), float('inf')
    cases = [((None, s2.ctypes.data, 2, 0, None), 'null targets'), ((t2.ctypes.data, None, 0, 0, None), 'n_targets 0'),
             ((t2.ctypes.data, None, 33, 0, None), 'n_targets 33'), ((t2.ctypes.data, None, -1, 1, None), 'n_targets -1')]
    for field, values, word in (('point', (-1, 1, 8), 'point'), ('max_iterations', (0, -3, 257), 'max_iterations'),
                                ('tolerance', (0.0, -1.0, nan, inf), 'tolerance'), ('damping', (0.0, -0.1, nan, inf), 'damping'),
                                ('max_step', (0.0, -0.5, nan, inf), 'max_step'), ('flags', (4, 7, 0x80000000), 'flag')):
        for v in values:
            opt = nat.IkOptions()
            setattr(opt, field, v)
            cases.append(((t2.ctypes.data, s2.ctypes.data, 2, 0, C.byref(opt)), word))

    def refused():
        for args, word in cases:
            assert L.rr_posture_ik(env.h, *args) == -1, (word, args)
            msg = L.rr_last_error().decode()
            assert 'rr_posture_ik:' in msg and word in msg, msg

    # on a fresh handle: refused first calls, then the buffers as a first look finds them -- K = 0, zero over the whole allocation
    refused()
    before = _buffers(env)
    assert [n for _, n in before] == [0, 0, 0] and all(p for p, _ in before) and len({p for p, _ in before}) == 3
    for name in nat.PIK_FIELDS:
        assert env.posture_ik_buffer(name, host=True).shape[:2] == (N, 0) and env.posture_ik_buffer(name).shape[:2] == (N, 0)
    env.sync()
    for (p, _), row in zip(before, (11, 4, 2)):
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (N * 32 * row,), '<i4', env)).any().item()
    # a valid call works behind them
    st = env.state
    out = env.posture_ik(t2, s2, host=True)
    sizes = [N * 2 * 44, N * 2 * 16, N * 2 * 8]
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    assert (out['status'] == 0).any()
    first = [env.posture_ik_buffer(w, host=True).tobytes() for w in range(3)]
    # refused again: pointers, sizes and contents unchanged; and a valid call behind each kind
    refused()
    p, x = C.c_void_p(), C.c_size_t()
    for which in (3, -1):
        assert L.rr_posture_ik_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_posture_ik_buffer' in L.rr_last_error().decode()
    scratch = np.zeros(4, np.float32)
    assert L.rr_posture_ik_copy_to_host(env.h, 0, scratch.ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    assert L.rr_posture_ik_copy_to_host(env.h, 0, None, sizes[0]) == -1 and 'rr_posture_ik_copy_to_host' in L.rr_last_error().decode()
    assert L.rr_posture_ik_copy_to_host(env.h, 3, scratch.ctypes.data, 16) == -1
    for kw in (dict(point=1), dict(max_iterations=0), dict(max_iterations=257), dict(tolerance=0.0), dict(damping=nan), dict(max_step=inf)):
        with pytest.raises(nat.NativeError, match='rr_posture_ik'):
            env.posture_ik(t2, s2, **kw)
    assert [env.posture_ik_buffer(w, host=True).tobytes() for w in range(3)] == first
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    assert env.state.tobytes() == st.tobytes()
    # the options reach the kernel: NULL options are the defaults; a cap of 1 stops after one update; point 1 exists once it is set
    assert L.rr_posture_ik(env.h, t2.ctypes.data, s2.ctypes.data, 2, 0, None) == 0
    assert [env.posture_ik_buffer(w, host=True).tobytes() for w in range(3)] == first
    one = env.posture_ik(t2, s2, max_iterations=1, host=True)
    assert (one['iterations'] <= 1).all() and (one['iterations'][one['status'] == 1] == 1).all() and (one['status'] == 1).any()
    env.set_kinematic_points([8, 8], [[0, 0, 0], [0, 0, 0.1]])
    moved = env.posture_ik(t2, s2, point=1, host=True)
    assert (moved['posture'] != out['posture']).any()
    with pytest.raises(nat.NativeError, match='point 2'):
        env.posture_ik(t2, s2, point=2)
    assert [p for p, _ in _buffers(env)] == [p for p, _ in before]
    env.close()
