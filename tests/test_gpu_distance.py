"""GPU tests (-m gpu) of the whole-batch closest-point queries between collision hulls (rr_closest_points, include/realrobot.h): the
two device buffers against the independent float64 reference (tests/numpy_distance.py: qhull on the Minkowski difference, no GJK) on
states set from outside and after real steps; the negative controls; bit-identity between calls, batch sizes, forks, permuted tables
and host / device copies; that the query has no effect on the simulation; the pair-table API; the cull; a non-finite env; the vector
env's switch and DLPack.

Tolerance.  TOL bounds |distance - exact|, lower bound - exact, the closest vector (through the projection inequality) and how far
a and b may lie outside their hulls, on every DECIDED item (|exact| >= 1 mm).  It is four times the largest |distance - exact|
measured on the MI355X over the decided items of test 1 (MEASURED; the factor covers other seeds and compiler versions), and it must
stay below a tenth of the smallest error a negative control shows (test_negative_controls asserts it): anything larger would be a
wrong algorithm, not rounding.  profiles/distance_bench.json carries both figures.  What follows from float32 rounding alone --
|a - b| against distance, n against (a - b) / distance -- is held to numpy_distance.R32 instead."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_collide as ncol
from tests import numpy_distance as nd

pytestmark = pytest.mark.gpu

U = np.uint32
MEASURED = 1.71e-7            # m: the largest |distance - exact| over the decided items of test 1 on the MI355X (N = 5, Q = 7: link_7 against the robot's base, 1.05 m apart)
TOL = 4 * MEASURED


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _same(x, y, rows=None):
    """two results of closest_points(host=True), bit for bit (on the rows given)"""
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    return all((_bits(sel(x[k])) == _bits(sel(y[k]))).all() for k in x)


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _report(where, fig, fails):
    print(where, {k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in fig.items()}, fails)


def _env(N, nobj=3):
    return BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)


_device = {}


def _case(N):
    """(state, pairs, reference, device result) of a parity case: the device is asked once per process."""
    st, pairs, ref = nd.case(N)
    if N not in _device:
        env = _env(N)
        env.state = st
        assert (_bits(env.state) == _bits(st)).all()
        env.set_distance_pairs('collision' if len(pairs) > 7 else pairs)
        assert (env.distance_pairs()[0] == pairs).all()
        _device[N] = _copy(env.closest_points(host=True))
        env.close()
    return st, pairs, ref, _device[N]


@pytest.mark.parametrize('N', [n for n, _, _ in nd.cases()])
def test_against_float64_on_states_set_from_outside(N):
    """N = 1 with the 92 pairs of 'collision', N = 5 with seven pairs of every vertex-count class, N = 67 with one: random postures
    and object poses, the cube 5 mm above the table with parallel faces, an object between the fingers, overlapping objects."""
    st, pairs, ref, out = _case(N)
    assert out['distance'].shape == (N, len(pairs)) and out['point_a'].shape == (N, len(pairs), 3) and out['status'].dtype == np.int32
    fig, fails = nd.compare(out, ref, TOL, pairs)
    _report('outside N=%d Q=%d' % (N, len(pairs)), fig, fails)
    assert not fails, fails
    assert fig['decided'] >= 0.9 * fig['items'] and fig['overlapping'] >= 1
    body = np.array([ncol.body_id(s) for s in ncol.shapes()])
    assert (out['body_a'] == body[pairs[:, 0]][None]).all() and (out['body_b'] == body[pairs[:, 1]][None]).all()
    assert (out['iterations'][out['status'] != 2] >= 1).all() and out['iterations'].max() <= 32
    if N == 1:
        cube, table, tomato = (nd.names()[k] for k in ('cube', 'table', 'tomato'))
        j = [tuple(p) for p in pairs.tolist()].index((cube, table))
        assert abs(out['distance'][0, j] - 0.005) <= 1e-5 and abs(out['normal'][0, j, 2] - 1.0) <= 1e-5      # parallel faces, 5 mm apart
        assert out['status'][0, [tuple(p) for p in pairs.tolist()].index((cube, tomato))] == 1


def test_after_real_steps():
    """States that come from the simulator: a reach-and-close command sequence over 60 steps at N = 5 with the 'collision' table.
    Resting contacts are undecided: they are only required to be finite with status 0 or 1."""
    N = 5
    env = _env(N)
    env.reset()
    env.set_distance_pairs('collision')
    rng = np.random.default_rng(11)
    base = np.array([0.0, 0.9, 0.0, -1.3, 0.0, 0.9, 0.0, 0.0, 0.0])
    for t in range(60):
        if t % 20 == 0:
            cmd = (base + np.concatenate([rng.uniform(-0.4, 0.4, size=(N, 7)), np.zeros((N, 2))], 1)).astype(np.float32)
            cmd[:, 7] = 0.8 * (t >= 20)
            cmd[:, 8] = 0.8 * (t >= 40)
        env.step(cmd)
    st = env.state
    assert np.isfinite(st).all() and np.abs(st[:, :7]).max() > 0.5
    out = _copy(env.closest_points(host=True))
    env.close()
    pairs = nd.collision_pairs(3)
    ref = nd.reference(st, pairs)
    fig, fails = nd.compare(out, ref, TOL, pairs)
    _report('steps', fig, fails)
    assert not fails, fails
    assert all(np.isfinite(out[k]).all() for k in ('distance', 'lower', 'point_a', 'point_b', 'normal')) and np.isin(out['status'], (0, 1)).all()
    assert (~ref['decided']).any() or fig['overlapping'] + fig['separated'] == fig['items']


@pytest.mark.parametrize('variant', nd.VARIANTS)
def test_negative_controls(variant):
    """Each deliberately wrong restatement disagrees with the device on decided items, by far more than TOL."""
    st, pairs, ref, out = _case(5)
    var = nd.case(5, variant=variant)[2]
    fig, fails = nd.compare(out, var, TOL, pairs)
    err = nd.control_error(ref, var)
    _report(variant, dict(fig, control_error=err), fails)
    assert fails, variant
    assert TOL < 0.1 * err, (TOL, err)


def test_bit_identity_of_calls_batches_forks_tables_and_copies():
    import torch
    s1, pairs, _, one = _case(5)
    N = 67
    st = nd.states(N, nd.SEED + 2)
    st[66] = s1[0]
    env = _env(N)
    env.state = st
    env.set_distance_pairs(pairs)
    first = _copy(env.closest_points(host=True))
    again = _copy(env.closest_points(host=True))
    assert _same(first, again)
    assert _same({k: v[66] for k, v in first.items()}, {k: v[0] for k, v in one.items()})          # env 66 of 67 == env 0 of 5
    lone = _env(1)
    lone.state = s1[:1]
    lone.set_distance_pairs(pairs)
    assert _same({k: v[0] for k, v in _copy(lone.closest_points(host=True)).items()}, {k: v[66] for k, v in first.items()})
    lone.close()
    # host and device copies of the two buffers
    view = env.closest_points()
    t = {k: torch.from_dlpack(v) for k, v in view.items()}
    env.sync()
    for k, v in t.items():
        assert v.is_cuda and (_bits(v.cpu().numpy()) == _bits(first[k])).all(), k
    dev_pts = torch.from_dlpack(env.distance_buffer('points'))
    assert (_bits(dev_pts.cpu().numpy()) == _bits(env.distance_buffer('points', host=True))).all()
    assert not _bits(env.distance_buffer('points', host=True)[..., 11]).any()                        # the pad column is +0.0
    # a permuted table gives permuted rows
    perm = np.array([3, 0, 6, 5, 1, 4, 2])
    env.set_distance_pairs(pairs[perm])
    shuffled = _copy(env.closest_points(host=True))
    assert _same({k: v[:, perm] for k, v in first.items()}, shuffled)
    env.set_distance_pairs(pairs)
    # after a fork a copy's rows equal its source's, bit for bit
    src = np.full(N, -1, np.int32)
    src[[3, 8, 30]] = [20, 20, 66]
    env.fork(src)
    forked = _copy(env.closest_points(host=True))
    for d, s in ((3, 20), (8, 20), (30, 66)):
        assert _same({k: v[d] for k, v in forked.items()}, {k: v[s] for k, v in first.items()})
    others = np.setdiff1d(np.arange(N), [3, 8, 30])
    assert _same(forked, first, rows=others)
    env.close()


def test_no_effect_on_the_simulation():
    """40 steps with a query after each leave state, contact lists, touch, error flags (the checkpoint) and a rendered frame
    bit-identical to 40 steps without."""
    from real_robots_amd.distributed import synthetic_actions
    a, b = _env(8), _env(8)
    a.reset()
    b.reset()
    b.set_distance_pairs(nd.seven_pairs(), 0.05)
    for t in range(40):
        cmd = synthetic_actions(list(range(8)), t)
        a.step(cmd, render=(t == 39))
        b.step(cmd, render=(t == 39))
        b.closest_points()
        if t == 20:
            b.set_distance_pairs('collision')
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    for f in (nat.F_ERRFLAGS, nat.F_TOUCH, nat.F_RGB, nat.F_DEPTH, nat.F_STATE):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert (b.distance_buffer('points', host=True)[..., 0] > 0).any()
    a.close()
    b.close()


def _buffers(env):
    out = []
    for w in range(2):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_distance_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_pair_table_api():
    N = 5
    env = _env(N, nobj=2)
    L = env.L
    pairs, md = env.distance_pairs()
    assert pairs.shape == (0, 2) and md == 0.0                                  # a fresh handle has no pairs
    assert L.rr_closest_points(env.h) == -1 and 'rr_closest_points' in L.rr_last_error().decode()      # Q == 0
    with pytest.raises(ValueError):
        env.closest_points()
    before = _buffers(env)
    assert [n for _, n in before] == [0, 0] and all(p for p, _ in before)
    n = nd.names()
    p3 = np.array([(n['cube'], n['table']), (n['skin_00'], n['tomato']), (n['base'], n['shelf'])], np.int32)
    env.set_distance_pairs(p3, 0.25)
    assert [x for _, x in _buffers(env)] == [N * 3 * 48, N * 3 * 16]
    assert not _bits(env.distance_buffer('points', host=True)).any() and not env.distance_buffer('id', host=True).any()      # zero before the first query
    env.state = nd.states(N, 41)
    first = _copy(env.closest_points(host=True))
    # refused calls: RR_EINVAL, the pair named, nothing changes
    i32 = lambda x: np.array(x, np.int32)
    bad = ((97, i32([0] * 97), i32([1] * 97), 0.0, 'pair 96'), (-2, i32([0]), i32([1]), 0.0, '-2'), (2, i32([0, 22]), i32([1, 1]), 0.0, 'pair 1'),
           (2, i32([0, 3]), i32([1, -1]), 0.0, 'pair 1'), (1, i32([4]), i32([4]), 0.0, 'pair 0'), (2, i32([0, 0]), i32([1, n['mustard']]), 0.0, 'pair 1'),
           (1, i32([0]), i32([1]), float('nan'), 'NaN'))
    for q, a, b, m, word in bad:
        assert L.rr_set_distance_pairs(env.h, q, a.ctypes.data, b.ctypes.data, m) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_set_distance_pairs' in msg and word in msg, msg
    assert L.rr_set_distance_pairs(env.h, 1, None, None, 0.0) == -1 and 'null' in L.rr_last_error().decode()
    pairs, md = env.distance_pairs()
    assert (pairs == p3).all() and md == np.float32(0.25)
    assert _same(first, _copy(env.closest_points(host=True)))
    p, x = C.c_void_p(), C.c_size_t()
    for which in (2, -1):
        assert L.rr_distance_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_distance_buffer' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.distance_buffer('depth')
    # the table survives reset, set_state and restore
    ck = env.checkpoint()
    env.reset()
    assert (env.distance_pairs()[0] == p3).all()
    env.state = nd.states(N, 42)
    env.restore(ck)
    assert (env.distance_pairs()[0] == p3).all() and env.distance_pairs()[1] == np.float32(0.25)
    assert _same(first, _copy(env.closest_points(host=True)))
    # -1: the step's own collision pairs, those of the objects the handle has
    env.set_distance_pairs('collision')
    want = nd.collision_pairs(2)
    assert (env.distance_pairs()[0] == want).all() and env.distance_pairs()[1] == 0.0
    after = _buffers(env)
    assert [p for p, _ in after] == [p for p, _ in before] and [x for _, x in after] == [N * len(want) * 48, N * len(want) * 16]
    assert env.closest_points(host=True)['distance'].shape == (N, len(want))
    full = _env(1)
    full.set_distance_pairs('collision')
    assert (full.distance_pairs()[0] == nd.collision_pairs(3)).all() and len(nd.collision_pairs(3)) == 92
    full.set_distance_pairs([(0, 1)] * 96)
    assert full.closest_points(host=True)['status'].shape == (1, 96)
    full.close()
    env.set_distance_pairs([])
    assert env.distance_pairs()[0].shape == (0, 2) and L.rr_closest_points(env.h) == -1
    assert [p for p, _ in _buffers(env)] == [p for p, _ in before]
    env.close()


def test_cull():
    """max_distance = 5 cm: decided far items have status 2 and the reference's sphere gap; near items are bit for bit the unculled
    result."""
    st, pairs, _, plain = _case(1)
    ref = nd.case(1, max_distance=0.05)[2]
    env = _env(1)
    env.state = st
    env.set_distance_pairs('collision', 0.05)
    out = _copy(env.closest_points(host=True))
    env.close()
    fig, fails = nd.compare(out, ref, TOL, pairs)
    _report('cull', fig, fails)
    assert not fails, fails
    assert fig['culled'] >= 10 and fig['separated'] + fig['overlapping'] >= 10
    far = out['status'] == 2
    assert (out['iterations'][far] == 0).all() and _same(out, plain, rows=~far)
    u = out['point_a'][far].astype(np.float64) - out['point_b'][far]
    assert np.abs(np.linalg.norm(u, axis=-1) - out['distance'][far]).max() <= nd.R32
    assert np.abs(u / np.linalg.norm(u, axis=-1, keepdims=True) - out['normal'][far]).max() <= 1e-5


def test_non_finite_state_in_one_env():
    """A NaN object pose in one env: the call returns, the stream syncs, every other env's rows are bit for bit those of a run
    without it (the loop bounds do not depend on data)."""
    st, pairs, _, plain = _case(5)
    env = _env(5)
    env.state = st
    env.set_distance_pairs(pairs)
    bad = st.copy()
    bad[2, 22:29] = np.nan
    env.write_state(bad, np.array([0, 0, 1, 0, 0], np.uint8), obj_pose=True)
    out = _copy(env.closest_points(host=True))
    env.sync()
    env.close()
    assert _same(out, plain, rows=[0, 1, 3, 4])
    assert np.isin(out['status'][2], (0, 1, 2, 3)).all() and (out['iterations'][2] <= 32).all()


def test_vector_env_switch_and_dlpack():
    import torch
    from real_robots_amd.envs.robot import Kuka
    from real_robots_amd.vector import REALRobotVectorEnv
    kw = dict(objects=1, eye_width=64, eye_height=64)
    base = Kuka(False, 1, 64, 64, env=None).observation_space
    plain = REALRobotVectorEnv(2, **kw)
    obs, _ = plain.reset(seed=0)
    assert not {'pair_distance', 'pair_status'} & set(obs) and set(plain.single_observation_space.spaces) == set(base.spaces)
    plain.close()
    pairs = [('skin_00', 'cube'), ('skin_10', 'cube'), ('cube', 'table')]
    v = REALRobotVectorEnv(2, distance_pairs=pairs, distance_max=2.0, **kw)
    assert set(v.single_observation_space.spaces) == set(base.spaces) | {'pair_distance', 'pair_status'}
    cmd = np.tile(np.array([0.3, 0.5, 0, -0.8, 0, 0.6, 0, 0.5, 0.2], np.float32), (2, 1))
    obs0, _ = v.reset(seed=0)
    obs1 = v.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    for obs in (obs0, obs1):
        for key, dt in (('pair_distance', np.float32), ('pair_status', np.int32)):
            sp = v.single_observation_space[key]
            assert sp.shape == (3,) and sp.dtype == dt and v.observation_space[key].shape == (2, 3), key
            assert obs[key].shape == (2, 3) and obs[key].dtype == dt and v.observation_space[key].contains(np.ascontiguousarray(obs[key])), key
    back = _copy(v._be.closest_points(host=True))
    assert (_bits(obs1['pair_distance']) == _bits(back['distance'])).all() and (obs1['pair_status'] == back['status']).all()
    assert (obs1['pair_distance'][:, :2] > 0).all() and (obs1['pair_distance'] != obs0['pair_distance']).any()
    v.close()
    c = REALRobotVectorEnv(2, distance_pairs='collision', **kw)
    assert c.single_observation_space['pair_distance'].shape == (len(nd.collision_pairs(1)),) == (len(c._be.distance_pairs()[0]),)
    c.close()
    d = REALRobotVectorEnv(2, device_obs=True, distance_pairs=pairs, distance_max=2.0, **kw)
    d.reset(seed=0)
    obs = d.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    assert obs['pair_distance'].shape == (2, 3) and obs['pair_distance'].typestr == np.dtype(np.float32).str
    td, ts = torch.from_dlpack(obs['pair_distance']), torch.from_dlpack(obs['pair_status'])
    d._be.sync()
    assert td.is_cuda and tuple(td.shape) == (2, 3) and ts.dtype == torch.int32
    assert (_bits(td.cpu().numpy()) == _bits(back['distance'])).all() and (ts.cpu().numpy() == back['status']).all()
    d.close()
    with pytest.raises(ValueError):
        REALRobotVectorEnv(2, distance_pairs=[('no_such_shape', 'cube')], **kw)
