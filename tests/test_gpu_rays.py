"""GPU tests (-m gpu) of the whole-batch ray casts against the collision hulls (rr_ray_cast, include/realrobot.h): the two device
buffers against the independent float64 restatement (tests/numpy_rays.py: world-space clipping, dense, no cull) on states set from
outside and after real steps; the negative controls; bit-identity between the table, host tensors and device tensors, between calls
and across a fork; that the cast has no effect on the simulation; the ray-table API; a height sensor closed through the device; the
vector env's switch and DLPack.

Tolerances (tests/numpy_rays.py, compare): on every DECIDED ray the ids match exactly; |distance error| <= 1e-4 m -- the project's
frame tolerance of 2e-6 on R and p over a lever of at most 1.5 m gives 5e-6 m at the surface and at most 5e-5 m along a ray at
incidence |n . d^| >= 0.1; the bound leaves a factor of two --; the position follows from the distance at the same bound; normals
5e-6 per component; a miss is exactly fraction 1.0, a +0.0 normal and ids -1, with the length and the end point at the same bound.
Fewer than 5 % of the rays may be undecided."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_rays as nr

pytestmark = pytest.mark.gpu

U = np.uint32


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _report(where, fig, fails):
    print(where, {k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in fig.items()}, fails)


def _check(env, out, where, links, segs, variant=None):
    """One cast's host arrays against float64 from env.state; prints every figure before it asserts.  Returns (reference, failures)."""
    N, R = env.N, len(links)
    assert out['hit'].shape == (N, R, 8) and out['hit'].dtype == np.float32 and out['id'].shape == (N, R, 4) and out['id'].dtype == np.int32
    ref = nr.cast(env.state, links, segs, env.n_objects, variant=variant)
    fig, fails = nr.compare(out['hit'], out['id'], ref)
    _report(where, fig, fails)
    return ref, fails


@pytest.fixture(scope='module')
def parity():
    """Both parity cases cast once: {N: (env state, links, segments, {R: (links, segments, device result)})}; the envs are closed."""
    out = {}
    for N, nobj in nr.CASES:
        st, links, segs = nr.case(N, nobj)
        env = BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)
        env.state = st
        assert (_bits(env.state) == _bits(st)).all()
        res = {}
        env.set_rays(links)                                     # R = 64: per-env segments (host path), NULL defaults
        res[64] = (links, segs, env.ray_cast(segs, host=True))
        for R in (1, 5):                                        # R = 1, 5: the table's segments
            l, s = nr.table_rays(R, nr.SEED + 200)
            env.set_rays(l, s)
            res[R] = (l, s, env.ray_cast(host=True))
        out[N] = (st, nobj, res)
        env.close()
    return out


class _State:
    """What the comparisons need of an env whose state is known on the host."""
    def __init__(self, st, nobj):
        self.state, self.n_objects, self.N = st, nobj, len(st)


@pytest.mark.parametrize('N', [n for n, _ in nr.CASES])
@pytest.mark.parametrize('R', [1, 5, 64])
def test_against_float64_on_states_set_from_outside(parity, N, R):
    """N = 3 with one object: fewer envs than any workgroup holds, and the shapes of objects 1, 2 do not exist; N = 131 with three: a
    ragged tail for any power of two.  R = 64: world rays aimed at every shape, short of / beyond the table top, an exact tie, zero
    length, random segments, rays on links 0, 4, 8, finger_01, skin_10 from inside their own hulls and from outside."""
    st, nobj, res = parity[N]
    links, segs, out = res[R]
    ref, fails = _check(_State(st, nobj), out, 'outside N=%d R=%d' % (N, R), links, segs)
    assert not fails, fails
    if R == 64:
        miss = ref['shape'] < 0
        assert (out['id'][miss & ref['decided']] == -1).all()
        world = miss & ref['decided'] & (links < 0)[None, :]
        assert (_bits(out['hit'][..., 2:5][world]) == _bits(segs[..., 3:][world])).all()      # a world ray's end point is the caller's floats
        if N > 100:
            won = np.unique(out['id'][..., 3][ref['decided']])
            assert set(range(22)) <= set(won.tolist()), won


def test_after_real_steps():
    """States that come from the simulator: 60 steps with random commands at N = 131, then the 64 aimed rays."""
    N = 131
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    env.reset()
    rng = np.random.default_rng(7)
    lo, hi = np.array([-2.0] * 7 + [0, 0]), np.array([2.0] * 7 + [1.5, 1.5])
    for t in range(60):
        if t % 20 == 0:
            cmd = rng.uniform(lo, hi, size=(N, 9)).astype(np.float32)
            cmd[:, 8] = np.minimum(cmd[:, 8], 2 * cmd[:, 7])
        env.step(cmd)
    st = env.state
    assert np.isfinite(st).all() and np.abs(st[:, :7]).max() > 0.5
    links, segs = nr.aimed_rays(st, 3, 300)
    env.set_rays(links)
    out = env.ray_cast(segs, host=True)
    ref, fails = _check(env, out, 'steps', links, segs)
    assert not fails, fails
    env.close()


@pytest.mark.parametrize('variant', nr.VARIANTS)
def test_negative_controls(parity, variant):
    """Each deliberately wrong restatement of the rule disagrees with the device on decided rays."""
    st, nobj, res = parity[131]
    links, segs, out = res[64]
    ref, fails = _check(_State(st, nobj), out, variant, links, segs, variant=variant)
    assert [f for f in fails if not f.startswith('undecided')], variant      # (ids, distances or normals -- not merely the cap)


def test_bit_identity_of_paths_calls_and_forks():
    import torch
    N, nobj = 37, 2
    st = nr.states(N, nobj, 21)
    env = BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)
    env.state = st
    links, segs = nr.table_rays(5, 22)
    env.set_rays(links, segs)
    first = env.ray_cast(host=True)
    again = env.ray_cast(host=True)
    tensor = np.ascontiguousarray(np.broadcast_to(segs, (N, 5, 6)))
    by_host = env.ray_cast(tensor, host=True)
    on_dev = _dev(tensor)
    by_dev = env.ray_cast(on_dev, host=True)
    view = env.ray_cast(on_dev)                                 # zero copy: DLPack of the two buffers
    t_hit, t_id = torch.from_dlpack(view['hit']), torch.from_dlpack(view['id'])
    env.sync()
    for name in nat.RAY_FIELDS:
        for other, what in ((again, 'second call'), (by_host, 'host tensor'), (by_dev, 'device tensor')):
            assert (_bits(first[name]) == _bits(other[name])).all(), (name, what)
    assert (t_hit.cpu().numpy().view(U) == _bits(first['hit'])).all() and (t_id.cpu().numpy() == first['id']).all()
    assert (first['id'][..., 3] >= 0).any() and (first['id'][..., 3] < 0).any()
    # a non-finite segment on the device path is a miss; its neighbours are untouched
    bad = tensor.copy()
    bad[1, 2, 4] = np.nan
    bad[2, 0, 0] = np.inf
    out = env.ray_cast(_dev(bad), host=True)
    assert (out['id'][1, 2] == -1).all() and (out['id'][2, 0] == -1).all() and out['hit'][1, 2, 0] == 1.0 and out['hit'][2, 0, 0] == 1.0
    keep = np.ones((N, 5), bool)
    keep[1, 2] = keep[2, 0] = False
    assert (_bits(out['hit'][keep]) == _bits(first['hit'][keep])).all() and (out['id'][keep] == first['id'][keep]).all()
    # ... and on the host path an error that names env and ray, with the buffers as they were
    rc = env.L.rr_ray_cast(env.h, bad.ctypes.data, 0)
    msg = env.L.rr_last_error().decode()
    assert rc == -1 and 'env 1' in msg and 'ray 2' in msg, msg
    assert (_bits(env.ray_buffer('hit', host=True)) == _bits(out['hit'])).all()
    # after a fork a copy's rows equal its source's, bit for bit
    src = np.full(N, -1, np.int32)
    src[[3, 8, 30]] = [20, 20, 5]
    env.fork(src)
    forked = env.ray_cast(host=True)
    for d, s in ((3, 20), (8, 20), (30, 5)):
        assert (_bits(forked['hit'][d]) == _bits(first['hit'][s])).all() and (forked['id'][d] == first['id'][s]).all()
    others = np.setdiff1d(np.arange(N), [3, 8, 30])
    assert (_bits(forked['hit'][others]) == _bits(first['hit'][others])).all()
    env.close()


def test_no_effect_on_the_simulation():
    """40 steps with a cast after each leave state, contact lists, touch, error flags (the checkpoint) and a rendered frame
    bit-identical to 40 steps without."""
    from real_robots_amd.distributed import synthetic_actions
    a = BatchedREALRobotEnv(8, objects=3, width=64, height=64)
    b = BatchedREALRobotEnv(8, objects=3, width=64, height=64)
    a.reset()
    b.reset()
    links, segs = nr.table_rays(5, 23)
    b.set_rays(links, segs)
    for t in range(40):
        cmd = synthetic_actions(list(range(8)), t)
        a.step(cmd, render=(t == 39))
        b.step(cmd, render=(t == 39))
        b.ray_cast()
        if t == 20:
            b.set_rays([-1] * 64, np.tile(np.array([0, 0, 0.9, 0.1, 0.1, 0.0], np.float32), (64, 1)))
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    for f in (nat.F_ERRFLAGS, nat.F_TOUCH, nat.F_RGB, nat.F_DEPTH, nat.F_STATE):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert (b.ray_buffer('id', host=True)[..., 3] >= 0).any()
    a.close()
    b.close()


def _buffers(env):
    out = []
    for w in range(2):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_ray_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_ray_table_api():
    N = 5
    env = BatchedREALRobotEnv(N, objects=2, width=64, height=64)
    L = env.L
    links, segs = env.rays()
    assert links.shape == (0,) and segs.shape == (0, 6)                       # a fresh handle has no rays
    assert L.rr_ray_cast(env.h, None, 0) == -1 and 'rr_ray_cast' in L.rr_last_error().decode()      # R == 0
    with pytest.raises(ValueError):
        env.ray_cast()
    before = _buffers(env)
    assert [n for _, n in before] == [0, 0] and all(p for p, _ in before)
    l5, s5 = nr.table_rays(5, 24)
    env.set_rays(l5, s5)
    assert [n for _, n in _buffers(env)] == [N * 5 * 32, N * 5 * 16]
    assert not _bits(env.ray_buffer('hit', host=True)).any() and not env.ray_buffer('id', host=True).any()      # zero before the first cast
    env.state = nr.states(N, 2, 25)
    first = env.ray_cast(host=True)
    # refused calls: RR_EINVAL, the ray named, nothing changes
    z = np.zeros((65, 6), np.float32)
    nan = z.copy()
    nan[1, 4] = np.nan
    for n, lk, sg, word in ((65, [0] * 65, z, 'ray 64'), (-1, [0], z, 'negative'), (2, [8, 17], z, 'ray 1'), (1, [-2], z, 'ray 0'), (2, [8, 8], nan, 'ray 1')):
        lk = np.array(lk, np.int32)
        assert L.rr_set_rays(env.h, n, lk.ctypes.data, sg.ctypes.data) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_set_rays' in msg and word in msg, msg
    links, segs = env.rays()
    assert list(links) == list(l5) and (_bits(segs) == _bits(s5)).all()
    again = env.ray_cast(host=True)
    assert (_bits(first['hit']) == _bits(again['hit'])).all() and (first['id'] == again['id']).all()
    p, n = C.c_void_p(), C.c_size_t()
    for which in (2, -1):
        assert L.rr_ray_buffer(env.h, which, C.byref(p), C.byref(n)) == -1 and 'rr_ray_buffer' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.ray_buffer('depth')
    with pytest.raises(ValueError):
        env.ray_cast(np.zeros((N, 4, 6), np.float32))
    with pytest.raises(ValueError):
        env.ray_cast(np.zeros((N, 5, 6), np.float64))
    # the table survives reset, set_state and restore
    ck = env.checkpoint()
    env.reset()
    assert list(env.rays()[0]) == list(l5)
    env.state = nr.states(N, 2, 26)
    env.restore(ck)
    assert list(env.rays()[0]) == list(l5) and (_bits(env.rays()[1]) == _bits(s5)).all()
    rest = env.ray_cast(host=True)
    assert (_bits(rest['hit']) == _bits(first['hit'])).all() and (rest['id'] == first['id']).all()
    # a change of R: the same pointers, the sizes follow R; NULL segments are zeros: every ray a miss of zero length
    lk = np.array([8, -1, 0], np.int32)
    nat.check(L.rr_set_rays(env.h, 3, lk.ctypes.data, None))
    after = _buffers(env)
    assert [p for p, _ in after] == [p for p, _ in before] and [n for _, n in after] == [N * 3 * 32, N * 3 * 16]
    out = env.ray_cast(host=True)
    assert out['hit'].shape == (N, 3, 8) and (out['id'] == -1).all() and (out['hit'][..., 0] == 1.0).all() and not out['hit'][..., 1].any()
    assert not _bits(out['hit'][..., 5:8]).any() and not out['hit'][:, 1, 2:5].any()
    env.set_rays([-1] * 64)
    assert [p for p, _ in _buffers(env)] == [p for p, _ in before] and env.ray_cast(host=True)['hit'].shape == (N, 64, 8)
    env.set_rays([])
    assert env.rays()[0].shape == (0,) and L.rr_ray_cast(env.h, None, 0) == -1
    env.close()


def test_a_height_sensor_closes_a_loop_through_the_device():
    """A ray straight down from beside the gripper base, built on the device from the device's own link pose, while a joint
    command lowers the arm for 100 steps: whenever the reference says the table is the first thing under it, the reading is the
    origin's height over the table top (the table hull's top plane) within 1e-4 m."""
    import torch
    from tests import numpy_collide as ncol
    table = ncol.shapes()[0]
    assert np.array_equal(table['N'][2], [0, 0, 1])
    top = float(table['D'][2])
    N = 4
    env = BatchedREALRobotEnv(N, objects=1, width=64, height=64)
    env.reset()
    env.set_rays(['world'])
    target = np.array([0, 0.4, 0, -1.9, 0, 1.0, 0, 0, 0], np.float32)
    offs = torch.tensor([[0.0, -0.12, 0.0], [0.0, 0.12, 0.0], [-0.1, 0.0, 0.0], [0.0, -0.2, 0.0]], device='cuda')
    down = torch.tensor([0.0, 0.0, -1.5], device='cuda')
    n_table, worst, lowest = 0, 0.0, 9.0
    for t in range(100):
        env.step(np.tile(target * (t + 1) / 100.0, (N, 1)))
        pose = torch.from_dlpack(env.kinematic_observations()['link_pose'])
        env.sync()
        origin = pose[:, nat.EE_LINK, :3] + offs
        rays = torch.cat([origin, origin + down], 1).reshape(N, 1, 6).contiguous()
        torch.cuda.synchronize()
        out = env.ray_cast(rays, host=True)
        ref = nr.cast(env.state, [-1], rays.cpu().numpy(), 1)
        sel = ref['decided'][:, 0] & (ref['shape'][:, 0] == 0)
        n_table += int(sel.sum())
        if sel.any():
            assert (out['id'][sel, 0, 3] == 0).all() and (out['id'][sel, 0, 0] == nr.shape_ids()[0, 0]).all(), t
            height = origin.cpu().numpy().astype(np.float64)[:, 2] - top
            err = np.abs(out['hit'][sel, 0, 1] - height[sel]).max()
            worst, lowest = max(worst, float(err)), min(lowest, float(height[sel].min()))
            assert err <= nr.TOL_DIST, (t, err)
    print("height sensor: %d readings over the table, lowest %.3f m, worst error %.2e m" % (n_table, lowest, worst))
    assert n_table >= 150 and lowest < 0.3
    env.close()


def test_vector_env_switch_and_dlpack():
    import torch
    from real_robots_amd.envs.robot import Kuka
    from real_robots_amd.vector import REALRobotVectorEnv
    kw = dict(objects=1, eye_width=64, eye_height=64)
    base = Kuka(False, 1, 64, 64, env=None).observation_space
    plain = REALRobotVectorEnv(2, **kw)
    obs, _ = plain.reset(seed=0)
    assert not {'ray_distance', 'ray_uid'} & set(obs) and set(plain.single_observation_space.spaces) == set(base.spaces) == set(plain.observation_space.spaces)
    plain.close()
    links, segs = nr.table_rays(5, 27)
    v = REALRobotVectorEnv(2, ray_sensors=(['base', 'world', 0, 4, 'finger_01'], segs), **kw)
    assert list(v._be.rays()[0]) == list(links)
    assert set(v.single_observation_space.spaces) == set(base.spaces) | {'ray_distance', 'ray_uid'}
    cmd = np.tile(np.array([0.3, 0.5, 0, -0.8, 0, 0.6, 0, 0.5, 0.2], np.float32), (2, 1))
    obs0, _ = v.reset(seed=0)
    obs1 = v.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    for obs in (obs0, obs1):
        for key, dt in (('ray_distance', np.float32), ('ray_uid', np.int32)):
            sp = v.single_observation_space[key]
            assert sp.shape == (5,) and sp.dtype == dt and v.observation_space[key].shape == (2, 5), key
            assert obs[key].shape == (2, 5) and obs[key].dtype == dt and v.observation_space[key].contains(np.ascontiguousarray(obs[key])), key
    back = v._be.ray_cast(host=True)
    assert (_bits(obs1['ray_distance']) == _bits(back['hit'][..., 1])).all() and (obs1['ray_uid'] == back['id'][..., 0]).all()
    assert (obs1['ray_uid'] >= 0).any() and (obs1['ray_distance'] != obs0['ray_distance']).any()
    v.close()
    d = REALRobotVectorEnv(2, device_obs=True, ray_sensors=(links, segs), **kw)
    d.reset(seed=0)
    obs = d.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    assert obs['ray_distance'].shape == (2, 5) and obs['ray_distance'].typestr == np.dtype(np.float32).str
    td, tu = torch.from_dlpack(obs['ray_distance']), torch.from_dlpack(obs['ray_uid'])
    d._be.sync()
    host = d._be.ray_cast(host=True)
    assert td.is_cuda and tuple(td.shape) == (2, 5) and tuple(tu.shape) == (2, 5) and tu.dtype == torch.int32
    assert (td.cpu().numpy().view(U) == _bits(host['hit'][..., 1])).all() and (tu.cpu().numpy() == host['id'][..., 0]).all()
    assert (_bits(host['hit'][..., 1]) == _bits(back['hit'][..., 1])).all()
    d.close()
    with pytest.raises(ValueError):
        REALRobotVectorEnv(2, ray_sensors=(['no_such_link'], None), **kw)
