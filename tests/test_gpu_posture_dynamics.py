"""GPU tests (-m gpu) of the joint-space dynamics at candidate postures (rr_posture_dynamics, include/realrobot.h): the mass matrix,
the gravity torques, the bias, the inverse dynamics and M^-1 of K rows per env against tests/numpy_step.py in float64 at the float32
inputs (tests/numpy_dynamics.py: M from the body Jacobians, the bias from the Lagrangian by complex step -- the device runs composite
bodies and Newton-Euler); the structure of the buffers bit for bit; that a row is a function of its inputs alone; the present-state
form; that the call has no effect on the simulation; refusals, non-finite rows and the vector env's switch.

Ceilings (tests/numpy_dynamics.py has the formulas): mass_matrix C_M = 2e-5 of sqrt(M_ii M_jj); gravity, bias, torque C_V = 2e-5 of
the error scale in the mass metric; mass_inverse 1e-4 of sqrt(Minv_ii Minv_jj).  tests/test_numpy_dynamics.py shows that the wrong
references -- no rotational inertia, no Coriolis terms, a body's mass off by 1 % -- miss them on every row of these inputs.

MEASURED on the MI355X, the worst ratio to the ceiling over all rows (every test prints its own; no ceiling was raised): the table
MEASURED below -- at most 0.22 of the ceiling for M (4.4e-6 of sqrt(M_ii M_jj)), 0.21 for the vectors, 0.18 for M^-1."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_dynamics as nd
from tests.test_gpu_kinematic_obs import _random_state

pytestmark = pytest.mark.gpu

U = np.uint32
VECTORS = ('gravity', 'bias', 'torque')
# worst ratio to the ceiling on the MI355X: (N, K) of test_against_float64, or test_present_state -> field -> ratio (a record, not a bound)
MEASURED = {
    (3, 1): dict(mass_matrix=0.0709, gravity=0.0213, bias=0.0125, torque=0.0163, mass_inverse=0.032),
    (5, 3): dict(mass_matrix=0.116, gravity=0.0236, bias=0.0252, torque=0.044, mass_inverse=0.123),
    (37, 32): dict(mass_matrix=0.222, gravity=0.0925, bias=0.0672, torque=0.0705, mass_inverse=0.175),
    'present_state': dict(mass_matrix=0.159, gravity=0.204, bias=0.207, torque=0.109, mass_inverse=0.0817),
}


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _env(N, objects=3, **kw):
    return BatchedREALRobotEnv(N, objects=objects, width=64, height=64, **kw)


def _same(a, b, names=nat.PD_FIELDS):
    return all((_bits(a[k]) == _bits(b[k])).all() for k in names if k in a and k in b)


def _ratios(out, ref, qdd):
    scale = nd.scales(ref, qdd)
    return {k: float(nd.row_ratios(out[k], ref, scale, k).max()) for k in nat.PD_FIELDS if k in out}


@pytest.mark.parametrize('N,K', nd.SHAPES)
def test_against_float64(N, K):
    """3, 15 and 1 184 rows: the first two leave a ragged last group for any rows-per-wave of 4 and up and any rows-per-workgroup up
    to 64, 1 184 = 18 x 64 + 32.  Every eighth row is an edge row (tests/numpy_dynamics.inputs).  The env holds a random state far
    from every candidate: a kernel that read the state instead of the tensors fails."""
    import torch
    env = _env(N)
    rng = np.random.default_rng(100 + N)
    env.state = _random_state(env, rng)
    st = env.state
    q, qd, qdd = nd.inputs(N, K)
    assert np.abs(q[:, :, :7] - st[:, None, :7]).max(-1).min() > 0.05
    out = env.posture_dynamics(q, qd, qdd, inverse=True, host=True)
    assert [out[k].shape for k in nat.PD_FIELDS] == [(N, K, 11, 11), (N, K, 11), (N, K, 11), (N, K, 11), (N, K, 11, 11)]
    assert all(out[k].dtype == np.float32 for k in nat.PD_FIELDS)
    ref = nd.reference_of_inputs(N, K)
    fig = _ratios(out, ref, qdd)
    print((N, K), 'worst ratio to the ceiling', {k: float('%.3g' % v) for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= 1.0, (k, v)
    # the structure holds on these rows too
    M = out['mass_matrix']
    assert (_bits(M) == _bits(M.transpose(0, 1, 3, 2))).all()
    assert not _bits(M[:, :, 7:9, 9:11]).any() and not _bits(M[:, :, 9:11, 7:9]).any()
    # CUDA torch tensors read in place: the bits of the staged host arrays
    t = [torch.from_numpy(np.array(a)).cuda() for a in (q, qd, qdd)]
    torch.cuda.synchronize()
    view = env.posture_dynamics(*t, inverse=True)
    dev = {k: torch.from_dlpack(v) for k, v in view.items()}
    env.sync()
    for k in nat.PD_FIELDS:
        assert dev[k].is_cuda and tuple(dev[k].shape) == out[k].shape and (_bits(dev[k].cpu().numpy()) == _bits(out[k])).all(), k
    assert env.state.tobytes() == st.tobytes()
    env.close()


def test_structure_bit_for_bit():
    N, K = 5, 3
    env = _env(N)
    q, qd, qdd = nd.inputs(N, K)
    full = env.posture_dynamics(q, qd, qdd, inverse=True, host=True)
    M = full['mass_matrix']
    assert (_bits(M) == _bits(M.transpose(0, 1, 3, 2))).all()                                        # symmetric
    assert not _bits(M[:, :, 7:9, 9:11]).any() and not _bits(M[:, :, 9:11, 7:9]).any()               # sixteen entries, +0.0
    assert (M[:, :, np.arange(11), np.arange(11)] > 0).all()
    # without velocities bias has the bytes of gravity; without accelerations torque has the bytes of bias
    no_v = env.posture_dynamics(q, None, qdd, host=True)
    assert 'mass_inverse' not in no_v
    assert (_bits(no_v['bias']) == _bits(no_v['gravity'])).all() and (_bits(no_v['gravity']) == _bits(full['gravity'])).all()
    assert (_bits(no_v['torque']) != _bits(no_v['bias'])).any()
    no_a = env.posture_dynamics(q, qd, None, host=True)
    assert (_bits(no_a['torque']) == _bits(no_a['bias'])).all() and (_bits(no_a['bias']) == _bits(full['bias'])).all()
    assert (_bits(no_a['bias']) != _bits(no_a['gravity'])).any()
    bare = env.posture_dynamics(q, host=True)
    assert (_bits(bare['torque']) == _bits(bare['gravity'])).all() and (_bits(bare['bias']) == _bits(bare['gravity'])).all()
    assert (_bits(bare['mass_matrix']) == _bits(M)).all()
    # without the flag mass_inverse keeps the bytes of the previous call -- here those of `full`, though the postures differ now
    other = np.ascontiguousarray(q[::-1])
    env.posture_dynamics(other, qd, qdd)
    assert (_bits(env.posture_dynamics_buffer('mass_inverse', host=True)) == _bits(full['mass_inverse'])).all()
    assert (_bits(env.posture_dynamics_buffer('mass_matrix', host=True)) != _bits(M)).any()
    again = env.posture_dynamics(other, qd, qdd, inverse=True, host=True)
    assert (_bits(again['mass_inverse']) == _bits(full['mass_inverse'][::-1])).all()
    env.close()


def test_a_row_is_a_function_of_its_inputs_alone():
    import torch
    N, K = 6, 5
    q, qd, qdd = nd.inputs(N, K)
    a = _env(N)
    rng = np.random.default_rng(31)
    a.state = _random_state(a, rng)
    first = a.posture_dynamics(q, qd, qdd, inverse=True, host=True)
    assert _same(first, a.posture_dynamics(q, qd, qdd, inverse=True, host=True))                      # two calls in a row
    # the same rows permuted across envs and K: the same bytes per row
    perm = rng.permutation(N * K)
    sh = lambda x: np.ascontiguousarray(x.reshape(N * K, 11)[perm].reshape(N, K, 11))
    shuffled = a.posture_dynamics(sh(q), sh(qd), sh(qdd), inverse=True, host=True)
    for name in nat.PD_FIELDS:
        rows = first[name].reshape((N * K,) + first[name].shape[2:])
        assert (_bits(shuffled[name].reshape(rows.shape)) == _bits(rows[perm])).all(), name
    # another K: row k alone
    alone = a.posture_dynamics(*(np.ascontiguousarray(x[:, 2:3]) for x in (q, qd, qdd)), inverse=True, host=True)
    for name in nat.PD_FIELDS:
        assert (_bits(alone[name][:, 0]) == _bits(first[name][:, 2])).all(), name
    # a second handle in another state, with other object dynamics and other actuators: identical buffers
    b = _env(N, objects=2)
    b.state = _random_state(b, rng)
    b.set_object_dynamics(mass=0.7, friction=0.2)
    b.set_env_actuators(kp=0.3, kd=0.8, max_force=50.0, damping=rng.uniform(0.0, 2.0, (N, 11)).astype(np.float32))
    for t in range(3):
        b.step(rng.uniform(-1, 1, (N, 9)).astype(np.float32))
    assert np.abs(a.state[:, :22] - b.state[:, :22]).max() > 0.5
    assert _same(first, b.posture_dynamics(q, qd, qdd, inverse=True, host=True))
    # a device call on the same values: identical buffers
    t = [torch.from_numpy(np.array(x)).cuda() for x in (q, qd, qdd)]
    torch.cuda.synchronize()
    b.posture_dynamics(*t, inverse=True)
    assert _same(first, {name: b.posture_dynamics_buffer(name, host=True) for name in nat.PD_FIELDS})
    a.close()
    b.close()


def test_present_state():
    """postures=None after 20 random steps from reset: q and qd are the env's own.  Worst ratios on the MI355X: MEASURED['present_state']."""
    N = 37
    env = _env(N)
    env.reset()
    rng = np.random.default_rng(3)
    for t in range(20):
        env.step(rng.uniform(-1, 1, (N, 9)).astype(np.float32))
    st = env.state
    assert np.abs(st[:, 11:22]).max() > 0.1
    qdd = rng.uniform(-10, 10, (N, 1, 11)).astype(np.float32)
    out = env.posture_dynamics(accelerations=qdd, inverse=True, host=True)
    assert out['mass_matrix'].shape == (N, 1, 11, 11) and out['bias'].shape == (N, 1, 11)
    ref = nd.reference(st[:, None, :11], st[:, None, 11:22], qdd)
    fig = _ratios(out, ref, qdd)
    print('present state: worst ratio to the ceiling', {k: float('%.3g' % v) for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= 1.0, (k, v)
    # the same rows given as tensors: the same bytes
    as_rows = env.posture_dynamics(np.ascontiguousarray(st[:, None, :11]), np.ascontiguousarray(st[:, None, 11:22]), qdd, inverse=True, host=True)
    assert _same(out, as_rows)
    bare = env.posture_dynamics(host=True)
    assert (_bits(bare['torque']) == _bits(bare['bias'])).all() and (_bits(bare['bias']) == _bits(out['bias'])).all()
    # velocities with postures=None are refused, by the binding and by the library
    with pytest.raises(ValueError):
        env.posture_dynamics(None, np.zeros((N, 1, 11), np.float32))
    v = np.zeros((N, 1, 11), np.float32)
    assert env.L.rr_posture_dynamics(env.h, None, v.ctypes.data, None, 1, 0, 0) == -1
    assert 'rr_posture_dynamics: velocities without postures' in env.L.rr_last_error().decode()
    assert env.L.rr_posture_dynamics(env.h, None, None, None, 2, 0, 0) == -1 and 'without postures' in env.L.rr_last_error().decode()
    assert env.state.tobytes() == st.tobytes()
    env.close()


def test_no_effect_on_the_simulation():
    """Two handles run the same 10 actions; one calls posture_dynamics before every step -- candidates on the device and the
    present-state form: state, observations and contact counts stay bit-identical after every step."""
    import torch
    N, K = 8, 3
    a, b = _env(N), _env(N)
    rng = np.random.default_rng(5)
    for env in (a, b):
        env.reset()
    q, qd, qdd = nd.inputs(5, 3)
    dev = [torch.from_numpy(np.ascontiguousarray(np.resize(x, (N, K, 11)))).cuda() for x in (q, qd, qdd)]
    torch.cuda.synchronize()
    fields = (nat.F_STATE, nat.F_JOINTS, nat.F_TOUCH, nat.F_OBJ_POSE, nat.F_CONTACT_COUNT, nat.F_ERRFLAGS, nat.F_PREP)
    for t in range(10):
        cmd = rng.uniform(-1, 1, (N, 9)).astype(np.float32)
        b.posture_dynamics(*dev, inverse=bool(t % 2))
        b.posture_dynamics(inverse=not t % 2)
        a.step(cmd, render=(t == 9))
        b.step(cmd, render=(t == 9))
        for f in fields:
            assert a.host(f).tobytes() == b.host(f).tobytes(), (t, f)
    for f in (nat.F_RGB, nat.F_DEPTH):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert np.abs(b.posture_dynamics_buffer('mass_matrix', host=True)).max() > 0.1
    a.close()
    b.close()


def _buffers(env):
    out = []
    for w in range(len(nat.PD_FIELDS)):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_posture_dynamics_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_refusals_and_non_finite_rows():
    import torch
    N, K = 5, 3
    env = _env(N, objects=2)
    L = env.L
    before = _buffers(env)
    assert [n for _, n in before] == [0] * 5 and all(p for p, _ in before) and len({p for p, _ in before}) == 5      # K counts as 0
    env.sync()
    for (p, _), row in zip(before, (121, 11, 11, 11, 121)):                                          # zero-filled over the whole allocation
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (N * 32 * row,), '<i4', env)).any().item()
    q, qd, qdd = (np.array(x) for x in nd.inputs(N, K))
    first = env.posture_dynamics(q, qd, qdd, inverse=True, host=True)
    sizes = [N * K * r * 4 for r in (121, 11, 11, 11, 121)]
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    # refused: K = 0, K = 33, unknown flags, a bad buffer index, a null destination, a size mismatch -- RR_EINVAL (-1), function and
    # cause named, pointers, sizes and contents unchanged
    for args, word in (((q.ctypes.data, None, None, 0, 0, 0), 'n_postures 0'), ((q.ctypes.data, None, None, 33, 0, 0), 'n_postures 33'),
                       ((q.ctypes.data, None, None, K, 0, 2), 'unknown flag bits')):
        assert L.rr_posture_dynamics(env.h, *args) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_posture_dynamics' in msg and word in msg, msg
    p, x = C.c_void_p(), C.c_size_t()
    for which in (5, -1):
        assert L.rr_posture_dynamics_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_posture_dynamics_buffer' in L.rr_last_error().decode()
    scratch = np.zeros(4, np.float32)
    assert L.rr_posture_dynamics_copy_to_host(env.h, 0, scratch.ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    assert L.rr_posture_dynamics_copy_to_host(env.h, 0, None, sizes[0]) == -1
    assert 'rr_posture_dynamics_copy_to_host: null destination' in L.rr_last_error().decode()
    for bad in ((np.zeros((N, 0, 11), np.float32), None, None), (np.zeros((N, 33, 11), np.float32), None, None), (q[:, :, :9], None, None),
                (q.astype(np.float64), None, None), (q, qd[:, :2], None),
                (q, torch.from_numpy(qd).cuda(), None), (torch.from_numpy(q).cuda(), None, qdd)):      # mixed host / device sets
        with pytest.raises(ValueError):
            env.posture_dynamics(*bad)
    with pytest.raises(ValueError):
        env.posture_dynamics_buffer('jacobian')
    assert [env.posture_dynamics_buffer(w, host=True).tobytes() for w in range(5)] == [first[k].tobytes() for k in nat.PD_FIELDS]
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    # a row with a NaN joint: NaN in that row's outputs, its neighbours untouched, and the call returns 0
    bad = q.copy()
    bad[1, 1, 0] = np.nan
    assert L.rr_posture_dynamics(env.h, bad.ctypes.data, qd.ctypes.data, qdd.ctypes.data, K, 0, nat.PD_INVERSE) == 0
    got = {k: env.posture_dynamics_buffer(k, host=True) for k in nat.PD_FIELDS}
    others = np.ones((N, K), bool)
    others[1, 1] = False
    for k in nat.PD_FIELDS:
        assert (_bits(got[k][others]) == _bits(first[k][others])).all(), k
    for k in VECTORS:
        assert np.isnan(got[k][1, 1]).all(), k
    assert np.isnan(got['mass_matrix'][1, 1][np.arange(11), np.arange(11)]).all() and np.isnan(got['mass_inverse'][1, 1]).any()
    # ... and a non-finite velocity or acceleration stays in its row as well
    bad_v, bad_a = qd.copy(), qdd.copy()
    bad_v[2, 0, 3], bad_a[4, 2, 10] = np.inf, np.nan
    got = env.posture_dynamics(q, bad_v, bad_a, inverse=True, host=True)
    others[:] = True
    others[2, 0] = others[4, 2] = False
    for k in nat.PD_FIELDS:
        assert (_bits(got[k][others]) == _bits(first[k][others])).all(), k
    assert not np.isfinite(got['bias'][2, 0]).all() and not np.isfinite(got['torque'][4, 2]).all()
    assert (_bits(got['mass_matrix']) == _bits(first['mass_matrix'])).all() and (_bits(got['bias'][4, 2]) == _bits(first['bias'][4, 2])).all()
    # DLPack into torch without a copy; the pointers never change
    for w, name in enumerate(nat.PD_FIELDS):
        buf = env.posture_dynamics_buffer(name)
        t = torch.from_dlpack(buf)
        assert t.is_cuda and t.data_ptr() == buf.ptr == before[w][0] and tuple(t.shape) == got[name].shape, name
    env.close()


def test_use_urdf_inertia_answers_with_its_own_inertias():
    """The masses and inertias are the handle's own: a handle created with use_urdf_inertia differs in M where the rotational inertia
    counts, and not in the gravity torques, which no inertia enters."""
    N, K = 3, 1
    q, _, _ = nd.inputs(N, K)
    a, b = _env(N), _env(N, use_urdf_inertia=True)
    x, y = a.posture_dynamics(q, host=True), b.posture_dynamics(q, host=True)
    assert np.abs(x['mass_matrix'] - y['mass_matrix']).max() > 1e-4
    assert (_bits(x['gravity']) == _bits(y['gravity'])).all()
    a.close()
    b.close()


def test_vector_env_switch():
    import torch
    from real_robots_amd.vector import REALRobotVectorEnv
    kw = dict(objects=1, eye_width=64, eye_height=64)
    shapes = dict(mass_matrix=(11, 11), bias=(11,))
    plain = REALRobotVectorEnv(2, **kw)
    obs, _ = plain.reset(seed=0)
    assert not set(shapes) & set(obs) and not set(shapes) & set(plain.single_observation_space.spaces)
    plain.close()
    v = REALRobotVectorEnv(2, dynamics_obs=True, **kw)
    cmd = np.tile(np.array([0.3, 0.5, 0, -0.8, 0, 0.6, 0, 0.5, 0.2], np.float32), (2, 1))
    obs0, _ = v.reset(seed=0)
    obs1 = v.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    for obs in (obs0, obs1):
        for key, sh in shapes.items():
            sp = v.single_observation_space[key]
            assert sp.shape == sh and sp.dtype == np.float32 and v.observation_space[key].shape == (2,) + sh, key
            assert obs[key].shape == (2,) + sh and obs[key].dtype == np.float32 and v.observation_space[key].contains(obs[key]), key
    back = v._be.posture_dynamics(host=True)
    for key in shapes:
        assert (_bits(obs1[key]) == _bits(back[key][:, 0])).all() and obs1[key].any(), key
    v.close()
    d = REALRobotVectorEnv(2, dynamics_obs=True, device_obs=True, **kw)
    d.reset(seed=0)
    obs = d.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    for key, sh in shapes.items():
        t = torch.from_dlpack(obs[key])
        d._be.sync()
        assert t.is_cuda and tuple(t.shape) == (2,) + sh and (_bits(t.cpu().numpy()) == _bits(back[key][:, 0])).all(), key
    d.close()
