"""GPU tests (-m gpu) of the whole-batch kinematic observations (rr_kinematic_observations, include/realrobot.h): the seven device
buffers against the independent float64 restatement (tests/numpy_kinematics.py: complex-step Jacobians, not axis x lever), on
states set from outside and after real steps; that the call has no effect on the simulation; the points API; a resolved-rate loop
closed through the device's Jacobian; the vector env's switch and DLPack.

Tolerances: the project's own frame tolerance of 2e-6 on R, p and axes (tests/test_gpu_numpy_step.py) and the 5e-6 of
test_link_poses_match_fk_fixture: positions and quaternions 5e-6; angular Jacobian rows 2e-6 (they are the axes); linear rows 1e-5
(an axis error times a lever of at most 1.4 m, plus a lever error); velocities those two times the sum of |qd_k| over the joints
that move the link."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model
from tests import numpy_kinematics as nk

pytestmark = pytest.mark.gpu

U = np.uint32
NL = len(nat.LINK_NAMES)
TOL_POS, TOL_QUAT, TOL_JW, TOL_JV = 5e-6, 5e-6, 2e-6, 1e-5
# the eight points of the parity test: fixed to the world | mid-arm | the default point | the same link with an offset | finger_01
# (body 8) | skin_10 (body 9) | two more finger-side links
POINT_LINKS = [0, 4, 8, 8, nat.LINK_NAMES.index('finger_01'), nat.LINK_NAMES.index('skin_10'), 14, 11]
ZERO_COLS = {0: range(11), 1: range(4, 11), 2: range(7, 11), 3: range(7, 11), 4: (9, 10), 5: (7, 8, 10)}


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _point_offsets(rng):
    loc = rng.uniform(-0.2, 0.2, (8, 3)).astype(np.float32)
    loc[2] = 0.0
    return loc


def _random_state(env, rng):
    """The env's reset state with q uniform within the joint limits, qd in +-3 rad/s, object velocities +-1 m/s and +-5 rad/s."""
    env.reset()
    st = env.state
    lim = np.array(load_model()['body_limits'], np.float64)          # rows 8 and 10 are [0, -1.571]: min and max per row
    st[:, :11] = rng.uniform(lim.min(1), lim.max(1), (env.N, 11)).astype(np.float32)
    st[:, 11:22] = rng.uniform(-3, 3, (env.N, 11)).astype(np.float32)
    for o in range(3):
        st[:, 22 + 13 * o + 7:22 + 13 * o + 10] = rng.uniform(-1, 1, (env.N, 3)).astype(np.float32)
        st[:, 22 + 13 * o + 10:22 + 13 * o + 13] = rng.uniform(-5, 5, (env.N, 3)).astype(np.float32)
    return st


def _align(q, ref):
    return q * np.where((q * ref).sum(-1, keepdims=True) < 0, -1.0, 1.0)


def _check(env, obs, where, links=(8,), local=None):
    """The seven host arrays of one call against float64 from env.state; prints every figure before it asserts."""
    N, P = env.N, len(links)
    st = env.state
    ref = nk.observations(st, links, local)
    assert [obs[k].shape for k in nat.KIN_FIELDS] == [(N, 11), (N, NL, 7), (N, NL, 6), (N, env.n_objects, 6), (N, P, 3), (N, P, 6), (N, P, 6, 11)]
    assert all(obs[k].dtype == np.float32 for k in nat.KIN_FIELDS)
    # the floats of RR_F_STATE, bit for bit
    assert (_bits(obs['joint_vel']) == _bits(st[:, 11:22])).all(), where
    for o in range(env.n_objects):
        assert (_bits(obs['obj_vel'][:, o]) == _bits(st[:, 22 + 13 * o + 7:22 + 13 * o + 13])).all(), (where, o)
    qd_abs = np.abs(st[:, 11:22].astype(np.float64))
    s_link = qd_abs @ nk.ancestors(range(NL)).T                      # [N, 17] sum of |qd_k| over the joints that move the link
    s_pt = qd_abs @ nk.ancestors(links).T
    fig = dict(
        link_pos=np.abs(obs['link_pose'][..., :3] - ref['link_pos']).max(),
        link_quat=np.abs(_align(obs['link_pose'][..., 3:].astype(np.float64), ref['link_quat']) - ref['link_quat']).max(),
        point_pos=np.abs(obs['point_pos'] - ref['point_pos']).max(),
        jac_lin=np.abs(obs['jacobian'][:, :, :3] - ref['point_jac'][:, :, :3]).max(),
        jac_ang=np.abs(obs['jacobian'][:, :, 3:] - ref['point_jac'][:, :, 3:]).max(),
        link_v=(np.abs(obs['link_vel'][..., :3] - ref['link_vel'][..., :3]).max(-1) - TOL_JV * s_link).max(),
        link_w=(np.abs(obs['link_vel'][..., 3:] - ref['link_vel'][..., 3:]).max(-1) - TOL_JW * s_link).max(),
        point_v=(np.abs(obs['point_vel'][..., :3] - ref['point_vel'][..., :3]).max(-1) - TOL_JV * s_pt).max(),
        point_w=(np.abs(obs['point_vel'][..., 3:] - ref['point_vel'][..., 3:]).max(-1) - TOL_JW * s_pt).max(),
        link_v_abs=np.abs(obs['link_vel'][..., :3] - ref['link_vel'][..., :3]).max(),
        link_w_abs=np.abs(obs['link_vel'][..., 3:] - ref['link_vel'][..., 3:]).max())
    print(where, {k: float('%.3g' % v) for k, v in fig.items()})
    assert fig['link_pos'] < TOL_POS and fig['point_pos'] < TOL_POS and fig['link_quat'] < TOL_QUAT, (where, fig)
    assert fig['jac_lin'] < TOL_JV and fig['jac_ang'] < TOL_JW, (where, fig)
    assert fig['link_v'] <= 0 and fig['link_w'] <= 0 and fig['point_v'] <= 0 and fig['point_w'] <= 0, (where, fig)      # (error minus its tolerance)
    # structural zeros are +0.0 bit for bit: the joints that do not move a point's link, and everything of a link rigid with the world
    anc = nk.ancestors(links)
    for j in range(P):
        assert not _bits(obs['jacobian'][:, j][:, :, anc[j] == 0]).any(), (where, j)
        if not anc[j].any():
            assert not _bits(obs['point_vel'][:, j]).any(), (where, j)
    assert not _bits(obs['link_vel'][:, 0]).any(), where
    # both are float32 forms of one expression
    lp = env.link_poses()
    assert np.abs(obs['link_pose'][..., :3] - lp[..., :3]).max() < 1e-6, where
    assert np.abs(_align(obs['link_pose'][..., 3:], lp[..., 3:]) - lp[..., 3:]).max() < 1e-6, where
    return ref


@pytest.mark.parametrize('N,objects', [(3, 1), (131, 3)])
def test_against_float64_on_states_set_from_outside(N, objects):
    """N = 3: less than any workgroup of envs; N = 131: a ragged tail for 4, 16 or 64 envs per workgroup.  Eight points."""
    env = BatchedREALRobotEnv(N, objects=objects, width=64, height=64)
    rng = np.random.default_rng(10 + N)
    env.state = _random_state(env, rng)
    local = _point_offsets(rng)
    env.set_kinematic_points(POINT_LINKS, local)
    links, loc = env.kinematic_points()
    assert list(links) == POINT_LINKS and (_bits(loc) == _bits(local)).all()
    obs = env.kinematic_observations(host=True)
    _check(env, obs, 'outside N=%d' % N, POINT_LINKS, local)
    for j, cols in ZERO_COLS.items():
        assert not _bits(obs['jacobian'][:, j][:, :, list(cols)]).any(), j
        live = [k for k in range(11) if k not in cols]
        assert live == [] or np.abs(obs['jacobian'][:, j][:, 3:, live]).max() > 0.5, j          # ... and the other columns are axes
    env.close()


def test_after_real_steps_with_the_default_point():
    from real_robots_amd.distributed import synthetic_actions
    env = BatchedREALRobotEnv(67, objects=3, width=64, height=64)
    env.reset()
    for t in range(40):
        env.step(synthetic_actions(list(range(67)), t))
    obs = env.kinematic_observations(host=True)
    _check(env, obs, 'steps')
    assert np.abs(obs['joint_vel']).max() > 0.1 and np.abs(obs['link_vel'][:, 8]).max() > 0.01      # the arm is moving
    assert (_bits(obs['point_pos'][:, 0]) == _bits(obs['link_pose'][:, 8, :3])).all()
    env.close()


def test_no_effect_on_the_simulation():
    from real_robots_amd.distributed import synthetic_actions
    a = BatchedREALRobotEnv(8, objects=3, width=64, height=64)
    b = BatchedREALRobotEnv(8, objects=3, width=64, height=64)
    a.reset()
    b.reset()
    for t in range(60):
        cmd = synthetic_actions(list(range(8)), t)
        a.step(cmd)
        b.step(cmd)
        b.kinematic_observations()
        if t == 30:
            b.set_kinematic_points(['finger_01', 'base', 0], [[0, 0, 0.05], [0.1, 0, 0], [0, 0, 0]])
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    assert (a.host(nat.F_ERRFLAGS) == b.host(nat.F_ERRFLAGS)).all()
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    a.close()
    b.close()


def _buffers(env):
    out = []
    for w in range(7):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_kinematic_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_points_api():
    N = 5
    env = BatchedREALRobotEnv(N, objects=2, width=64, height=64)
    L = env.L
    # allocated by the first accessor, all zero before the first observation call
    for name in nat.KIN_FIELDS:
        assert not _bits(env.kinematic_buffer(name, host=True)).any(), name
    before = _buffers(env)
    assert [n for _, n in before] == [N * k * 4 for k in (11, 119, 102, 12, 3, 6, 66)]
    links, loc = env.kinematic_points()
    assert list(links) == [nat.EE_LINK] and loc.shape == (1, 3) and not loc.any()          # a fresh handle: the gripper base
    env.state = _random_state(env, np.random.default_rng(3))
    first = env.kinematic_observations(host=True)
    # refused calls: RR_EINVAL, the point named, nothing changes
    zeros9 = np.zeros((9, 3), np.float32)
    nan = np.zeros((2, 3), np.float32)
    nan[1, 2] = np.nan
    for n, lk, lc, word in ((9, [8] * 9, zeros9, 'point 8'), (2, [8, 17], zeros9, 'point 1'), (1, [-1], zeros9, 'point 0'), (2, [8, 8], nan, 'point 1')):
        lk = np.array(lk, np.int32)
        assert L.rr_set_kinematic_points(env.h, n, lk.ctypes.data, lc.ctypes.data) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_set_kinematic_points' in msg and word in msg, msg
    links, loc = env.kinematic_points()
    assert list(links) == [nat.EE_LINK] and not loc.any()
    again = env.kinematic_observations(host=True)
    for name in nat.KIN_FIELDS:
        assert (_bits(first[name]) == _bits(again[name])).all(), name
    assert _buffers(env) == before
    p, n = C.c_void_p(), C.c_size_t()
    for which in (7, -1):
        assert L.rr_kinematic_buffer(env.h, which, C.byref(p), C.byref(n)) == -1
        assert 'rr_kinematic_buffer' in L.rr_last_error().decode()
    # a change of P: the same pointers, the sizes of the three point buffers follow P; NULL offsets are zeros
    lk = np.array([8, 3, 0], np.int32)
    nat.check(L.rr_set_kinematic_points(env.h, 3, lk.ctypes.data, None))
    after = _buffers(env)
    assert [p for p, _ in after] == [p for p, _ in before]
    assert [n for _, n in after] == [N * k * 4 for k in (11, 119, 102, 12, 9, 18, 198)]
    links, loc = env.kinematic_points()
    assert list(links) == [8, 3, 0] and loc.shape == (3, 3) and not loc.any()
    obs = env.kinematic_observations(host=True)
    _check(env, obs, 'three points', [8, 3, 0], None)
    assert (_bits(obs['jacobian'][:, 0]) == _bits(first['jacobian'][:, 0])).all()
    # the points survive reset, set_state and restore
    ck = env.checkpoint()
    env.reset()
    env.restore(ck)
    assert list(env.kinematic_points()[0]) == [8, 3, 0]
    rest = env.kinematic_observations(host=True)
    assert (_bits(rest['jacobian']) == _bits(obs['jacobian'])).all()
    with pytest.raises(ValueError):
        env.set_kinematic_points(['base'] * 9)
    env.close()


def test_the_jacobian_closes_a_loop():
    """Resolved rate through the device's own tensors: point_pos, link_pose[:, 8] and jacobian[:, 0, :, :7] drive the damped
    least-squares step of oracle.kinematics._dls (damping 0.1, clamp 0.5, wrap) in float64 on the host; q goes back through
    env.state.  Every env is below 1e-3 within 40 iterations (the float64 loop with the oracle's own Jacobian needs 14, 16, 15)."""
    from oracle import kinematics as ok
    targets = np.array([[-0.1, 0.1, 0.5], [0.05, -0.3, 0.45], [-0.2, 0.4, 0.6], [-0.2, 0.4, 0.6]])
    quat = np.asarray(ok.quat_from_euler(0, 3.14, -1.57), dtype=np.float64)
    Rt = ok.quat_to_mat(quat / np.linalg.norm(quat))
    env = BatchedREALRobotEnv(4, objects=1, width=64, height=64)
    env.reset()
    st = env.state
    assert not st[:, :22].any()          # the rest pose
    done_at = [None] * 4
    for it in range(40):
        obs = env.kinematic_observations(host=True)
        q = st[:, :11].astype(np.float64)
        for i in range(4):
            if done_at[i] is not None:
                continue
            if ok.ee_residual(q[i], targets[i], quat) < 1e-3:
                done_at[i] = it
                continue
            Re = ok.quat_to_mat(obs['link_pose'][i, 8, 3:].astype(np.float64))
            e = ok.pose_residual(Re, obs['point_pos'][i, 0].astype(np.float64), targets[i], Rt)
            J = obs['jacobian'][i, 0, :, :7].astype(np.float64)
            dq = J.T @ np.linalg.solve(J @ J.T + 0.01 * np.eye(6), e)
            n = np.abs(dq).max()
            if n > 0.5:
                dq *= 0.5 / n
            q[i, :7] = (q[i, :7] + dq + np.pi) % (2 * np.pi) - np.pi
        st[:, :11] = q.astype(np.float32)
        env.state = st
    res = [ok.ee_residual(st[i, :11].astype(np.float64), targets[i], quat) for i in range(4)]
    print('iterations', done_at, 'residuals', res)
    assert all(r < 1e-3 for r in res), (done_at, res)
    env.close()


def test_vector_env_switch_and_dlpack():
    import torch
    from real_robots_amd.envs.robot import Kuka
    from real_robots_amd.vector import REALRobotVectorEnv
    kw = dict(objects=1, eye_width=64, eye_height=64)
    shapes = dict(joint_velocities=(11,), link_poses=(17, 7), link_velocities=(17, 6), object_velocities=(1, 6), point_positions=(1, 3),
                  point_velocities=(1, 6), jacobian=(1, 6, 11))
    base = Kuka(False, 1, 64, 64, env=None).observation_space
    plain = REALRobotVectorEnv(2, **kw)
    obs, _ = plain.reset(seed=0)
    assert not set(shapes) & set(obs) and set(plain.single_observation_space.spaces) == set(base.spaces) == set(plain.observation_space.spaces)
    plain.close()
    v = REALRobotVectorEnv(2, kinematic_obs=True, **kw)
    assert set(v.single_observation_space.spaces) == set(base.spaces) | set(shapes)
    cmd = np.tile(np.array([0.3, 0.5, 0, -0.8, 0, 0.6, 0, 0.5, 0.2], np.float32), (2, 1))
    obs0, _ = v.reset(seed=0)
    obs1 = v.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    for obs in (obs0, obs1):
        for key, sh in shapes.items():
            sp = v.single_observation_space[key]
            assert sp.shape == sh and sp.dtype == np.float32 and v.observation_space[key].shape == (2,) + sh, key
            assert obs[key].shape == (2,) + sh and obs[key].dtype == np.float32 and v.observation_space[key].contains(obs[key]), key
    assert not obs0['joint_velocities'].any() and obs1['joint_velocities'].any()
    back = v._be.kinematic_observations(host=True)
    for key, name in v.KINEMATIC_KEYS:
        assert (_bits(obs1[key]) == _bits(back[name])).all(), key
    v.close()
    d = REALRobotVectorEnv(2, kinematic_obs=True, device_obs=True, kinematic_points=(['base', 'finger_01'], [[0, 0, 0.1], [0, 0, 0]]), **kw)
    assert d.single_observation_space['jacobian'].shape == (2, 6, 11)
    d.reset(seed=0)
    obs = d.step({"joint_command": cmd, "render": np.zeros(2, np.int8)})[0]
    assert obs['jacobian'].shape == (2, 2, 6, 11) and obs['jacobian'].typestr == np.dtype(np.float32).str
    t = torch.from_dlpack(obs['jacobian'])
    d._be.sync()
    host = d._be.kinematic_buffer('jacobian', host=True)
    assert t.is_cuda and tuple(t.shape) == (2, 2, 6, 11) and (t.cpu().numpy().view(U) == _bits(host)).all() and host.any()
    d.close()
