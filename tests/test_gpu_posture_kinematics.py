"""GPU tests (-m gpu) of the kinematics at candidate postures (rr_posture_kinematics, include/realrobot.h): link poses, point positions
and point Jacobians at K candidate joint postures per env against the independent float64 restatement of the kinematic observations
(tests/numpy_kinematics.py: complex-step Jacobians, not axis x lever) on a [N K, 61] state whose first eleven columns are the
candidates; bit-identity with rr_kinematic_observations where the candidate is the present posture; that a row depends on its posture
alone; that the call has no effect on the simulation; the buffers and the refusals.

Tolerances: those of tests/test_gpu_kinematic_obs.py for the same arithmetic -- positions and quaternions 5e-6 (quaternions after sign
alignment), angular Jacobian rows 2e-6, linear rows 1e-5.  Candidates are uniform within the joint limits, as that file's
_random_state draws its joints.

One RR_EINVAL of the header is not provoked here: a model without the 17 URDF links needs another compiled model; the condition is
rr_kinematic_observations' own."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model
from tests import numpy_kinematics as nk
from tests.test_gpu_kinematic_obs import POINT_LINKS, TOL_JV, TOL_JW, TOL_POS, TOL_QUAT, _align, _point_offsets, _random_state

pytestmark = pytest.mark.gpu

U = np.uint32
NL = len(nat.LINK_NAMES)
ARM = 7          # joints 0..6: the arm


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _env(N, objects=3):
    return BatchedREALRobotEnv(N, objects=objects, width=64, height=64)


def _candidates(rng, q_now, K):
    """float32 [N, K, 11] uniform within the joint limits; every candidate differs from its env's present joints by >= 0.1 rad in at
    least one arm joint (a draw that does not is drawn again: 7 joints within +-0.1 rad of 2.9 .. 5.9 rad ranges)."""
    lim = np.array(load_model()['body_limits'], np.float64)          # rows 8 and 10 are [0, -1.571]: min and max per row
    N = len(q_now)
    po = rng.uniform(lim.min(1), lim.max(1), (N, K, 11)).astype(np.float32)
    for _ in range(8):
        near = (np.abs(po[:, :, :ARM] - q_now[:, None, :ARM]) < 0.1).all(-1)
        if not near.any():
            break
        po[near] = rng.uniform(lim.min(1), lim.max(1), (int(near.sum()), 11)).astype(np.float32)
    return po


def _reference(po, links, local):
    """float64 fields of the N K candidates as [N, K, ...]: the observations of a state whose joints are the candidate."""
    N, K = po.shape[:2]
    st = np.zeros((N * K, 61))
    st[:, :11] = po.reshape(N * K, 11)
    ref = nk.observations(st, links, local)
    return {k: ref[k].reshape((N, K) + ref[k].shape[1:]) for k in ('link_pos', 'link_quat', 'point_pos', 'point_jac')}


def _figures(out, ref):
    return dict(
        link_pos=np.abs(out['link_pose'][..., :3] - ref['link_pos']).max(),
        link_quat=np.abs(_align(out['link_pose'][..., 3:].astype(np.float64), ref['link_quat']) - ref['link_quat']).max(),
        point_pos=np.abs(out['point_pos'] - ref['point_pos']).max(),
        jac_lin=np.abs(out['jacobian'][..., :3, :] - ref['point_jac'][..., :3, :]).max(),
        jac_ang=np.abs(out['jacobian'][..., 3:, :] - ref['point_jac'][..., 3:, :]).max())


def _same(a, b):
    return all((_bits(a[k]) == _bits(b[k])).all() for k in nat.PK_FIELDS)


@pytest.mark.parametrize('N,K,P', [(3, 1, 1), (5, 3, 8), (131, 32, 8)])
def test_against_float64(N, K, P):
    """(3, 1, 1): fewer rows than a workgroup, and P = 1, whose 3-float rows are the awkward alignment; (5, 3, 8) and (131, 32, 8): a
    ragged tail for any rows-per-workgroup up to 64 (15 and 4192 = 65 x 64 + 32 rows).  The env has a random present state that no
    candidate is near: a kernel that read the state instead of the tensor fails."""
    import torch
    env = _env(N)
    rng = np.random.default_rng(100 + N)
    env.state = _random_state(env, rng)
    st = env.state
    if P == 1:
        links, local = [nat.EE_LINK], None          # the point of a fresh handle
    else:
        links, local = POINT_LINKS, _point_offsets(rng)
        env.set_kinematic_points(links, local)
    po = _candidates(rng, st[:, :11], K)
    assert (np.abs(po[:, :, :ARM] - st[:, None, :ARM]).max(-1) >= 0.1).all()
    out = env.posture_kinematics(po, host=True)
    assert [out[k].shape for k in nat.PK_FIELDS] == [(N, K, NL, 7), (N, K, P, 3), (N, K, P, 6, 11)]
    assert all(out[k].dtype == np.float32 for k in nat.PK_FIELDS)
    ref = _reference(po, links, local)
    fig = _figures(out, ref)
    print((N, K, P), {k: float('%.3g' % v) for k, v in fig.items()})
    assert fig['link_pos'] < TOL_POS and fig['point_pos'] < TOL_POS and fig['link_quat'] < TOL_QUAT, fig
    assert fig['jac_lin'] < TOL_JV and fig['jac_ang'] < TOL_JW, fig
    # structural zeros are +0.0 bit for bit: the joints that do not move a point's link
    anc = nk.ancestors(links)
    for j in range(P):
        assert not _bits(out['jacobian'][:, :, j][..., anc[j] == 0]).any(), j
        live = np.flatnonzero(anc[j])
        assert live.size == 0 or np.abs(out['jacobian'][:, :, j][:, :, 3:][..., live]).max() > 0.5, j      # ... and the other columns are axes
    # a CUDA torch tensor read in place: the bits of the staged host array
    t = torch.from_numpy(po).cuda()
    torch.cuda.synchronize()
    view = env.posture_kinematics(t)
    dev = {k: torch.from_dlpack(v) for k, v in view.items()}
    env.sync()
    for k in nat.PK_FIELDS:
        assert dev[k].is_cuda and tuple(dev[k].shape) == out[k].shape and (_bits(dev[k].cpu().numpy()) == _bits(out[k])).all(), k
    # the env's present state is where it was
    assert env.state.tobytes() == st.tobytes()
    env.close()


def _present_rows(env, K):
    """posture_kinematics at K copies of every env's present joints against kinematic_observations(), bit for bit, for every k."""
    obs = env.kinematic_observations(host=True)
    po = np.ascontiguousarray(np.repeat(env.state[:, None, :11], K, axis=1))
    out = env.posture_kinematics(po, host=True)
    for k in range(K):
        for name in nat.PK_FIELDS:
            assert (_bits(out[name][:, k]) == _bits(obs[name])).all(), (name, k)
    return obs, out


def test_bit_identity_with_the_present_state_query():
    from real_robots_amd.distributed import synthetic_actions
    env = _env(67)
    env.reset()
    for t in range(40):
        env.step(synthetic_actions(list(range(67)), t))
    obs, out = _present_rows(env, 3)
    assert np.abs(obs['joint_vel']).max() > 0.1 and np.abs(obs['jacobian']).max() > 0.5           # the arm has moved, the default point has a Jacobian
    assert (_bits(out['point_pos'][:, :, 0]) == _bits(out['link_pose'][:, :, nat.EE_LINK, :3])).all()
    # a state set from outside, eight points, K = 32: more rows than a workgroup, a ragged tail
    rng = np.random.default_rng(7)
    env.state = _random_state(env, rng)
    env.set_kinematic_points(POINT_LINKS, _point_offsets(rng))
    _present_rows(env, 32)
    env.close()


def test_row_independence_and_determinism():
    N, K = 6, 5
    env = _env(N)
    rng = np.random.default_rng(31)
    st = _random_state(env, rng)
    env.state = st
    env.set_kinematic_points(POINT_LINKS, _point_offsets(rng))
    po = _candidates(rng, st[:, :11], K)
    first = env.posture_kinematics(po, host=True)
    assert _same(first, env.posture_kinematics(po, host=True))                                       # a second call
    # the candidates permuted across (e, k): the rows are permuted
    perm = rng.permutation(N * K)
    shuffled = env.posture_kinematics(np.ascontiguousarray(po.reshape(N * K, 11)[perm].reshape(N, K, 11)), host=True)
    for name in nat.PK_FIELDS:
        rows = first[name].reshape((N * K,) + first[name].shape[2:])
        assert (_bits(shuffled[name].reshape(rows.shape)) == _bits(rows[perm])).all(), name
    # another K: posture k alone
    alone = env.posture_kinematics(np.ascontiguousarray(po[:, 2:3]), host=True)
    for name in nat.PK_FIELDS:
        assert (_bits(alone[name][:, 0]) == _bits(first[name][:, 2])).all(), name
    # another state of the env (joints, velocities, objects): nothing changes
    st2 = _random_state(env, rng)
    st2[:, 22:25] += 0.05
    env.state = st2
    assert np.abs(st2[:, :11] - st[:, :11]).max() > 0.5
    assert _same(first, env.posture_kinematics(po, host=True))
    # non-finite and out-of-limit rows finish, and every other row keeps its bits
    bad = po.copy()
    bad[0, 1, 3] = np.nan
    bad[2, 0, :] = np.inf
    bad[3, 4, 0] = -np.inf
    bad[4, 2, :] = np.pi
    bad[5, 3, :] = -np.pi
    got = env.posture_kinematics(bad, host=True)
    env.sync()
    others = np.ones((N, K), bool)
    for e, k in ((0, 1), (2, 0), (3, 4), (4, 2), (5, 3)):
        others[e, k] = False
    for name in nat.PK_FIELDS:
        assert (_bits(got[name][others]) == _bits(first[name][others])).all(), name
    for e, k in ((4, 2), (5, 3)):                                                                    # not clamped: evaluated as given
        assert all(np.isfinite(got[name][e, k]).all() for name in nat.PK_FIELDS)
    pi_ref = _reference(np.ascontiguousarray(bad[4:6, 2:4]), POINT_LINKS, env.kinematic_points()[1])
    fig = _figures({name: got[name][4:6, 2:4] for name in nat.PK_FIELDS}, pi_ref)
    assert fig['link_pos'] < TOL_POS and fig['point_pos'] < TOL_POS and fig['jac_lin'] < TOL_JV and fig['jac_ang'] < TOL_JW, fig
    env.close()


def test_no_effect_on_the_simulation():
    """60 steps with a query after each leave contact counts at every step, and error flags, state, preparation record and checkpoint
    at the end, bit-identical to a twin that never asked; the RR_KIN_*, RR_PC_* and RR_SD_* buffers written before a query are
    unchanged behind it."""
    import torch
    from real_robots_amd.distributed import synthetic_actions
    from tests import numpy_posture as npo
    N = 8
    a, b = _env(N), _env(N)
    rng = np.random.default_rng(5)
    pairs = npo.robot_pairs()
    for env in (a, b):
        env.reset()
        env.set_distance_pairs(pairs, 0.25)
    po = _candidates(rng, np.zeros((N, 11), np.float32), 3)
    dev = torch.from_numpy(po).cuda()
    torch.cuda.synchronize()
    for t in range(60):
        cmd = synthetic_actions(list(range(N)), t)
        a.step(cmd)
        b.step(cmd)
        if t % 20 == 7:
            b.kinematic_observations()
            b.posture_clearance(po)
            b.signed_distance(po)
            before = ([b.kinematic_buffer(w, host=True).tobytes() for w in range(len(nat.KIN_FIELDS))],
                      [b.posture_buffer(w, host=True).tobytes() for w in range(len(nat.PC_FIELDS))],
                      [b.signed_buffer(w, host=True).tobytes() for w in range(len(nat.SD_FIELDS))])
        b.posture_kinematics(dev if t % 2 else po)
        if t == 30:
            b.set_kinematic_points(['finger_01', 'base', 0], [[0, 0, 0.05], [0.1, 0, 0], [0, 0, 0]])
        if t % 20 == 7:
            after = ([b.kinematic_buffer(w, host=True).tobytes() for w in range(len(nat.KIN_FIELDS))],
                     [b.posture_buffer(w, host=True).tobytes() for w in range(len(nat.PC_FIELDS))],
                     [b.signed_buffer(w, host=True).tobytes() for w in range(len(nat.SD_FIELDS))])
            assert before == after, t
        assert (a.host(nat.F_CONTACT_COUNT) == b.host(nat.F_CONTACT_COUNT)).all(), t
    for f in (nat.F_ERRFLAGS, nat.F_STATE, nat.F_PREP, nat.F_TOUCH):
        assert a.host(f).tobytes() == b.host(f).tobytes(), f
    ca, cb = a.checkpoint(), b.checkpoint()
    assert ca.shape == cb.shape and (ca == cb).all()
    assert b.posture_kinematics_buffer('jacobian', host=True).shape == (N, 3, 3, 6, 11)
    assert np.abs(b.posture_kinematics_buffer('jacobian', host=True)).max() > 0.5
    a.close()
    b.close()


def _buffers(env):
    out = []
    for w in range(len(nat.PK_FIELDS)):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_posture_kinematics_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


def test_buffers_and_errors():
    import torch
    N = 5
    env = _env(N, objects=2)
    L = env.L
    before = _buffers(env)
    assert [n for _, n in before] == [0, 0, 0] and all(p for p, _ in before) and len({p for p, _ in before}) == 3      # K counts as 0
    for w, name in enumerate(nat.PK_FIELDS):
        assert env.posture_kinematics_buffer(name, host=True).shape[:2] == (N, 0) and env.posture_kinematics_buffer(w).shape[:2] == (N, 0)
    env.sync()
    for (p, _), row in zip(before, (NL * 7, 8 * 3, 8 * 66)):                                         # zero-filled over the whole allocation
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (N * 32 * row,), '<i4', env)).any().item()
    rng = np.random.default_rng(17)
    env.state = _random_state(env, rng)
    st = env.state
    good = _candidates(rng, st[:, :11], 2)
    env.posture_kinematics(good)
    first = [env.posture_kinematics_buffer(w, host=True).tobytes() for w in range(3)]
    sizes = [N * 2 * NL * 7 * 4, N * 2 * 1 * 3 * 4, N * 2 * 1 * 66 * 4]
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    # refused calls: RR_EINVAL (-1), function and cause named, pointers, sizes and contents unchanged
    for args, word in (((None, 2, 0), 'null postures'), ((good.ctypes.data, 0, 0), 'n_postures 0'), ((good.ctypes.data, 33, 0), 'n_postures 33'),
                       ((good.ctypes.data, -1, 1), 'n_postures -1')):
        assert L.rr_posture_kinematics(env.h, *args) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_posture_kinematics' in msg and word in msg, msg
    p, x = C.c_void_p(), C.c_size_t()
    for which in (3, -1):
        assert L.rr_posture_kinematics_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_posture_kinematics_buffer' in L.rr_last_error().decode()
    scratch = np.zeros(4, np.float32)
    assert L.rr_posture_kinematics_copy_to_host(env.h, 0, scratch.ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    assert L.rr_posture_kinematics_copy_to_host(env.h, 0, None, sizes[0]) == -1 and 'rr_posture_kinematics_copy_to_host' in L.rr_last_error().decode()
    assert L.rr_posture_kinematics_copy_to_host(env.h, 3, scratch.ctypes.data, 16) == -1
    for bad in (good[:, :, :9], good.astype(np.float64), np.zeros((N, 33, 11), np.float32), good[:4], np.zeros((N, 0, 11), np.float32), None):
        with pytest.raises(ValueError):
            env.posture_kinematics(bad)
    with pytest.raises(ValueError):
        env.posture_kinematics_buffer('point_vel')
    assert [env.posture_kinematics_buffer(w, host=True).tobytes() for w in range(3)] == first
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    assert env.state.tobytes() == st.tobytes()
    # another K, then another P: the same pointers, the sizes follow
    k5 = _candidates(rng, st[:, :11], 5)
    out = env.posture_kinematics(k5, host=True)
    assert out['jacobian'].shape == (N, 5, 1, 6, 11)
    assert _buffers(env) == list(zip([p for p, _ in before], [N * 5 * NL * 7 * 4, N * 5 * 3 * 4, N * 5 * 66 * 4]))
    env.set_kinematic_points([8, 3, 0])
    assert _buffers(env) == list(zip([p for p, _ in before], [N * 5 * NL * 7 * 4, N * 5 * 3 * 3 * 4, N * 5 * 3 * 66 * 4]))
    out3 = env.posture_kinematics(k5, host=True)
    assert out3['point_pos'].shape == (N, 5, 3, 3) and out3['jacobian'].shape == (N, 5, 3, 6, 11)
    assert (_bits(out3['jacobian'][:, :, 0]) == _bits(out['jacobian'][:, :, 0])).all() and (_bits(out3['link_pose']) == _bits(out['link_pose'])).all()
    assert [p for p, _ in _buffers(env)] == [p for p, _ in before]
    # DLPack into torch without a copy
    for w, name in enumerate(nat.PK_FIELDS):
        buf = env.posture_kinematics_buffer(name)
        t = torch.from_dlpack(buf)
        assert t.is_cuda and t.data_ptr() == buf.ptr == before[w][0] and tuple(t.shape) == out3[name].shape, name
        env.sync()
        assert (_bits(t.cpu().numpy()) == _bits(out3[name])).all(), name
    env.close()
