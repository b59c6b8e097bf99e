"""CPU tests (-m "not gpu") of the whole-batch kinematic observations: the C boundary (header, binding, constants), the host-side
argument checks of `set_kinematic_points`, and the independent float64 restatement (tests/numpy_kinematics.py) against the
references that exist without a GPU (oracle/kinematics.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import kinematics as ok
from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model
from tests import numpy_kinematics as nk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_set_kinematic_points', 'rr_get_kinematic_points', 'rr_kinematic_observations', 'rr_kinematic_buffer', 'rr_kinematic_copy_to_host')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_enum_and_keeps_abi_7():
    h = _header()
    kin = dict((k, int(v)) for k, v in re.findall(r'\b(RR_KIN_[A-Z_]+)\s*=\s*(\d+)', h))
    assert kin == dict(RR_KIN_JOINT_VEL=0, RR_KIN_LINK_POSE=1, RR_KIN_LINK_VEL=2, RR_KIN_OBJ_VEL=3, RR_KIN_POINT_POS=4,
                       RR_KIN_POINT_VEL=5, RR_KIN_JACOBIAN=6, RR_KIN_COUNT=7)
    assert int(re.search(r'#define\s+RR_KIN_MAX_POINTS\s+(\d+)', h).group(1)) == nat.KIN_MAX_POINTS == 8
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(\s*rr_env\s*\*\s*env\b' % name, h), name
    doc = h[h.index('Kinematic observations on the device'):h.index('int rr_kinematic_copy_to_host(')]
    for word in ('getJointState', 'getLinkState', 'getBaseVelocity', 'calculateJacobian', 'robot.py:188-201', 'STREAM CONTRACT', 'Out of scope'):
        assert word in doc, word


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert nat.KIN_FIELDS == ('joint_vel', 'link_pose', 'link_vel', 'obj_vel', 'point_pos', 'point_vel', 'jacobian')
    assert nat.EE_LINK == 8 == ok.EE_LINK and nat.LINK_NAMES[nat.EE_LINK] == 'base' and len(nat.LINK_NAMES) == nk.NL == 17


def test_q_from_cmd_is_the_coupling_of_apply_action():
    """dq = Q_FROM_CMD @ dcmd reproduces the state a command is turned into: st[7] = st[9] = cmd[7], st[8] = st[10] = -cmd[8]."""
    Q = nat.Q_FROM_CMD
    assert Q.shape == (11, 9) and Q.dtype == np.float32
    cmd = np.random.default_rng(0).uniform(-1, 1, (5, 9)).astype(np.float32)
    st = np.zeros((5, 11), np.float32)
    st[:, :7] = cmd[:, :7]
    st[:, 7] = st[:, 9] = cmd[:, 7]
    st[:, 8] = st[:, 10] = -cmd[:, 8]
    assert (cmd @ Q.T == st).all()


def test_point_arguments_are_checked_on_the_host():
    """Every argument error is a ValueError raised before the native call: the check is a static method (no handle, no GPU)."""
    arg = BatchedREALRobotEnv._kinematic_points_arg
    idx, loc = arg(['base', 'finger_01', 4], [[0, 0, 0.1], [0.01, 0, 0], [0, 0, 0]])
    assert idx.dtype == np.int32 and list(idx) == [8, nat.LINK_NAMES.index('finger_01'), 4]
    assert loc.dtype == np.float32 and loc.shape == (3, 3) and loc[0, 2] == np.float32(0.1)
    idx, loc = arg('base')
    assert list(idx) == [8] and loc.shape == (1, 3) and not loc.any()
    for bad in (dict(links=['no_such_link']), dict(links=[17]), dict(links=[-1]), dict(links=[]), dict(links=list(range(9))),
                dict(links=[1.5]), dict(links=[8], local_pos=[0, 0, 0]), dict(links=[8, 9], local_pos=[[0, 0, 0]]),
                dict(links=[8], local_pos=[[0, np.nan, 0]]), dict(links=[8], local_pos=[[0, np.inf, 0]]), dict(links=[8], local_pos=[[0, 1e39, 0]])):
        with pytest.raises(ValueError):
            arg(**bad)


def _random_q(rng, n):
    lim = np.array(load_model()['body_limits'], np.float64)          # rows 8 and 10 are [0, -1.571]: min and max per row
    return rng.uniform(lim.min(1), lim.max(1), (n, 11))


def test_helper_jacobian_of_the_default_point_is_the_oracles():
    """20 random q within the limits: the complex-step Jacobian of link 8 at zero offset equals oracle.kinematics.ee_jacobian (axis x
    lever, float64) in columns 0..6 to 1e-12 and is zero in 7..10; position and rotation are the oracle's too."""
    q = _random_q(np.random.default_rng(1), 20)
    st = np.zeros((20, 61))
    st[:, :11] = q
    o = nk.observations(st)
    for i in range(20):
        J, Re, pe = ok.ee_jacobian(q[i])
        assert np.abs(o['point_jac'][i, 0, :, :7] - J).max() < 1e-12
        assert not o['point_jac'][i, 0, :, 7:].any()
        assert np.abs(o['point_pos'][i, 0] - pe).max() < 1e-12
        qt = o['link_quat'][i, 8]
        assert np.abs(ok.quat_to_mat(qt) - Re).max() < 1e-12 and abs(np.linalg.norm(qt) - 1) < 1e-12
    assert (o['point_jac'] == o['link_jac'][:, 8:9]).all() and (o['point_pos'] == o['link_pos'][:, 8:9]).all()


def test_helper_link_positions_and_velocities():
    """Link positions equal oracle.kinematics.link_pose; velocities are J @ qd; a link rigid with the world has zero rows; an offset
    point moves with its link: v = v_link + w x (R local)."""
    rng = np.random.default_rng(2)
    st = np.zeros((6, 61))
    st[:, :11], st[:, 11:22] = _random_q(rng, 6), rng.uniform(-3, 3, (6, 11))
    links, local = [0, 10, 16], rng.uniform(-0.2, 0.2, (3, 3))
    o = nk.observations(st, links, local)
    for i in range(6):
        for l in range(17):
            R, p = ok.link_pose(st[i, :11], l)
            assert np.abs(o['link_pos'][i, l] - p).max() < 1e-12
            # (the model's link_rot is float32 data: orthonormal to 6e-8 only, and a quaternion stands for a rotation nearby)
            assert np.abs(ok.quat_to_mat(o['link_quat'][i, l]) - R).max() < 1e-7 and abs(np.linalg.norm(o['link_quat'][i, l]) - 1) < 1e-7
        for j, l in enumerate(links):
            R, p = ok.link_pose(st[i, :11], l)
            assert np.abs(o['point_pos'][i, j] - (p + R @ local[j])).max() < 1e-12
            v = o['link_vel'][i, l, :3] + np.cross(o['link_vel'][i, l, 3:], R @ local[j])
            # (the rigid-body identity holds as far as the float32 model data are rotations and unit axes: 6e-8 x |w| <= 33 rad/s x 0.35 m)
            assert np.abs(o['point_vel'][i, j, :3] - v).max() < 1e-6 and np.abs(o['point_vel'][i, j, 3:] - o['link_vel'][i, l, 3:]).max() < 1e-12
    assert not o['link_jac'][:, 0].any() and not o['link_vel'][:, 0].any() and not o['point_vel'][:, 0].any()
    anc = nk.ancestors(range(17))
    assert not (o['link_jac'] * (1 - anc)[None, :, None, :]).any()          # structural zeros: the joints that do not move the link
    assert list(np.nonzero(nk.ancestors([10])[0])[0]) == list(range(9)) and list(np.nonzero(nk.ancestors([16])[0])[0]) == [0, 1, 2, 3, 4, 5, 6, 9]
