"""Tests of the C boundary of the step's joint torque inputs (rr_set_joint_torques, include/realrobot.h) that need no GPU: the header,
the binding, the refusals that need no handle, the Python-side argument checks and the vector env's spaces.  The GPU side is
tests/test_gpu_joint_torques.py, the reference's own tests tests/test_numpy_torque.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.vector import REALRobotVectorEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_set_joint_torques', 'rr_get_joint_torques', 'rr_joint_torque_buffer')


def test_header_declares_the_entry_points_and_keeps_abi_7():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert re.search(r'\bint\s+rr_set_joint_torques\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*torques\s*(/\*.*?\*/)?\s*,\s*int32_t\s+torques_on_device\s*,'
                     r'\s*const\s+uint8_t\s*\*\s*env_mask\s*(/\*.*?\*/)?\s*,\s*int32_t\s+mask_on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_get_joint_torques\s*\(\s*rr_env\s*\*\s*env\s*,\s*float\s*\*\s*out_host\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_joint_torque_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    doc = h[h.index('Joint torque inputs of the step'):h.index('int rr_joint_torque_buffer(')]
    for word in ('TORQUE_CONTROL', 'INDEPENDENT', "qd*' = qd* + dt M^-1 tau", 'RR_F_PREP', 'max_force = 0', 'feed-forward', 'RR_PD_BIAS',
                 'NOT compensated', 'NOT clamped', 'PERSISTENT', 'unlike pybullet', 'nothing clears the table', 'rr_reset', 'auto-reset',
                 'rr_write_state', 'rr_copy_envs', 'rr_checkpoint_restore', 'zero-row rule', 'either sign', 'NOT TOUCHED', 'bit for bit',
                 'frozen env', 'torques == NULL', 'turns the feature OFF', 'IN PLACE', 'STREAM CONTRACT', 'NOT validated', 'finiteness',
                 'changes NOTHING', 'mixed pair', 'look-ahead stays valid', 'NINE entries', 'RR_EINVAL', 'all or nothing', 'Out of scope'):
        assert word in doc, word
    # the dynamics query no longer calls torque control out of scope
    assert 'Out of scope: torque control in the step' not in h


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_set_joint_torques.argtypes) == 5 and len(L.rr_get_joint_torques.argtypes) == 2 and len(L.rr_joint_torque_buffer.argtypes) == 3
    # the refusals that need no device: a null env -- RR_EINVAL with the entry point's name
    assert L.rr_set_joint_torques(None, None, 0, None, 0) == -1 and 'rr_set_joint_torques: null env' in L.rr_last_error().decode()
    assert L.rr_get_joint_torques(None, None) == -1 and 'rr_get_joint_torques: null env' in L.rr_last_error().decode()
    assert L.rr_joint_torque_buffer(None, None, None) == -1 and 'rr_joint_torque_buffer: null env' in L.rr_last_error().decode()
    # the order of the refusals that need a handle, on the source: the mixed pair and the finiteness check come in front of the first
    # allocation, copy or launch, and of the flag -- a refusal changes nothing
    src = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_host.inc')).read()
    body = src[src.index('int rr_set_joint_torques('):src.index('int rr_joint_torque_buffer(')]
    first_effect = min(body.index(w) for w in ('ensure_torques(', 'hipMemcpyAsync', 'hipLaunchKernelGGL', 'e->jt_on ='))
    assert body.index('null env') < body.index('same side') < body.index('is not finite') < first_effect
    assert 'la_valid' not in body.replace('la_valid are not touched', '')       # the call never touches la_valid
    for name in ('set_joint_torques', 'joint_torques'):
        assert callable(getattr(BatchedREALRobotEnv, name))
    assert isinstance(BatchedREALRobotEnv.joint_torque_buffer, property)
    assert list(inspect.signature(BatchedREALRobotEnv.set_joint_torques).parameters)[1:] == ['torques', 'env_mask']
    p = inspect.signature(REALRobotVectorEnv.__init__).parameters['joint_torque_actions']
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_the_step_launches_the_kernel_only_while_torques_are_set():
    """On the source: one host branch in rr_step, behind the look-ahead's fallback and bind_frames, in front of the plan."""
    src = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_host.inc')).read()
    body = src[src.index('int rr_step('):src.index('int rr_render(')]
    assert body.count('k_joint_torque') == 1
    at = body.index('if (e->jt_on) hipLaunchKernelGGL(k_joint_torque,')
    assert body.index('if (!e->la_valid) state_part_all(e, overlap);') < body.index('bind_frames(e);') < at < body.index('plan_step(in)')
    assert 'e->stream' in body[at:body.index('\n', at)] and 'TIMED' not in body[at:body.index('\n', at)]
    # rr_fork.inc, rr_prep.inc and rr_solve.inc know nothing of the table
    for f in ('rr_fork.inc', 'rr_prep.inc', 'rr_solve.inc'):
        assert 'jt_' not in open(os.path.join(ROOT, 'real_robots_amd', 'csrc', f)).read(), f


class _FakeDevice:
    """An object that says it is device memory (`__cuda_array_interface__`); never dereferenced: the checks run before the library."""

    def __init__(self, shape, typestr='<f4', strides=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x1000, False), version=2, strides=strides)


def test_python_side_arguments_and_refusals_need_no_device():
    N = 4
    args = BatchedREALRobotEnv._torque_args
    assert args(N, None, None)[:4] == (None, 0, None, 0)
    # numpy broadcasts to [N, 11]
    for t in (np.ones((N, 11), np.float32), np.ones(11), 2.5, np.ones((1, 11), np.float64), [[1.0] * 11] * N):
        tp, t_dev, mp, m_dev, keep = args(N, t, None)
        assert t_dev == 0 and mp is None and keep[-1].shape == (N, 11) and keep[-1].dtype == np.float32 and tp == keep[-1].ctypes.data
    m = np.array([1, 0, 0, 1], np.uint8)
    tp, t_dev, mp, m_dev, keep = args(N, np.ones(11), m)
    assert (t_dev, m_dev) == (0, 0) and mp == keep[0].ctypes.data and np.array_equal(keep[0], m)
    assert args(N, None, np.array([True, False, False, True]))[2] is not None          # a mask alone: zero those rows
    # a non-finite value counts in the masked rows only
    t = np.ones((N, 11), np.float32)
    t[1, 3] = np.nan
    args(N, t, m)
    for bad_mask in (None, np.array([0, 1, 0, 0], np.uint8)):
        with pytest.raises(ValueError, match='finite'):
            args(N, t, bad_mask)
    with pytest.raises(ValueError, match='finite'):
        args(N, 1e39, None)                                                              # not finite in float32
    # device objects: the full shape, [N, 11] or the [N, 1, 11] view of posture_dynamics(), float32, compact
    for shape in ((N, 11), (N, 1, 11)):
        tp, t_dev, mp, m_dev, _ = args(N, _FakeDevice(shape), None)
        assert (tp, t_dev, mp) == (0x1000, 1, None)
    view = nat.DeviceBuffer(0x2000, (N, 1, 11), '<f4', None)
    assert args(N, view, _FakeDevice((N,), '|u1'))[:4] == (0x2000, 1, 0x1000, 1)
    bad = [
        (np.ones((N, 10)), None),                                    # shape
        (np.ones((N + 1, 11)), None),
        (np.ones((N, 11)), np.ones(N + 1, np.uint8)),                # mask shape
        (_FakeDevice((11,)), None),                                  # a device object does not broadcast
        (_FakeDevice((1, 11)), None),
        (_FakeDevice((N, 11, 1)), None),
        (_FakeDevice((N, 11), '<f8'), None),                         # dtype
        (_FakeDevice((N, 11), '<f4', (88, 4)), None),                # not compact
        (_FakeDevice((N, 11)), m),                                   # mixed sides
        (np.ones((N, 11), np.float32), _FakeDevice((N,), '|u1')),
        (_FakeDevice((N, 11)), _FakeDevice((N,), '<i4')),            # mask dtype
    ]
    for t, mk in bad:
        with pytest.raises(ValueError):
            args(N, t, mk)
    with pytest.raises(ValueError, match='same side'):
        args(N, _FakeDevice((N, 11)), m)


def test_nine_entry_torques_map_through_q_from_cmd():
    """The documented map for users who think in the nine command entries: [N, 9] @ Q_FROM_CMD.T -> [N, 11] puts entry 7 on q[7] and
    q[9] and minus entry 8 on q[8] and q[10]; @ Q_FROM_CMD is the generalised force on the command entries (virtual work:
    tau9 . dcmd = tau11 . dq with dq = Q dcmd)."""
    Q = nat.Q_FROM_CMD
    assert Q.shape == (11, 9)
    t9 = np.arange(1.0, 10.0)[None]
    t11 = t9 @ Q.T
    assert t11.shape == (1, 11) and np.array_equal(t11[0], [1, 2, 3, 4, 5, 6, 7, 8, -9, 8, -9])
    rng = np.random.default_rng(0)
    tau, dcmd = rng.normal(size=(5, 11)), rng.normal(size=(5, 9))
    assert np.allclose(np.einsum('ni,ni->n', tau @ Q, dcmd), np.einsum('ni,ni->n', tau, dcmd @ Q.T))
    for doc in (BatchedREALRobotEnv.set_joint_torques.__doc__,):
        assert 'torques9 @ _native.Q_FROM_CMD.T' in doc and 'torques11 @ _native.Q_FROM_CMD' in doc


def test_vector_env_spaces_with_and_without_joint_torque_actions():
    from real_robots_amd.vector import Kuka
    robot = Kuka(False, 3, 64, 64, env=None)
    N = 6
    single0, batched0 = REALRobotVectorEnv._action_spaces(robot, N)
    assert list(single0.spaces) == ['joint_command', 'render'] and list(batched0.spaces) == ['joint_command', 'render']
    single, batched = REALRobotVectorEnv._action_spaces(robot, N, True)
    assert list(single.spaces) == ['joint_command', 'render', 'joint_torques'] and list(batched.spaces) == list(single.spaces)
    s, b = single.spaces['joint_torques'], batched.spaces['joint_torques']
    assert s.shape == (11,) and b.shape == (N, 11) and s.dtype == b.dtype == np.float32
    assert np.isneginf(s.low).all() and np.isposinf(s.high).all() and np.isneginf(b.low).all() and np.isposinf(b.high).all()
    for key in ('joint_command', 'render'):                        # the default's entries are those of the torque env
        assert single.spaces[key].shape == single0.spaces[key].shape and batched.spaces[key].shape == batched0.spaces[key].shape
    assert batched0.spaces['joint_command'].shape == (N, 9)
