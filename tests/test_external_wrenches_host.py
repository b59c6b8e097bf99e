"""Tests of the C boundary of the step's external wrenches (rr_set_external_wrenches, include/realrobot.h) that need no GPU: the
header, the binding, the refusals that need no handle, the Python-side argument checks and the vector env's spaces.  The GPU side is
tests/test_gpu_external_wrenches.py, the reference's own tests tests/test_numpy_wrench.py."""
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
NEW = ('rr_set_external_wrenches', 'rr_get_external_wrenches', 'rr_external_wrench_buffer')


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points_and_keeps_the_abi_numbers():
    h = _read('include', 'realrobot.h')
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert re.search(r'#define\s+RR_NUM_KERNELS\s+9\b', h) and re.search(r'\bRR_F_COUNT\s*=\s*16\b', h)
    assert int(re.search(r'#define\s+RR_XW_BODIES\s+(\d+)', h).group(1)) == nat.XW_BODIES == 14
    assert re.search(r'\bint\s+rr_set_external_wrenches\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*wrenches\s*(/\*.*?\*/)?\s*,\s*int32_t\s+wrenches_on_device\s*,'
                     r'\s*const\s+uint8_t\s*\*\s*env_mask\s*(/\*.*?\*/)?\s*,\s*int32_t\s+mask_on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_get_external_wrenches\s*\(\s*rr_env\s*\*\s*env\s*,\s*float\s*\*\s*out_host\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_external_wrench_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    doc = h[h.index('External wrenches on robot bodies and objects in the step'):h.index('int rr_external_wrench_buffer(')]
    doc = re.sub(r'\s*\n \*\s*', ' ', doc)                     # (the comment's line breaks are not part of its words)
    for word in ('applyExternalForce', 'applyExternalTorque', 'WORLD frame', 'CENTRE OF MASS', 'c_b = p_b + R_b com_b', 'rows 0..10', 'rows 11..13',
                 "v*' = v* + dt F / m_i", "w*' = w* + dt Iinv_i T", 'a_k . ((c_b - p_k) x F_b + T_b)', "qd*' = qd* + dt M^-1 tau", 'RR_F_PREP',
                 "ENV's own mass", 'HOME pose', 'NOT clamped', 'the torque term is added first, then the wrench term', 'T += r x F', 'PERSISTENT', 'unlike pybullet',
                 'nothing clears the table', 'rr_reset', 'auto-reset', 'rr_write_state', 'rr_set_state', 'rr_copy_envs', 'rr_checkpoint_restore',
                 'PER TARGET', 'either sign', 'NOT TOUCHED', 'bit for bit', 'frozen env', 'NaN counts as non-zero', 'wrenches == NULL',
                 'turns the feature OFF', 'never allocated', 'IN PLACE', 'STREAM CONTRACT', 'NOT validated', 'finiteness', 'env, row and entry',
                 'changes NOTHING', 'mixed pair', 'look-ahead stays valid', 'RR_EINVAL', 'all or nothing', 'N x 336 bytes', 'Out of scope'):
        assert word in doc, word
    # the torque section no longer calls wrenches out of scope, and keeps its own words
    tdoc = h[h.index('Joint torque inputs of the step'):h.index('int rr_joint_torque_buffer(')]
    assert 'wrenches on objects' not in tdoc and 'Out of scope' in tdoc and 'rr_set_external_wrenches' in tdoc
    v = _read('real_robots_amd', 'csrc', 'realrobot.hip')
    assert v.index('#include "rr_torque.inc"') < v.index('#include "rr_wrench.inc"')


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_set_external_wrenches.argtypes) == 5 and len(L.rr_get_external_wrenches.argtypes) == 2 and len(L.rr_external_wrench_buffer.argtypes) == 3
    # the refusals that need no device: a null env -- RR_EINVAL with the entry point's name
    assert L.rr_set_external_wrenches(None, None, 0, None, 0) == -1 and 'rr_set_external_wrenches: null env' in L.rr_last_error().decode()
    assert L.rr_get_external_wrenches(None, None) == -1 and 'rr_get_external_wrenches: null env' in L.rr_last_error().decode()
    assert L.rr_external_wrench_buffer(None, None, None) == -1 and 'rr_external_wrench_buffer: null env' in L.rr_last_error().decode()
    # the order of the refusals that need a handle, on the source: the mixed pair and the finiteness check come in front of the first
    # allocation, copy or launch, and of the flag -- a refusal changes nothing
    src = _read('real_robots_amd', 'csrc', 'rr_host.inc')
    body = src[src.index('int rr_set_external_wrenches('):src.index('int rr_external_wrench_buffer(')]
    first_effect = min(body.index(w) for w in ('ensure_wrenches(', 'hipMemcpyAsync', 'hipLaunchKernelGGL', 'e->xw_on ='))
    assert body.index('null env') < body.index('same side') < body.index('is not finite') < first_effect
    assert body.index('!wrenches && !e->xw_table') < body.index('ensure_wrenches(')       # zeroing a table that never was: nothing allocated
    assert 'la_valid' not in body and 'scratch' not in body and 'D.state' not in body     # neither the look-ahead, the record nor the state
    for name in ('set_external_wrenches', 'external_wrenches', 'wrench_row_names', '_wrench_args'):
        assert callable(getattr(BatchedREALRobotEnv, name))
    assert isinstance(BatchedREALRobotEnv.external_wrench_buffer, property)
    assert list(inspect.signature(BatchedREALRobotEnv.set_external_wrenches).parameters)[1:] == ['wrenches', 'env_mask']
    p = inspect.signature(REALRobotVectorEnv.__init__).parameters['external_wrench_actions']
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_the_step_launches_the_kernel_only_while_wrenches_are_set():
    """On the source: one host branch in rr_step, directly behind the torque launch, in front of the command line and the plan."""
    src = _read('real_robots_amd', 'csrc', 'rr_host.inc')
    body = src[src.index('int rr_step('):src.index('int rr_render(')]
    assert body.count('k_ext_wrench') == 1 and body.count('k_joint_torque') == 1
    jt = body.index('if (e->jt_on) hipLaunchKernelGGL(k_joint_torque,')
    at = body.index('if (e->xw_on) hipLaunchKernelGGL(k_ext_wrench,')
    assert body.index('bind_frames(e);') < jt < at < body.index('e->D.cmd_in =') < body.index('plan_step(in)')
    # nothing but comment lines between the two launches
    between = body[body.index('\n', jt) + 1:at].splitlines()
    assert all(l.strip().startswith('//') or not l.strip() for l in between), between
    line = body[at:body.index('\n', at)]
    assert 'e->stream' in line and 'TIMED' not in line and 'e->xw_table' in line
    # rr_fork.inc, rr_prep.inc and rr_solve.inc know nothing of the table; the kernel file holds no atomics
    for f in ('rr_fork.inc', 'rr_prep.inc', 'rr_solve.inc'):
        assert 'xw_' not in _read('real_robots_amd', 'csrc', f), f
    k = _read('real_robots_amd', 'csrc', 'rr_wrench.inc')
    code = '\n'.join(l.split('//')[0] for l in k.splitlines())
    assert 'atomic' not in code and '__shared__' not in code and '__shfl' not in code and '__builtin_amdgcn_ds_bpermute' in code
    assert "'k_ext_wrench'" in _read('tools', 'check_scratch.py')


class _FakeDevice:
    """An object that says it is device memory (`__cuda_array_interface__`); never dereferenced: the checks run before the library."""

    def __init__(self, shape, typestr='<f4', strides=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x1000, False), version=2, strides=strides)


def test_python_side_arguments_and_refusals_need_no_device():
    N = 4
    args = BatchedREALRobotEnv._wrench_args
    assert args(N, None, None)[:4] == (None, 0, None, 0)
    # numpy broadcasts to [N, 14, 6]
    for t in (np.ones((N, 14, 6), np.float32), np.ones(6), 2.5, np.ones((14, 6)), np.ones((1, 14, 6), np.float64), np.ones((N, 1, 6)), [[[1.0] * 6] * 14] * N):
        wp, w_dev, mp, m_dev, keep = args(N, t, None)
        assert w_dev == 0 and mp is None and keep[-1].shape == (N, 14, 6) and keep[-1].dtype == np.float32 and wp == keep[-1].ctypes.data
        assert keep[-1].flags.c_contiguous
    m = np.array([1, 0, 0, 1], np.uint8)
    wp, w_dev, mp, m_dev, keep = args(N, np.ones(6), m)
    assert (w_dev, m_dev) == (0, 0) and mp == keep[0].ctypes.data and np.array_equal(keep[0], m)
    assert args(N, None, np.array([True, False, False, True]))[2] is not None          # a mask alone: zero those rows
    # a non-finite value counts in the masked envs only
    t = np.ones((N, 14, 6), np.float32)
    t[1, 12, 3] = np.nan
    args(N, t, m)
    for bad_mask in (None, np.array([0, 1, 0, 0], np.uint8)):
        with pytest.raises(ValueError, match='finite'):
            args(N, t, bad_mask)
    with pytest.raises(ValueError, match='finite'):
        args(N, 1e39, None)                                                              # not finite in float32
    # the dict form: row names or indices, [N, 6] each, the other rows zero
    names = BatchedREALRobotEnv._wrench_rows(3)
    assert names == ['lbr_iiwa_link_1', 'lbr_iiwa_link_2', 'lbr_iiwa_link_3', 'lbr_iiwa_link_4', 'lbr_iiwa_link_5', 'lbr_iiwa_link_6', 'lbr_iiwa_link_7',
                     'finger_00', 'finger_01', 'finger_10', 'finger_11', 'cube', 'tomato', 'mustard']
    assert BatchedREALRobotEnv._wrench_rows(1) == names[:12]
    push = np.arange(N * 6, dtype=np.float64).reshape(N, 6)
    keep = args(N, {'cube': [0, 0, 14.7, 0, 0, 0], 6: push, 'finger_11': np.ones((1, 6))}, None)[4]
    a = keep[-1]
    assert a.shape == (N, 14, 6) and a.dtype == np.float32
    want = np.zeros((N, 14, 6), np.float32)
    want[:, 11, 2], want[:, 6], want[:, 10] = 14.7, push, 1.0
    assert np.array_equal(a, want)
    assert not args(N, {}, None)[4][-1].any()
    for bad in ({'mustard': np.ones(6)}, {13: np.ones(6)}):                              # an object a two-object handle does not have
        with pytest.raises(ValueError):
            args(N, bad, None, n_objects=2)
    args(N, {'tomato': np.ones(6), 12: np.ones(6)}, None, n_objects=2)
    for bad in ({'table': np.ones(6)}, {'base': np.ones(6)}, {14: np.ones(6)}, {-1: np.ones(6)}, {1.5: np.ones(6)}, {'cube': np.ones(5)}, {'cube': np.ones((N + 1, 6))},
                {'cube': [np.inf, 0, 0, 0, 0, 0]}):
        with pytest.raises(ValueError):
            args(N, bad, None)
    # device objects: the full shape, float32, compact
    wp, w_dev, mp, m_dev, _ = args(N, _FakeDevice((N, 14, 6)), None)
    assert (wp, w_dev, mp) == (0x1000, 1, None)
    view = nat.DeviceBuffer(0x2000, (N, 14, 6), '<f4', None)
    assert args(N, view, _FakeDevice((N,), '|u1'))[:4] == (0x2000, 1, 0x1000, 1)
    bad = [
        (np.ones((N, 14, 5)), None),                                    # shape
        (np.ones((N, 13, 6)), None),
        (np.ones((N + 1, 14, 6)), None),
        (np.ones((N, 14, 6)), np.ones(N + 1, np.uint8)),               # mask shape
        (_FakeDevice((14, 6)), None),                                  # a device object does not broadcast
        (_FakeDevice((1, 14, 6)), None),
        (_FakeDevice((N, 84)), None),
        (_FakeDevice((N, 14, 6), '<f8'), None),                        # dtype
        (_FakeDevice((N, 14, 6), '<f4', (672, 48, 8)), None),          # not compact
        (_FakeDevice((N, 14, 6)), m),                                  # mixed sides
        (np.ones((N, 14, 6), np.float32), _FakeDevice((N,), '|u1')),
        (_FakeDevice((N, 14, 6)), _FakeDevice((N,), '<i4')),           # mask dtype
    ]
    for t, mk in bad:
        with pytest.raises(ValueError):
            args(N, t, mk)
    with pytest.raises(ValueError, match='same side'):
        args(N, _FakeDevice((N, 14, 6)), m)


def test_vector_env_spaces_with_and_without_external_wrench_actions():
    from real_robots_amd.vector import Kuka
    robot = Kuka(False, 3, 64, 64, env=None)
    N = 6
    single0, batched0 = REALRobotVectorEnv._action_spaces(robot, N)
    assert list(single0.spaces) == ['joint_command', 'render'] and list(batched0.spaces) == ['joint_command', 'render']
    # the third positional argument keeps its meaning: joint torques
    single_t, batched_t = REALRobotVectorEnv._action_spaces(robot, N, True)
    assert list(single_t.spaces) == ['joint_command', 'render', 'joint_torques'] and list(batched_t.spaces) == list(single_t.spaces)
    single, batched = REALRobotVectorEnv._action_spaces(robot, N, external_wrench_actions=True)
    assert list(single.spaces) == ['joint_command', 'render', 'external_wrenches'] and list(batched.spaces) == list(single.spaces)
    both, _ = REALRobotVectorEnv._action_spaces(robot, N, True, True)
    assert list(both.spaces) == ['joint_command', 'render', 'joint_torques', 'external_wrenches']
    s, b = single.spaces['external_wrenches'], batched.spaces['external_wrenches']
    assert s.shape == (14, 6) and b.shape == (N, 14, 6) and s.dtype == b.dtype == np.float32
    assert np.isneginf(s.low).all() and np.isposinf(s.high).all() and np.isneginf(b.low).all() and np.isposinf(b.high).all()
    for key in ('joint_command', 'render'):
        assert single.spaces[key].shape == single0.spaces[key].shape and batched.spaces[key].shape == batched0.spaces[key].shape
