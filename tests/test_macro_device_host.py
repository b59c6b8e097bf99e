"""Tests of the C boundary of the device-resident macro actions (rr_step_macro, include/realrobot.h) that need no GPU: the header,
the binding, the refusals that need no handle, the Python-side argument checks and the vector env's spaces.  The GPU side is
tests/test_gpu_macro_device.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.envs.robot import Kuka
from real_robots_amd.vector import REALRobotVectorEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_step_macro', 'rr_macro_invalidate', 'rr_macro_buffer', 'rr_macro_copy_to_host')


def test_header_declares_the_entry_points_and_the_enum():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION
    assert re.search(r'\bint\s+rr_step_macro\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*macro\s*(/\*.*?\*/)?\s*,\s*int32_t\s+macro_on_device\s*,'
                     r'\s*const\s+uint8_t\s*\*\s*idle\s*(/\*.*?\*/)?\s*,\s*int32_t\s+idle_on_device\s*,\s*int32_t\s+render_mode\s*,'
                     r'\s*const\s+uint8_t\s*\*\s*render_flags_host\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_macro_invalidate\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+uint8_t\s*\*\s*env_mask\s*,\s*int32_t\s+mask_on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_macro_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_macro_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    for k, name in enumerate(('RR_MACRO_REQUEST', 'RR_MACRO_POSITION', 'RR_MACRO_REPLANNED', 'RR_MACRO_PLAN', 'RR_MACRO_COUNT')):
        assert re.search(r'\b%s\s*=\s*%d\b' % (name, k), h), name
    assert (nat.MACRO_REQUEST, nat.MACRO_POSITION, nat.MACRO_REPLANNED, nat.MACRO_PLAN) == (0, 1, 2, 3)
    assert nat.MACRO_NAMES == ('request', 'position', 'replanned', 'plan')
    doc = h[h.index('Device-resident macro actions'):h.index('int rr_macro_copy_to_host(')]
    for word in ('env.py:388-467', 'IEEE ==', '-0.0 equals 0.0', 'NaN', 'position >= 1000', 'PRESENT joints', 'RR_SOLVER_IK_SINGLE_SEED', 'zeros(9)',
                 'min(position, 999)', 'WITHOUT a wait', 'not validated', 'mixed pair', 'bad render_mode', 'rr_reset', 'rr_write_state', 'rr_copy_envs',
                 'checkpoint restores', 'policy state', 'rr_plan_macro', 'rr_step_plan', 'three buffers alone', 'all or nothing', 'RR_EINVAL'):
        assert word in doc, word


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert [len(getattr(L, n).argtypes) for n in NEW] == [7, 3, 4, 4]
    # the refusals that need no device: a null env -- RR_EINVAL with the entry point's name
    assert L.rr_step_macro(None, None, 0, None, 0, 0, None) == -1 and 'rr_step_macro: null env' in L.rr_last_error().decode()
    assert L.rr_macro_invalidate(None, None, 0) == -1 and 'rr_macro_invalidate: null env' in L.rr_last_error().decode()
    assert L.rr_macro_buffer(None, 0, None, None) == -1 and 'rr_macro_buffer: bad buffer' in L.rr_last_error().decode()
    buf = (C.c_char * 4)()
    assert L.rr_macro_copy_to_host(None, 0, buf, 4) == -1 and 'rr_macro_copy_to_host: bad buffer' in L.rr_last_error().decode()
    assert L.rr_macro_copy_to_host(None, 0, None, 4) == -1 and 'null destination' in L.rr_last_error().decode()


def test_the_refusals_come_first_and_the_call_never_waits_on_device_arguments():
    """On the source: every refusal stands in front of the first allocation, copy or launch; the launches come in the documented
    order on the main stream; the only wait is the staging helper's, which a device caller does not take; nothing is read back."""
    src = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_host.inc')).read()
    body = src[src.index('int rr_step_macro('):src.index('int rr_macro_invalidate(')]
    first_effect = min(body.index(w) for w in ('ensure_macro(', 'hipMemcpyAsync', 'hipLaunchKernelGGL', 'st.in('))
    assert body.index('null env') < body.index('null macro') < body.index('bad render_mode') < body.index('same side') < first_effect
    order = [body.index(w) for w in ('st.in(', 'k_macro_decide,', 'k_macro_replan,', 'k_plan_fetch,', 'rr_step(e, e->D.cmd, 1,', 'st.wait()')]
    assert order == sorted(order)
    assert 'hipStreamSynchronize' not in body and 'hipDeviceSynchronize' not in body and 'DeviceToHost' not in body
    assert 'hipStreamCreate' not in body and 'hipEventCreate' not in body
    assert body.count('hipLaunchKernelGGL') == 3 and body.count('e->stream') >= 3
    assert 'const HostStaging st = {e, !macro_on_device};' in body
    # the on-demand memory goes through the one owner
    ens = src[src.index('static int ensure_macro('):src.index('int rr_step_macro(')]
    assert 'ensure_group(' in ens and 'hipMalloc' not in ens
    # the existing entry points keep their text
    assert 'hipLaunchKernelGGL(k_plan_macro, dim3((N + 63) / 64), dim3(64), 0, e->stream, e->IK, e->P, e->D, e->ik_out, m, e->plan, e->plan_step);' in src
    ker = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_macro.inc')).read()
    assert 'atomic' not in ker.replace('No atomics', '') and '__shfl' not in ker


class _FakeDevice:
    """An object that says it is device memory (`__cuda_array_interface__`); never dereferenced: the checks run before the library."""

    def __init__(self, shape, typestr='<f4', strides=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x1000, False), version=2, strides=strides)


def test_python_side_arguments_and_refusals_need_no_device():
    N = 5
    args = BatchedREALRobotEnv._macro_args
    for m in (np.zeros((N, 2, 2)), np.zeros((N, 4), np.float32), [[[0.0, 0.1], [0.2, 0.3]]] * N, np.zeros((N, 4), np.int64)):
        mp, m_dev, ip, keep = args(N, m, None)
        assert m_dev == 0 and ip is None and keep[0].shape == (N, 4) and keep[0].dtype == np.float32 and mp == keep[0].ctypes.data
    idle = np.array([1, 0, 0, 1, 0], np.uint8)
    mp, m_dev, ip, keep = args(N, np.zeros((N, 2, 2)), idle)
    assert m_dev == 0 and ip == keep[1].ctypes.data
    assert args(N, np.zeros((N, 4)), idle.astype(bool))[2] is not None
    for shape in ((N, 2, 2), (N, 4)):
        assert args(N, _FakeDevice(shape), None)[:3] == (0x1000, 1, None)
    view = nat.DeviceBuffer(0x2000, (N, 4), '<f4', None)
    assert args(N, view, _FakeDevice((N,), '|u1'))[:3] == (0x2000, 1, 0x1000)
    assert args(N, view, _FakeDevice((N,), '|b1'))[:3] == (0x2000, 1, 0x1000)
    bad = [
        (np.zeros((N, 3)), None),                                     # shape
        (np.zeros((N + 1, 2, 2)), None),
        (np.zeros((N, 2, 2, 1)), None),
        (np.zeros(4), None),
        (np.zeros((N, 4), complex), None),                            # dtype
        (np.array([['a'] * 4] * N), None),
        (np.zeros((N, 4)), np.zeros(N + 1, np.uint8)),                # idle shape
        (np.zeros((N, 4)), np.zeros(N, np.float32)),                  # idle dtype
        (_FakeDevice((N, 4), '<f8'), None),                           # a device tensor must be float32
        (_FakeDevice((N, 4), '<f2'), None),
        (_FakeDevice((N, 3)), None),
        (_FakeDevice((4,)), None),
        (_FakeDevice((N, 4), '<f4', (32, 4)), None),                  # not compact
        (_FakeDevice((N, 4)), _FakeDevice((N,), '<i4')),              # idle dtype on the device
        (_FakeDevice((N, 4)), idle),                                  # mixed sides
        (np.zeros((N, 4)), _FakeDevice((N,), '|u1')),
    ]
    for m, i in bad:
        with pytest.raises(ValueError):
            args(N, m, i)
    with pytest.raises(ValueError, match='same side'):
        args(N, _FakeDevice((N, 4)), idle)
    # step_macro_device raises them before it touches the library: an object without a handle is enough
    ghost = object.__new__(BatchedREALRobotEnv)
    ghost.N, ghost.h, ghost.L = N, None, None
    for m, i in bad:
        with pytest.raises(ValueError):
            ghost.step_macro_device(m, idle=i)
    with pytest.raises(ValueError, match='unknown macro buffer'):
        ghost.macro_buffer('plans')
    with pytest.raises(ValueError, match='unknown macro buffer'):
        ghost.macro_buffer(4)
    with pytest.raises(ValueError):
        ghost.macro_invalidate(np.zeros(N + 1, np.uint8))
    assert list(inspect.signature(BatchedREALRobotEnv.step_macro_device).parameters)[1:] == ['macro_actions', 'idle', 'render']
    assert list(inspect.signature(BatchedREALRobotEnv.macro_invalidate).parameters)[1:] == ['env_mask']
    assert list(inspect.signature(BatchedREALRobotEnv.macro_buffer).parameters)[1:] == ['name', 'host']
    # step_macro is not rerouted: it keeps its host bookkeeping
    text = inspect.getsource(BatchedREALRobotEnv.step_macro)
    assert '_macro_req' in text and 'rr_step_macro' not in text and 'step_macro_device' not in text


def test_vector_env_action_spaces():
    N = 3
    robot = Kuka(False, 3, 64, 64, env=None)
    single, batched = REALRobotVectorEnv._action_spaces(robot, N, action_type='macro_action')
    assert set(single.spaces) == set(batched.spaces) == {'macro_action', 'render'}
    lo, hi = np.array([[-0.25, -0.5], [-0.25, -0.5]]), np.array([[0.05, 0.5], [0.05, 0.5]])         # macro_space, env.py:49-52
    assert single['macro_action'].shape == (2, 2) and np.array_equal(single['macro_action'].low, lo) and np.array_equal(single['macro_action'].high, hi)
    assert batched['macro_action'].shape == (N, 2, 2)
    assert np.array_equal(batched['macro_action'].low, np.broadcast_to(lo, (N, 2, 2))) and np.array_equal(batched['macro_action'].high, np.broadcast_to(hi, (N, 2, 2)))
    assert batched['render'].shape == (N,) and single['render'].shape == (1,)
    assert batched.contains(batched.sample())
    # the default is unchanged
    d_single, d_batched = REALRobotVectorEnv._action_spaces(robot, N)
    assert set(d_single.spaces) == set(d_batched.spaces) == {'joint_command', 'render'}
    assert d_batched['joint_command'].shape == (N, 9) and d_single['joint_command'].shape == (9,)
    j_single, j_batched = REALRobotVectorEnv._action_spaces(robot, N, False, False, 'joints')
    assert set(j_batched.spaces) == set(d_batched.spaces) and np.array_equal(j_batched['joint_command'].low, d_batched['joint_command'].low)
    sig = inspect.signature(REALRobotVectorEnv.__init__).parameters
    assert sig['action_type'].default == 'joints' and sig['action_type'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig['macro_replan_on_reset'].default is False and sig['macro_replan_on_reset'].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match='action_type'):
        REALRobotVectorEnv(2, action_type='cartesian')
    with pytest.raises(ValueError, match='macro_replan_on_reset'):
        REALRobotVectorEnv(2, macro_replan_on_reset=True)
