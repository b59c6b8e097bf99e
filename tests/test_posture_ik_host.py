"""Tests of the C boundary of the inverse kinematics at candidate targets (rr_posture_ik, include/realrobot.h) that need no GPU: the
header, the enum, the options struct, the binding and the refusals that need no handle.  The GPU side is tests/test_gpu_posture_ik.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_posture_ik', 'rr_posture_ik_buffer', 'rr_posture_ik_copy_to_host')


def test_header_declares_the_block_and_keeps_abi_7():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    pik = dict((k, int(v)) for k, v in re.findall(r'\b(RR_PIK_[A-Z_]+)\s*=\s*(\d+)u?\b', h))
    assert pik == dict(RR_PIK_POSITION_ONLY=1, RR_PIK_CLAMP_LIMITS=2, RR_PIK_POSTURE=0, RR_PIK_RESULT=1, RR_PIK_INFO=2, RR_PIK_COUNT=3)
    assert (nat.PIK_POSITION_ONLY, nat.PIK_CLAMP_LIMITS) == (1, 2)
    assert int(re.search(r'#define\s+RR_PIK_MAX_ITERATIONS\s+(\d+)', h).group(1)) == nat.PIK_MAX_ITERATIONS == 256
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    for name, value in (('RR_KIN_COUNT', 7), ('RR_PC_COUNT', 4), ('RR_PK_COUNT', 3), ('RR_F_COUNT', 16)):
        assert int(re.search(r'\b%s\s*=\s*(\d+)' % name, h).group(1)) == value, name
    assert int(re.search(r'#define\s+RR_PC_MAX_POSTURES\s+(\d+)', h).group(1)) == nat.PC_MAX_POSTURES == 32
    # the struct: field order and types are the binding's
    body = re.search(r'typedef\s+struct\s+rr_ik_options\s*\{(.*?)\}\s*rr_ik_options\s*;', h, re.S).group(1)
    fields = re.findall(r'^\s*(int32_t|uint32_t|float)\s+(\w+)\s*;', body, re.M)
    ctype = {'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'float': C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(nat.IkOptions._fields_)
    assert [n for _, n in fields] == ['point', 'max_iterations', 'tolerance', 'damping', 'max_step', 'flags']
    assert C.sizeof(nat.IkOptions) == 24
    d = nat.IkOptions()
    assert (d.point, d.max_iterations, d.flags) == (0, 32, nat.PIK_CLAMP_LIMITS)
    assert (d.tolerance, d.damping, d.max_step) == (np.float32(1e-3), np.float32(0.1), np.float32(0.5))
    assert re.search(r'\bint\s+rr_posture_ik\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*targets\s*(/\*.*?\*/)?\s*,\s*const\s+float\s*\*\s*seeds\s*(/\*.*?\*/)?\s*,'
                     r'\s*int32_t\s+n_targets\s*,\s*int32_t\s+on_device\s*,\s*const\s+rr_ik_options\s*\*\s*opt\s*(/\*.*?\*/)?\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_ik_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_ik_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    # behind the rr_posture_kinematics block, in front of rr_ik
    assert h.index('int rr_posture_kinematics_copy_to_host(') < h.index('Inverse kinematics at candidate targets on the device') < h.index('int rr_ik(')
    doc = h[h.index('Inverse kinematics at candidate targets on the device'):h.index('int rr_posture_ik_copy_to_host(')]
    for word in ('rr_set_kinematic_points', 'normalises', 'gripper base', 'seeds == NULL', 'never writes', 'STREAM CONTRACT', 'rr_posture_clearance',
                 '[N, 32, 7]', 'all or nothing', 'seven arm joints', 'fingers', 'keeps its seed value', 'link_3', 'antisymmetric',
                 'RR_PIK_POSITION_ONLY', '3 x 3', 'TRUE angle', 'Cholesky', 'max_step', 'body_limits', '(-pi, pi]', 'once more after the last',
                 'status 0', 'status 1', 'status 2', 'half-turn', 'unspecified', 'ALONE', 'No atomics', 'forms an address',
                 'No effect on the simulation', 'RR_F_PREP', 'rr_plan_macro', 'RR_EINVAL', 'nothing allocated', 'unknown flag', '2 176',
                 'pointer ever changes', '0 before the first', 'slowest row', 'Out of scope', 'cartesian actions', 'null-space', 'collision-aware',
                 'random restarts', 'vector env', 'ik_single_seed'):
        assert word in doc, word
    # the figure of the header: 32 targets x (11 + 4 + 2) four-byte values per env
    assert nat.PC_MAX_POSTURES * (nat.N_JOINTS + 4 + 2) * 4 == 2176


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_posture_ik.argtypes) == 6
    assert len(L.rr_posture_ik_buffer.argtypes) == 4 and len(L.rr_posture_ik_copy_to_host.argtypes) == 4
    assert nat.PIK_FIELDS == ('posture', 'result', 'info')
    # the refusals that need no device: a null env
    assert L.rr_posture_ik(None, None, None, 1, 0, None) == -1 and 'rr_posture_ik: null env' in L.rr_last_error().decode()
    assert L.rr_posture_ik_buffer(None, 0, None, None) == -1 and 'rr_posture_ik_buffer' in L.rr_last_error().decode()
    assert L.rr_posture_ik_copy_to_host(None, 0, None, 0) == -1 and 'rr_posture_ik_copy_to_host' in L.rr_last_error().decode()
    for name in ('posture_ik', 'posture_ik_buffer'):
        assert callable(getattr(BatchedREALRobotEnv, name))


class _NoLibrary:
    """Stands in for the library: any native call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("native call %s" % name)


class _FakeDevice:
    """A `__cuda_array_interface__` object: device memory as far as `_state_arg` can tell."""

    def __init__(self, shape, typestr='<f4'):
        self.shape = shape
        self.__cuda_array_interface__ = {'shape': shape, 'typestr': typestr, 'data': (4096, False), 'version': 2, 'strides': None}


def test_posture_ik_refuses_bad_arguments_before_any_native_call():
    env = object.__new__(BatchedREALRobotEnv)
    env.N, env.L, env.h = 3, _NoLibrary(), None
    good_t, good_s = np.zeros((3, 5, 7), np.float32), np.zeros((3, 5, 11), np.float32)
    for targets, seeds in ((np.zeros((3, 5, 6), np.float32), None), (np.zeros((2, 5, 7), np.float32), None), (np.zeros((3, 7), np.float32), None),
                           (np.zeros((3, 0, 7), np.float32), None), (np.zeros((3, 33, 7), np.float32), None),
                           (good_t.astype(np.float64), None), (np.zeros((3, 7, 5), np.float32).transpose(0, 2, 1), None), (7.0, None),
                           (good_t, np.zeros((3, 4, 11), np.float32)), (good_t, np.zeros((3, 5, 9), np.float32)), (good_t, good_s.astype(np.float64)),
                           (_FakeDevice((3, 5, 7), '<f8'), None),
                           (good_t, _FakeDevice((3, 5, 11))), (_FakeDevice((3, 5, 7)), good_s)):          # the last two: a mixed host / device pair
        with pytest.raises(ValueError):
            env.posture_ik(targets, seeds)
    with pytest.raises(ValueError, match='same side'):
        env.posture_ik(good_t, _FakeDevice((3, 5, 11)))
    for bad in ('pose', 3, -1, True, None):
        with pytest.raises(ValueError):
            env.posture_ik_buffer(bad)
