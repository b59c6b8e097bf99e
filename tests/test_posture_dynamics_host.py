"""Tests of the C boundary of the joint-space dynamics at candidate postures (rr_posture_dynamics, include/realrobot.h) that need no
GPU: the header, the enum, the binding, the refusals that need no handle and the Python-side argument checks.  The GPU side is
tests/test_gpu_posture_dynamics.py, the reference's own tests tests/test_numpy_dynamics.py."""
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
NEW = ('rr_posture_dynamics', 'rr_posture_dynamics_buffer', 'rr_posture_dynamics_copy_to_host')


def test_header_declares_the_enum_and_keeps_abi_7():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    pd = dict((k, int(v)) for k, v in re.findall(r'\b(RR_PD_[A-Z_]+)\s*=\s*(\d+)', h))
    assert pd == dict(RR_PD_MASS_MATRIX=0, RR_PD_GRAVITY=1, RR_PD_BIAS=2, RR_PD_TORQUE=3, RR_PD_MASS_INVERSE=4, RR_PD_COUNT=5, RR_PD_INVERSE=1)
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'#define\s+RR_PC_MAX_POSTURES\s+(\d+)', h).group(1)) == nat.PC_MAX_POSTURES == 32
    assert re.search(r'\bint\s+rr_posture_dynamics\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*postures\s*(/\*.*?\*/)?\s*,'
                     r'\s*const\s+float\s*\*\s*velocities\s*(/\*.*?\*/)?\s*,\s*const\s+float\s*\*\s*accelerations\s*(/\*.*?\*/)?\s*,'
                     r'\s*int32_t\s+n_postures\s*,\s*int32_t\s+on_device\s*,\s*uint32_t\s+flags\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_dynamics_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_dynamics_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    doc = h[h.index('Joint-space dynamics at candidate joint postures on the device'):h.index('int rr_posture_dynamics_copy_to_host(')]
    for word in ('calculateMassMatrix', 'calculateInverseDynamics', 'velocities == NULL', 'accelerations == NULL', 'postures == NULL',
                 'PRESENT-STATE', 'read and never written', 'same bytes as RR_PD_GRAVITY', 'same bytes as RR_PD_BIAS', 'mixed set', 'NOT validated',
                 'NOT clamped', "HANDLE'S OWN", 'use_urdf_inertia', "Gravity is the step's", 'Joint damping and the motors are NOT', 'BIT FOR BIT',
                 'exactly +0.0', 'ALONE', 'not an input', 'No effect on the simulation', 'RR_F_PREP', 'look-ahead stays valid', 'forms an address',
                 'non-finite', 'No atomics', 'RR_EINVAL', 'nothing allocated', '35 200', '144 MB', 'pointer ever changes', '0 before the first',
                 'left as it was', 'STREAM CONTRACT', 'Out of scope', 'operational-space inertia', 'derivatives'):
        assert word in doc, word
    # the figure of the header: 32 rows x (2 x 121 + 3 x 11) floats per env
    assert nat.PC_MAX_POSTURES * (2 * nat.N_JOINTS ** 2 + 3 * nat.N_JOINTS) * 4 == 35200


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_posture_dynamics.argtypes) == 7
    assert len(L.rr_posture_dynamics_buffer.argtypes) == 4 and len(L.rr_posture_dynamics_copy_to_host.argtypes) == 4
    assert nat.PD_FIELDS == ('mass_matrix', 'gravity', 'bias', 'torque', 'mass_inverse') and nat.PD_INVERSE == 1
    # the refusals that need no device: a null env, a null destination -- RR_EINVAL with the entry point's name
    assert L.rr_posture_dynamics(None, None, None, None, 1, 0, 0) == -1 and 'rr_posture_dynamics: null env' in L.rr_last_error().decode()
    assert L.rr_posture_dynamics_buffer(None, 0, None, None) == -1 and 'rr_posture_dynamics_buffer: null env' in L.rr_last_error().decode()
    assert L.rr_posture_dynamics_copy_to_host(None, 0, None, 0) == -1 and 'rr_posture_dynamics_copy_to_host: null env' in L.rr_last_error().decode()
    # (that a null destination is refused in front of everything that needs the handle's contents is checked on the accessor itself,
    # against a fake handle: tests/test_query_layout.py::test_the_copy_accessor)
    for name in ('posture_dynamics', 'posture_dynamics_buffer'):
        assert callable(getattr(BatchedREALRobotEnv, name))
    assert list(inspect.signature(BatchedREALRobotEnv.posture_dynamics).parameters)[1:] == ['postures', 'velocities', 'accelerations', 'inverse', 'host']
    p = inspect.signature(REALRobotVectorEnv.__init__).parameters['dynamics_obs']
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


class _FakeDevice:
    """An object that says it is device memory (`__cuda_array_interface__`); never dereferenced: the checks run before the library."""

    def __init__(self, shape, typestr='<f4'):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x1000, False), version=2, strides=None)


def test_python_side_refusals_need_no_device():
    N, K = 4, 3
    args = BatchedREALRobotEnv._dynamics_args
    ok = np.zeros((N, K, 11), np.float32)
    k, ptrs, on_dev, keep = args(N, ok, ok.copy(), None)
    assert k == K and on_dev == 0 and ptrs[0] == ok.ctypes.data and ptrs[2] is None and len(keep) == 2
    k, ptrs, on_dev, _ = args(N, _FakeDevice((N, K, 11)), None, _FakeDevice((N, K, 11)))
    assert k == K and on_dev == 1 and ptrs == [0x1000, None, 0x1000]
    k, ptrs, on_dev, _ = args(N, None, None, None)                      # the present-state form
    assert k == 1 and ptrs == [None, None, None]
    assert args(N, None, None, np.zeros((N, 1, 11), np.float32))[0] == 1
    bad = [
        (np.zeros((N, K, 10), np.float32), None, None),                 # shape
        (np.zeros((N + 1, K, 11), np.float32), None, None),
        (np.zeros((N, 0, 11), np.float32), None, None),                 # K = 0
        (np.zeros((N, 33, 11), np.float32), None, None),                # K = 33
        (np.zeros((N, K, 11), np.float64), None, None),                 # dtype
        (np.zeros((N, 11, K), np.float32).transpose(0, 2, 1), None, None),      # not contiguous
        (ok, np.zeros((N, K + 1, 11), np.float32), None),               # velocities of another K
        (ok, np.zeros((N, K, 11), np.float64), None),
        (ok, None, np.zeros((N, K, 11), np.int32)),
        (ok, None, np.zeros((N, 11), np.float32)),
        (None, np.zeros((N, 1, 11), np.float32), None),                 # velocities without postures
        (None, None, np.zeros((N, 2, 11), np.float32)),                 # the present-state form has K = 1
        (ok, _FakeDevice((N, K, 11)), None),                            # mixed sides
        (_FakeDevice((N, K, 11)), None, ok),
        (_FakeDevice((N, K, 11)), _FakeDevice((N, K, 11)), ok),
        (_FakeDevice((N, K, 11), '<f8'), None, None),
    ]
    for q, qd, qdd in bad:
        with pytest.raises(ValueError):
            args(N, q, qd, qdd)
    with pytest.raises(ValueError, match='same side'):
        args(N, ok, _FakeDevice((N, K, 11)), None)
    with pytest.raises(ValueError, match='velocities without postures'):
        args(N, None, ok, None)
