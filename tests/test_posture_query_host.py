"""CPU tests (-m "not gpu") of the clearance queries at candidate postures: the C boundary (header, binding, constants), the host-side
argument check of `posture_clearance` and the strided byte views of the status words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_posture_clearance', 'rr_posture_buffer', 'rr_posture_copy_to_host')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_enum_and_keeps_abi_7():
    h = _header()
    pc = dict((k, int(v)) for k, v in re.findall(r'\b(RR_PC_[A-Z_]+)\s*=\s*(\d+)', h))
    assert pc == dict(RR_PC_NEAREST=0, RR_PC_ID=1, RR_PC_DISTANCE=2, RR_PC_STATUS=3, RR_PC_COUNT=4)
    assert int(re.search(r'#define\s+RR_PC_MAX_POSTURES\s+(\d+)', h).group(1)) == nat.PC_MAX_POSTURES == 32
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_DIST_COUNT\s*=\s*(\d+)', h).group(1)) == 2 and int(re.search(r'\bRR_RAY_COUNT\s*=\s*(\d+)', h).group(1)) == 2
    assert int(re.search(r'\bRR_KIN_COUNT\s*=\s*(\d+)', h).group(1)) == 7 and int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    assert re.search(r'\bint\s+rr_posture_clearance\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*postures\s*(/\*.*?\*/)?\s*,\s*int32_t\s+n_postures\s*,'
                     r'\s*int32_t\s+on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    doc = h[h.index('Clearance at candidate joint postures on the device'):h.index('int rr_posture_copy_to_host(')]
    for word in ('FIRST MINIMUM', 'STREAM CONTRACT', 'Out of scope', 'unspecified', 'Q_FROM_CMD', 'rr_closest_points', 'NaN never wins', 'RR_PC_MAX_POSTURES',
                 'pointer ever changes', 'K counts as 0', 'No atomics', 'Jacobians'):
        assert word in doc, word
    assert 'first minimum' in doc.lower()


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_posture_clearance.argtypes) == 4 and len(L.rr_posture_buffer.argtypes) == 4 and len(L.rr_posture_copy_to_host.argtypes) == 4
    assert nat.PC_FIELDS == ('nearest', 'id', 'distance', 'status') and nat.PC_MAX_POSTURES == 32
    # the refusals that need no device: a null env
    assert L.rr_posture_clearance(None, None, 1, 0) == -1 and 'rr_posture_clearance: null env' in L.rr_last_error().decode()
    assert L.rr_posture_buffer(None, 0, None, None) == -1 and 'rr_posture_buffer' in L.rr_last_error().decode()


def test_posture_argument_is_checked_on_the_host():
    """Every argument error is a ValueError raised before the native call: the check is a static method (no handle, no GPU)."""
    arg = BatchedREALRobotEnv._posture_arg
    good = np.zeros((5, 3, 11), np.float32)
    assert arg(good, 5) == 3 and arg(np.zeros((1, 1, 11), np.float32), 1) == 1 and arg(np.zeros((2, 32, 11), np.float32), 2) == 32

    class Cai:
        def __init__(self, shape, typestr='<f4', strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(4096, False), version=2, strides=strides)
    assert arg(Cai((5, 4, 11)), 5) == 4 and arg(Cai((5, 4, 11), strides=(176, 44, 4)), 5) == 4
    for bad, n in ((np.zeros((5, 0, 11), np.float32), 5), (np.zeros((5, 33, 11), np.float32), 5), (np.zeros((5, 3, 9), np.float32), 5),
                   (np.zeros((5, 3, 11), np.float64), 5), (np.zeros((5, 3, 22), np.float32)[:, :, ::2], 5), (np.zeros((3, 5, 11), np.float32).transpose(1, 0, 2), 5),
                   (good, 4), (np.zeros((5, 11), np.float32), 5), ([[0.0] * 11] * 5, 5), ([[[0.0] * 11] * 3] * 5, 5), ([[[[0.0] * 11]]], 1), (None, 5), ('postures', 5),
                   (Cai((5, 4, 11), '<f8'), 5), (Cai((5, 4, 11), strides=(352, 88, 8)), 5), (Cai((5, 4, 9)), 5)):
        with pytest.raises(ValueError):
            arg(bad, n)


def test_strided_byte_views_of_the_status_words():
    st = nat.DeviceBuffer(4096, (5, 3, 80), '<i4', None)
    ps, pi = BatchedREALRobotEnv.status_bytes(st)
    assert ps.ptr == 4096 and pi.ptr == 4097 and ps.shape == pi.shape == (5, 3, 80)
    assert ps.strides == pi.strides == (3 * 80 * 4, 80 * 4, 4) and ps.typestr == pi.typestr == '|u1'
    host = (np.arange(24, dtype=np.int32).reshape(2, 3, 4) % 4) | (np.arange(24, dtype=np.int32).reshape(2, 3, 4) << 8)
    hs, hi = BatchedREALRobotEnv.status_bytes(host)
    assert hs.dtype == hi.dtype == np.uint8 and (hs == host & 255).all() and (hi == host >> 8).all() and np.shares_memory(hs, host)
