"""CPU tests (-m "not gpu") of the signed-distance queries: the C boundary (header, binding, constants), the refusals that need no
device and the strided byte views of the status words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_signed_distance', 'rr_signed_buffer', 'rr_signed_copy_to_host')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_enum_and_keeps_abi_7():
    h = _header()
    sd = dict((k, int(v)) for k, v in re.findall(r'\b(RR_SD_[A-Z_]+)\s*=\s*(\d+)', h))
    assert sd == dict(RR_SD_DEEPEST=0, RR_SD_ID=1, RR_SD_SIGNED=2, RR_SD_STATUS=3, RR_SD_POINTS=4, RR_SD_COUNT=5)
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_PC_COUNT\s*=\s*(\d+)', h).group(1)) == 4 and int(re.search(r'\bRR_DIST_COUNT\s*=\s*(\d+)', h).group(1)) == 2
    assert int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16 and int(re.search(r'#define\s+RR_PC_MAX_POSTURES\s+(\d+)', h).group(1)) == 32
    assert int(re.search(r'#define\s+RR_DIST_MAX\s+(\d+)', h).group(1)) == nat.DIST_MAX == 96
    assert re.search(r'\bint\s+rr_signed_distance\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*postures\s*(/\*.*?\*/)?\s*,\s*int32_t\s+n_postures\s*,'
                     r'\s*int32_t\s+on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_signed_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_signed_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    doc = h[h.index('Signed distance and penetration depth on the device'):h.index('int rr_signed_copy_to_host(')]
    for word in ('FIRST MINIMUM', 'STREAM CONTRACT', 'Out of scope', 'unspecified', 'rr_posture_clearance', 'NaN never wins', 'RR_PC_MAX_POSTURES',
                 'pointer ever changes', 'no atomics', 'a - b = signed * n', 'PRESENT-STATE', 'gradients', 'non-convex', 'vector env', 'narrow phase'):
        assert word in doc, word
    for status in range(6):
        assert re.search(r'\*\s+%d  ' % status, doc), status


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 4 and getattr(L, name).restype is C.c_int32, name
    assert nat.SD_FIELDS == ('deepest', 'id', 'signed', 'status', 'points')
    assert nat.PC_FIELDS == ('nearest', 'id', 'distance', 'status') and nat.DIST_FIELDS == ('points', 'id')
    # the refusals that need no device: a null env
    assert L.rr_signed_distance(None, None, 0, 0) == -1 and 'rr_signed_distance: null env' in L.rr_last_error().decode()
    assert L.rr_signed_buffer(None, 0, None, None) == -1 and 'rr_signed_buffer: null env' in L.rr_last_error().decode()
    buf = np.zeros(4, np.float32)
    assert L.rr_signed_copy_to_host(None, 0, buf.ctypes.data, 16) == -1 and 'rr_signed_copy_to_host: null env' in L.rr_last_error().decode()
    assert hasattr(BatchedREALRobotEnv, 'signed_distance') and hasattr(BatchedREALRobotEnv, 'signed_buffer')


def test_strided_byte_views_of_the_status_words():
    st = nat.DeviceBuffer(4096, (5, 3, 80), '<i4', None)
    ps, pi = BatchedREALRobotEnv.status_bytes(st)                      # the default keeps the two views of posture_clearance
    assert ps.ptr == 4096 and pi.ptr == 4097
    pi2, pe = BatchedREALRobotEnv.status_bytes(st, 1)
    assert pi2.ptr == 4097 and pe.ptr == 4098 and pe.shape == (5, 3, 80) and pe.strides == (3 * 80 * 4, 80 * 4, 4) and pe.typestr == '|u1'
    assert BatchedREALRobotEnv.status_bytes(st, offset=2)[1].ptr == 4099
    k = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    host = (k % 6) | ((k % 32) << 8) | ((31 - k) << 16)
    hs, hi = BatchedREALRobotEnv.status_bytes(host)
    hi2, he = BatchedREALRobotEnv.status_bytes(host, 1)
    assert he.dtype == np.uint8 and (hs == k % 6).all() and (hi == k % 32).all() and (hi2 == hi).all() and (he == 31 - k).all() and np.shares_memory(he, host)
    for bad in (3, -1, True, 1.0, None):
        with pytest.raises(ValueError):
            BatchedREALRobotEnv.status_bytes(host, bad)
