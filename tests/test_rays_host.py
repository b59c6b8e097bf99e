"""CPU tests (-m "not gpu") of the whole-batch ray casts: the C boundary (header, binding, constants) and the host-side argument
check of `set_rays`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_set_rays', 'rr_get_rays', 'rr_ray_cast', 'rr_ray_buffer', 'rr_ray_copy_to_host')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_enum_and_keeps_abi_7():
    h = _header()
    ray = dict((k, int(v)) for k, v in re.findall(r'\b(RR_RAY_[A-Z_]+)\s*=\s*(\d+)', h))
    assert ray == dict(RR_RAY_HIT=0, RR_RAY_ID=1, RR_RAY_COUNT=2)
    assert int(re.search(r'#define\s+RR_RAY_MAX\s+(\d+)', h).group(1)) == nat.RAY_MAX == 64
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    assert int(re.search(r'\bRR_KIN_COUNT\s*=\s*(\d+)', h).group(1)) == 7 and int(re.search(r'\bRR_EP_COUNT\s*=\s*(\d+)', h).group(1)) == 8
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(\s*rr_env\s*\*\s*env\b' % name, h), name
    doc = h[h.index('Ray casts against the collision hulls on the device'):h.index('int rr_ray_copy_to_host(')]
    for word in ('rayTestBatch', 'parentLinkIndex', 'STREAM CONTRACT', 'Out of scope'):
        assert word in doc, word


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert nat.RAY_FIELDS == ('hit', 'id') and nat.RAY_MAX == 64


def test_ray_arguments_are_checked_on_the_host():
    """Every argument error is a ValueError raised before the native call: the check is a static method (no handle, no GPU)."""
    arg = BatchedREALRobotEnv._rays_arg
    idx, seg = arg(['world', 'base', 'finger_01', 4, -1], np.arange(30).reshape(5, 6))
    assert idx.dtype == np.int32 and list(idx) == [-1, 8, nat.LINK_NAMES.index('finger_01'), 4, -1]
    assert seg.dtype == np.float32 and seg.shape == (5, 6) and seg[4, 5] == 29 and seg.flags.c_contiguous
    idx, seg = arg('base')
    assert list(idx) == [8] and seg.shape == (1, 6) and not seg.any()
    idx, seg = arg([])
    assert idx.shape == (0,) and seg.shape == (0, 6)
    idx, seg = arg([0] * 64)
    assert idx.shape == (64,)
    z6 = [0.0] * 6
    for bad in (dict(links=['no_such_link']), dict(links=[17]), dict(links=[-2]), dict(links=[0] * 65), dict(links=[1.5]), dict(links=[True]),
                dict(links=[8], segments=z6), dict(links=[8, 9], segments=[z6]), dict(links=[8], segments=[[0, 0, 0]]),
                dict(links=[8], segments=[[0, np.nan, 0, 0, 0, 0]]), dict(links=[8], segments=[[0, np.inf, 0, 0, 0, 0]]),
                dict(links=[8], segments=[[0, 1e39, 0, 0, 0, 0]]), dict(links=[8], segments=[['a'] * 6])):
        with pytest.raises(ValueError):
            arg(**bad)


def test_strided_device_view_of_a_column():
    """ray_column of a device buffer is a strided view: byte strides in __cuda_array_interface__, element strides in DLPack."""
    buf = nat.DeviceBuffer(4096, (5, 3, 8), '<f4', None)
    col = BatchedREALRobotEnv.ray_column(buf, 1)
    assert col.shape == (5, 3) and col.ptr == 4096 + 4 and col.strides == (96, 32)
    assert col.__cuda_array_interface__['strides'] == (96, 32) and buf.__cuda_array_interface__['strides'] is None
    host = np.arange(5 * 3 * 4, dtype=np.int32).reshape(5, 3, 4)
    assert (BatchedREALRobotEnv.ray_column(host, 0) == host[:, :, 0]).all()
