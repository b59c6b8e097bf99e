"""CPU tests (-m "not gpu") of the signed-distance gradient query: the C boundary (header, binding, constants), the refusals that need
no device and the strided views of the gradient rows."""
import ctypes as C
import os
import re

import numpy as np

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_signed_gradient', 'rr_signed_gradient_buffer', 'rr_signed_gradient_copy_to_host')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_enum_and_keeps_abi_7():
    h = _header()
    sg = dict((k, int(v)) for k, v in re.findall(r'\b(RR_SG_[A-Z_]+)\s*=\s*(\d+)', h))
    assert sg == dict(RR_SG_GRADIENT=0, RR_SG_COST=1, RR_SG_PAIR_GRADIENT=2, RR_SG_COUNT=3)
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_SD_COUNT\s*=\s*(\d+)', h).group(1)) == 5 and int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    assert re.search(r'\bint\s+rr_signed_gradient\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*postures\s*(/\*.*?\*/)?\s*,\s*int32_t\s+n_postures\s*,'
                     r'\s*int32_t\s+on_device\s*,\s*float\s+margin\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_signed_gradient_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_signed_gradient_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    doc = h[h.index('Joint gradients of the signed distance on the device'):h.index('int rr_signed_gradient_copy_to_host(')]
    for word in ('Out of scope', 'STREAM CONTRACT', 'unspecified', 'generalised gradient', 'Summation order', 'No atomics', 'pointer ever changes',
                 'PRESENT-STATE', 'Q_FROM_CMD', 'byte for byte', 'max_distance', 'NaN', 'second derivatives', 'object poses', '+0.0', 'permuted table'):
        assert word in doc, word
    # the siblings point here, and keep the word their own tests look for
    pc = h[h.index('Clearance at candidate joint postures on the device'):h.index('int rr_posture_copy_to_host(')]
    sd = h[h.index('Signed distance and penetration depth on the device'):h.index('int rr_signed_copy_to_host(')]
    for block in (pc, sd):
        scope = block[block.index('Out of scope'):]
        assert 'gradients' in scope and 'rr_signed_gradient' in scope


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_signed_gradient.argtypes) == 5 and L.rr_signed_gradient.argtypes[4] is C.c_float
    assert nat.SG_FIELDS == ('gradient', 'cost', 'pair_gradient')
    assert nat.SD_FIELDS == ('deepest', 'id', 'signed', 'status', 'points')
    # the refusals that need no device: a null env
    assert L.rr_signed_gradient(None, None, 0, 0, 0.0) == -1 and 'rr_signed_gradient: null env' in L.rr_last_error().decode()
    assert L.rr_signed_gradient_buffer(None, 0, None, None) == -1 and 'rr_signed_gradient_buffer: null env' in L.rr_last_error().decode()
    buf = np.zeros(4, np.float32)
    assert L.rr_signed_gradient_copy_to_host(None, 0, buf.ctypes.data, 16) == -1 and 'rr_signed_gradient_copy_to_host: null env' in L.rr_last_error().decode()
    assert hasattr(BatchedREALRobotEnv, 'signed_distance_gradient') and hasattr(BatchedREALRobotEnv, 'signed_gradient_buffer')
    assert 'Q_FROM_CMD' in BatchedREALRobotEnv.signed_distance_gradient.__doc__


def test_strided_views_of_the_gradient_rows():
    buf = nat.DeviceBuffer(4096, (5, 3, 12), '<f4', None)
    g, last = BatchedREALRobotEnv._gradient_views(buf, False)
    assert g.ptr == 4096 and g.shape == (5, 3, 11) and g.strides == (3 * 48, 48, 4) and g.typestr == '<f4'
    assert last.ptr == 4096 + 44 and last.shape == (5, 3) and last.strides == (3 * 48, 48)
    one = nat.DeviceBuffer(8192, (5, 1, 12), '<f4', None)
    g, last = BatchedREALRobotEnv._gradient_views(one, True)
    assert g.ptr == 8192 and g.shape == (5, 11) and g.strides == (48, 4) and last.ptr == 8192 + 44 and last.shape == (5,) and last.strides == (48,)
    host = np.arange(5 * 3 * 12, dtype=np.float32).reshape(5, 3, 12)
    g, last = BatchedREALRobotEnv._gradient_views(host, False)
    assert g.shape == (5, 3, 11) and last.shape == (5, 3) and np.shares_memory(g, host) and (last == host[:, :, 11]).all() and (g == host[:, :, :11]).all()
    g, last = BatchedREALRobotEnv._gradient_views(host[:, :1], True)
    assert g.shape == (5, 11) and last.shape == (5,) and (g == host[:, 0, :11]).all() and (last == host[:, 0, 11]).all()
