"""Tests of the C boundary of the swept clearance (rr_swept_clearance, include/realrobot.h).  Without a GPU (-m "not gpu"): the header,
the enum, the binding, the refusals that need no handle and the host-side argument check.  With one (marked gpu): every RR_EINVAL of
the header with nothing changed, and the buffers' pointers and sizes before and after a query."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_swept_clearance', 'rr_sweep_reach', 'rr_sweep_buffer', 'rr_sweep_copy_to_host')


def test_header_declares_the_enum_and_keeps_abi_7():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    sw = dict((k, int(v)) for k, v in re.findall(r'\b(RR_SW_[A-Z]+)\s*=\s*(\d+)', h))
    assert sw == dict(RR_SW_STOP=0, RR_SW_HIT=1, RR_SW_ID=2, RR_SW_FREE=3, RR_SW_COUNT=4)
    assert int(re.search(r'#define\s+RR_SW_MAX_STEPS\s+(\d+)', h).group(1)) == nat.SW_MAX_STEPS == 64
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_PC_COUNT\s*=\s*(\d+)', h).group(1)) == 4 and int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    assert re.search(r'\bint\s+rr_swept_clearance\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*segments\s*(/\*.*?\*/)?\s*,\s*int32_t\s+n_segments\s*,'
                     r'\s*int32_t\s+on_device\s*,\s*float\s+safety\s*,\s*float\s+tolerance\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_sweep_reach\s*\(\s*rr_env\s*\*\s*env\s*,\s*float\s*\*\s*out\s*(/\*.*?\*/)?\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_sweep_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_sweep_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    doc = h[h.index('Swept clearance along joint-space segments on the device'):h.index('int rr_sweep_copy_to_host(')]
    for word in ('CONSERVATIVE ADVANCEMENT', 'reach table', 'rounded UP', 'Lipschitz', 'RR_SW_MAX_STEPS', 'Guarantees', 'STREAM CONTRACT', 'Out of scope',
                 'pointer ever changes', 'No atomics', 'fake a hit', 'lowest pair index', 'unspecified'):
        assert word in doc, word


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_swept_clearance.argtypes) == 6 and len(L.rr_sweep_reach.argtypes) == 2
    assert len(L.rr_sweep_buffer.argtypes) == 4 and len(L.rr_sweep_copy_to_host.argtypes) == 4
    assert nat.SW_FIELDS == ('stop', 'hit', 'id', 'free')
    # the refusals that need no device: a null env
    assert L.rr_swept_clearance(None, None, 1, 0, 0.0, 1e-3) == -1 and 'rr_swept_clearance: null env' in L.rr_last_error().decode()
    assert L.rr_sweep_buffer(None, 0, None, None) == -1 and 'rr_sweep_buffer' in L.rr_last_error().decode()
    assert L.rr_sweep_reach(None, None) == -1 and 'rr_sweep_reach' in L.rr_last_error().decode()
    assert L.rr_sweep_copy_to_host(None, 0, None, 0) == -1 and 'rr_sweep_copy_to_host' in L.rr_last_error().decode()
    for name in ('swept_clearance', 'sweep_buffer', 'sweep_reach'):
        assert callable(getattr(BatchedREALRobotEnv, name))


def test_segment_argument_is_checked_on_the_host():
    """Every argument error is a ValueError raised before the native call: the check is a static method (no handle, no GPU)."""
    arg = BatchedREALRobotEnv._segment_arg
    good = np.zeros((5, 3, 2, 11), np.float32)
    assert arg(good, 5) == 3 and arg(np.zeros((1, 1, 2, 11), np.float32), 1) == 1 and arg(np.zeros((2, 32, 2, 11), np.float32), 2) == 32

    class Cai:
        def __init__(self, shape, typestr='<f4', strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(4096, False), version=2, strides=strides)
    assert arg(Cai((5, 4, 2, 11)), 5) == 4 and arg(Cai((5, 4, 2, 11), strides=(352, 88, 44, 4)), 5) == 4
    for bad, n in ((np.zeros((5, 0, 2, 11), np.float32), 5), (np.zeros((5, 33, 2, 11), np.float32), 5), (np.zeros((5, 3, 2, 9), np.float32), 5),
                   (np.zeros((5, 3, 1, 11), np.float32), 5), (np.zeros((5, 3, 11), np.float32), 5), (np.zeros((5, 3, 2, 11), np.float64), 5),
                   (np.zeros((5, 3, 2, 22), np.float32)[..., ::2], 5), (good, 4), (None, 5), ('segments', 5), (Cai((5, 4, 2, 11), '<f8'), 5),
                   (Cai((5, 4, 2, 11), strides=(704, 176, 88, 8)), 5)):
        with pytest.raises(ValueError):
            arg(bad, n)


def _buffers(env):
    out = []
    for w in range(4):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_sweep_buffer(env.h, w, C.byref(p), C.byref(n)))
        out.append((p.value, n.value))
    return out


@pytest.mark.gpu
def test_refusals_and_buffer_sizes():
    import torch
    from tests import numpy_distance as nd
    N = 5
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    L = env.L
    good = np.ascontiguousarray(nd.states(N * 4, 131)[:, :11].reshape(N, 2, 2, 11))
    call = lambda ptr, k, s, t: L.rr_swept_clearance(env.h, ptr, k, 0, s, t)
    # an empty pair table is refused, by the library and by the binding
    assert call(good.ctypes.data, 2, 0.0, 1e-3) == -1 and 'pair table is empty' in L.rr_last_error().decode()
    with pytest.raises(ValueError):
        env.swept_clearance(good)
    before = _buffers(env)
    assert [n for _, n in before] == [0, 0, 0, 0] and all(p for p, _ in before) and len({p for p, _ in before}) == 4
    n = nd.names()
    p3 = np.array([(n['skin_00'], n['cube']), (n['finger_01'], n['finger_11']), (n['tomato'], n['table'])], np.int32)
    env.set_distance_pairs(p3)
    assert [x for _, x in _buffers(env)] == [0, 0, 0, 0]                                             # before the first query K counts as 0
    for w, name in enumerate(nat.SW_FIELDS):
        assert env.sweep_buffer(name, host=True).shape[:2] == (N, 0) and env.sweep_buffer(w).shape[:2] == (N, 0)
    whole = (N * 32 * 12, N * 32 * 12, N * 32 * 4, N * 32 * nat.DIST_MAX)
    env.sync()
    for (p, _), count in zip(before, whole):                                                        # zero-filled over the whole allocation
        assert not torch.from_dlpack(nat.DeviceBuffer(p, (count,), '<i4', env)).any().item()
    env.state = nd.states(N, 132)
    env.swept_clearance(good, 0.01, 1e-3)
    first = [env.sweep_buffer(w, host=True).tobytes() for w in range(4)]
    sizes = [N * 2 * 48, N * 2 * 48, N * 2 * 16, N * 2 * 3 * 4]
    assert [x for _, x in _buffers(env)] == sizes
    # refused calls: RR_EINVAL (-1), the cause named, pointers, sizes and contents unchanged
    nan, inf = float('nan'), float('inf')
    for args, word in (((None, 2, 0.0, 1e-3), 'null segments'), ((good.ctypes.data, 0, 0.0, 1e-3), 'n_segments 0'), ((good.ctypes.data, 33, 0.0, 1e-3), 'n_segments 33'),
                       ((good.ctypes.data, 2, -1e-3, 1e-3), 'safety'), ((good.ctypes.data, 2, nan, 1e-3), 'safety'), ((good.ctypes.data, 2, inf, 1e-3), 'safety'),
                       ((good.ctypes.data, 2, 0.0, 5e-7), 'tolerance'), ((good.ctypes.data, 2, 0.0, nan), 'tolerance'), ((good.ctypes.data, 2, 0.0, 0.0), 'tolerance')):
        assert call(*args) == -1, word
        msg = L.rr_last_error().decode()
        assert 'rr_swept_clearance' in msg and word in msg, msg
    assert [env.sweep_buffer(w, host=True).tobytes() for w in range(4)] == first and [x for _, x in _buffers(env)] == sizes
    env.set_distance_pairs(p3, 0.05)                                                                # a cull below safety + tolerance
    assert call(good.ctypes.data, 2, 0.05, 1e-3) == -1 and 'max_distance' in L.rr_last_error().decode()
    with pytest.raises(nat.NativeError):
        env.swept_clearance(good, safety=0.06)
    assert call(good.ctypes.data, 2, 0.04, 1e-3) == 0                                               # ... and one above is served
    env.set_distance_pairs(p3)
    assert call(good.ctypes.data, 2, 0.01, 1e-3) == 0
    assert [env.sweep_buffer(w, host=True).tobytes() for w in range(4)] == first
    p, x = C.c_void_p(), C.c_size_t()
    for which in (4, -1):
        assert L.rr_sweep_buffer(env.h, which, C.byref(p), C.byref(x)) == -1 and 'rr_sweep_buffer' in L.rr_last_error().decode()
    scratch = np.zeros(4, np.float32)
    assert L.rr_sweep_copy_to_host(env.h, 0, scratch.ctypes.data, 4) == -1 and 'size mismatch' in L.rr_last_error().decode()
    assert L.rr_sweep_reach(env.h, None) == -1 and 'rr_sweep_reach' in L.rr_last_error().decode()
    for bad in (good[:, :, :, :9], good.astype(np.float64), np.zeros((N, 33, 2, 11), np.float32), good[:4]):
        with pytest.raises(ValueError):
            env.swept_clearance(bad)
    with pytest.raises(ValueError):
        env.sweep_buffer('points')
    assert _buffers(env) == list(zip([p for p, _ in before], sizes))
    # pointers stay across K and Q; the sizes follow
    k5 = np.ascontiguousarray(nd.states(N * 10, 133)[:, :11].reshape(N, 5, 2, 11))
    env.set_distance_pairs('collision')
    out = env.swept_clearance(k5, 0.0, 1e-3, host=True)
    assert out['pair_free_until'].shape == (N, 5, 92) and out['q_stop'].shape == (N, 5, 11) and out['status'].shape == (N, 5)
    assert _buffers(env) == list(zip([p for p, _ in before], [N * 5 * 48, N * 5 * 48, N * 5 * 16, N * 5 * 92 * 4]))
    assert env.sweep_reach().shape == (11, len(env.collision_shapes()))
    env.set_distance_pairs([])
    assert call(good.ctypes.data, 2, 0.0, 1e-3) == -1 and [p for p, _ in _buffers(env)] == [p for p, _ in before]
    env.close()
