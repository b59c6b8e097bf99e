"""CPU tests (-m "not gpu") of the whole-batch closest-point queries: the C boundary (header, binding, constants) and the host-side
argument check of `set_distance_pairs`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_set_distance_pairs', 'rr_get_distance_pairs', 'rr_closest_points', 'rr_distance_buffer', 'rr_distance_copy_to_host')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_enum_and_keeps_abi_7():
    h = _header()
    dist = dict((k, int(v)) for k, v in re.findall(r'\b(RR_DIST_[A-Z_]+)\s*=\s*(\d+)', h))
    assert dist == dict(RR_DIST_POINTS=0, RR_DIST_ID=1, RR_DIST_COUNT=2)
    assert int(re.search(r'#define\s+RR_DIST_MAX\s+(\d+)', h).group(1)) == nat.DIST_MAX == 96
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    assert int(re.search(r'\bRR_KIN_COUNT\s*=\s*(\d+)', h).group(1)) == 7 and int(re.search(r'\bRR_EP_COUNT\s*=\s*(\d+)', h).group(1)) == 8
    assert int(re.search(r'\bRR_RAY_COUNT\s*=\s*(\d+)', h).group(1)) == 2
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(\s*rr_env\s*\*\s*env\b' % name, h), name
    doc = h[h.index('Closest points between collision hulls on the device'):h.index('int rr_distance_copy_to_host(')]
    for word in ('getClosestPoints', 'contactNormalOnB', 'STREAM CONTRACT', 'Out of scope', 'VERTEX SET', '0.3 mm', 'PENETRATION DEPTH', 'lowest vertex',
                 'checkpoints do not carry it', 'launches nothing', 'unspecified'):
        assert word in doc, word


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert nat.DIST_FIELDS == ('points', 'id') and nat.DIST_MAX == 96


def test_collision_shapes_name_every_shape():
    rows = BatchedREALRobotEnv.collision_shapes()
    assert [r['index'] for r in rows] == list(range(22)) and len({r['name'] for r in rows}) == 22
    by = {r['name']: r for r in rows}
    assert by['table']['body'] == by['shelf']['body'] == by['robot_base']['body'] == -1 and by['robot_base']['link'] == 0
    assert [by[k]['body'] for k in ('cube', 'tomato', 'mustard')] == [16, 17, 18]
    assert by['finger_01']['link'] == nat.LINK_NAMES.index('finger_01') and 0 <= by['finger_01']['body'] < 11
    assert set(rows[0]) == {'index', 'uid', 'body', 'link', 'name'}


def test_pair_arguments_are_checked_on_the_host():
    """Every argument error is a ValueError raised before the native call: the check is a static method (no handle, no GPU)."""
    arg = BatchedREALRobotEnv._distance_arg
    by = {r['name']: r['index'] for r in BatchedREALRobotEnv.collision_shapes()}
    n, a, b, md = arg([('cube', 'table'), (by['skin_00'], 'tomato'), (np.int32(3), 1)], 0.05)
    assert n == 3 and a.dtype == b.dtype == np.int32 and list(a) == [by['cube'], by['skin_00'], 3] and list(b) == [0, by['tomato'], 1]
    assert md == float(np.float32(0.05)) and a.flags.c_contiguous and b.flags.c_contiguous
    assert arg('collision')[0] == -1 and arg('collision', np.inf)[3] == np.inf and arg([], None)[0] == 0 and arg([(0, 1)], -1.0)[3] == -1.0
    assert arg([(0, 1)] * 96)[0] == 96
    assert arg([('cube', 'table')], n_objects=1)[0] == 1
    for bad in (dict(pairs='all'), dict(pairs=5), dict(pairs=[(0, 1)] * 97), dict(pairs=[(0, 22)]), dict(pairs=[(-1, 0)]), dict(pairs=[(4, 4)]),
                dict(pairs=[('cube', 'cube')]), dict(pairs=[('no_such_shape', 0)]), dict(pairs=[(0, 1, 2)]), dict(pairs=[0, 1]), dict(pairs=['ab']),
                dict(pairs=[(0.5, 1)]), dict(pairs=[(True, 1)]), dict(pairs=[('tomato', 'table')], n_objects=1), dict(pairs=[(0, by['mustard'])], n_objects=2),
                dict(pairs=[(0, 1)], max_distance=float('nan')), dict(pairs=[(0, 1)], max_distance='far'), dict(pairs='collision', max_distance=np.nan)):
        with pytest.raises(ValueError):
            arg(**bad)


def test_strided_device_views_of_the_columns():
    pts, ids = nat.DeviceBuffer(4096, (5, 3, 12), '<f4', None), nat.DeviceBuffer(8192, (5, 3, 4), '<i4', None)
    cols = BatchedREALRobotEnv.distance_columns(pts, ids)
    assert set(cols) == {'distance', 'lower', 'point_a', 'point_b', 'normal', 'status', 'iterations', 'body_a', 'body_b'}
    assert cols['lower'].ptr == 4096 + 4 and cols['lower'].shape == (5, 3) and cols['lower'].strides == (144, 48)
    assert cols['point_b'].ptr == 4096 + 20 and cols['point_b'].shape == (5, 3, 3) and cols['point_b'].strides == (144, 48, 4)
    assert cols['body_b'].ptr == 8192 + 12 and cols['body_b'].strides == (48, 16) and cols['status'].typestr == '<i4'
    hp, hi = np.arange(180, dtype=np.float32).reshape(5, 3, 12), np.arange(60, dtype=np.int32).reshape(5, 3, 4)
    host = BatchedREALRobotEnv.distance_columns(hp, hi)
    assert (host['normal'] == hp[:, :, 8:11]).all() and (host['iterations'] == hi[:, :, 1]).all()
