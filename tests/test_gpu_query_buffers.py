"""The output buffers of the ten query families on a live handle, through the two generic accessors (rr_query.inc) and the family
table of `_native.py`: before any query every buffer exists with the bytes of the layout in force (K = 0) and a host copy of that
size succeeds; after one query of every family at its smallest shape every pointer is the one handed out before, every byte count
is the table's for the new layout, a copy of that size succeeds and one of four bytes less is refused by name.  No values are
checked here: the per-family tests own them.  The CPU side is tests/test_query_layout.py."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

pytestmark = pytest.mark.gpu

N, OBJECTS, K, Q, P, RAYS = 5, 3, 3, 4, 2, 2


def _all_buffers(env, dims):
    """{(family, field): device pointer} after checking, for every buffer of the Python table, a non-null pointer, the table's bytes
    for `dims` (P: per family, the rays for the ray casts) and a host copy of exactly that size."""
    out = {}
    for name, fam in nat.QUERY_FAMILIES.items():
        d = dict(dims, P=dims['R'] if name == 'ray' else dims['P'])
        for which, field in enumerate(fam.fields):
            p, n = C.c_void_p(), C.c_size_t()
            nat.check(getattr(env.L, fam.buffer)(env.h, which, C.byref(p), C.byref(n)))
            assert p.value, (name, field)
            assert n.value == fam.nbytes(which, d), (name, field, n.value, d)
            host = np.empty(max(n.value, 1), np.uint8)
            nat.check(getattr(env.L, fam.copy_to_host)(env.h, which, host.ctypes.data, n.value))
            assert env._query_buffer(fam, field, host=True).shape == fam.shape(which, d), (name, field)
            out[(name, field)] = p.value
    return out


def test_every_buffer_before_and_after_one_query_of_every_family():
    env = BatchedREALRobotEnv(N, objects=OBJECTS, width=32, height=32)
    try:
        # a fresh handle: one kinematic point, no rays, no pairs, no query yet
        before = _all_buffers(env, dict(N=N, O=OBJECTS, K=0, Q=0, P=1, R=0))
        assert len(set(before.values())) == len(before) == sum(len(f.fields) for f in nat.QUERY_FAMILIES.values())

        env.set_kinematic_points([nat.EE_LINK, nat.EE_LINK], [[0, 0, 0], [0, 0, 0.1]])
        env.set_rays(['world', nat.EE_LINK], [[0.0, 0.0, 1.0, 0.0, 0.0, 0.0], [0, 0, 0, 0, 0, 0.2]])
        env.set_distance_pairs([('cube', 'table'), ('tomato', 'table'), ('mustard', 'table'), ('cube', 'tomato')])
        rng = np.random.default_rng(5)
        postures = rng.uniform(-0.5, 0.5, (N, K, nat.N_JOINTS)).astype(np.float32)
        segments = np.ascontiguousarray(np.stack([postures, postures + np.float32(0.05)], 2))
        targets = np.tile(np.array([-0.1, 0.0, 0.9, 0, 0, 0, 1], np.float32), (N, K, 1))
        env.kinematic_observations()
        env.ray_cast()
        env.closest_points()
        env.posture_clearance(postures)
        env.signed_distance(postures)
        env.signed_distance_gradient(postures)
        env.swept_clearance(segments)
        env.posture_kinematics(postures)
        env.posture_ik(targets)
        env.posture_dynamics(postures)

        after = _all_buffers(env, dict(N=N, O=OBJECTS, K=K, Q=Q, P=P, R=RAYS))
        assert after == before                      # no pointer ever changes
        for name, fam in nat.QUERY_FAMILIES.items():
            for which, field in enumerate(fam.fields):
                n = fam.nbytes(which, dict(N=N, O=OBJECTS, K=K, Q=Q, P=RAYS if name == 'ray' else P))
                host = np.empty(n, np.uint8)
                assert getattr(env.L, fam.copy_to_host)(env.h, which, host.ctypes.data, n - 4) == -1, (name, field)
                assert env.L.rr_last_error().decode() == fam.copy_to_host + ': size mismatch'
    finally:
        env.close()
