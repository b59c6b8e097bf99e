"""Device-side state writes and reads without a GPU: rr_write_state / rr_read_state are declared, bound, exported and refuse a NULL
env; the ABI numbers stay; the header states the contract; the Python layer builds the parts word and the on_device flag and refuses
a bad argument before the library is called."""
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_both_calls_are_declared_bound_and_exported():
    for name, nargs in (('rr_write_state', 5), ('rr_read_state', 1)):
        m = re.search(r'\bint %s\(([^)]*)\);' % name, HEADER)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[0] == 'rr_env *env' and len(args) == nargs
        assert name in nat.SYMBOLS
    L = nat.load_library()
    assert len(L.rr_write_state.argtypes) == 5 and len(L.rr_read_state.argtypes) == 1
    assert L.rr_write_state(None, None, None, nat.W_RESET, 0) == -1
    assert L.rr_read_state(None) == -1
    for name, bit in (('JOINT_POS', 1), ('JOINT_VEL', 2), ('OBJ_POSE', 4), ('OBJ_VEL', 8), ('RESET', 16), ('FRESH', 32)):
        assert int(re.search(r'#define RR_W_%s\s+(\d+)' % name, HEADER).group(1)) == bit == getattr(nat, 'W_' + name)
    assert nat.W_COLUMNS == 15


def test_abi_numbers_stay():
    assert int(re.search(r'#define RR_ABI_VERSION (\d+)', HEADER).group(1)) == 7 == nat.RR_ABI_VERSION
    assert nat.load_library().rr_abi_version() == 7
    assert int(re.search(r'RR_F_COUNT = (\d+)', HEADER).group(1)) == 16
    assert int(re.search(r'RR_EP_COUNT = (\d+)', HEADER).group(1)) == 8
    assert int(re.search(r'#define RR_NUM_KERNELS (\d+)', HEADER).group(1)) == 9 == nat.NUM_KERNELS


def test_header_states_the_contract():
    i = HEADER.index('State writes and reads on the device')
    lines = HEADER[i:HEADER.index('int rr_read_state(', i)].splitlines()
    text = ' '.join(' '.join(re.sub(r'^\s*\*\s', '', line) for line in lines).split())      # (without the comment's line starts)
    for what in ('Equivalences, each bit for bit', 'rr_reset(mask)', 'rr_set_object_poses(poses, mask)', 'rr_set_state',
                 'auto-reset of rr_episode_update', 'STREAM CONTRACT', 'KEPT', 'contact history of the warm start', 'RR_F_TIMESTEP',
                 'error flags', 'touch sensors', 'motor-target rows', 'stays frozen unless RR_W_FRESH', 'STAGING AREA', 'rr_evaluate_goals',
                 'overwrite it', 'steps do not refresh it', 'never used', 'not validated', 'parts == 0', 'rr_set_env_goals',
                 'Out of scope', 'snapshot slots', 'indexed form'):
        assert what in text, what


class _FakeLib:
    def __init__(self):
        self.calls = []

    def rr_write_state(self, h, state, mask, parts, on_device):
        self.calls.append(('write', state, mask, parts, on_device))
        return 0

    def rr_reset(self, h, mask):
        self.calls.append(('reset', mask))
        return 0


def _fake_env(n=6):
    env = BatchedREALRobotEnv.__new__(BatchedREALRobotEnv)
    env.L, env.h, env.N, env.n_objects = _FakeLib(), None, n, 3
    return env


class _DeviceArray:
    """Something with __cuda_array_interface__ (no device behind it: the Python layer must not touch the memory)."""

    def __init__(self, shape, typestr='<f4', strides=None, ptr=0x1000):
        self.__cuda_array_interface__ = {'shape': shape, 'typestr': typestr, 'data': (ptr, False), 'version': 2, 'strides': strides}


def test_parts_and_side_reach_the_library():
    env = _fake_env()
    s, m = np.zeros((6, 61), np.float32), np.ones(6, np.uint8)
    ds, dm, db = _DeviceArray((6, 61)), _DeviceArray((6,), '|u1', None, 0x2000), _DeviceArray((6,), '|b1', (1,), 0x3000)
    env.write_state(s, joint_pos=True)
    env.write_state(s, m, joint_vel=True, obj_vel=True)
    env.write_state(ds, dm, obj_pose=True, reset=True)
    env.write_state(_DeviceArray((6, 61), '<f4', (244, 4)), db, joint_pos=True, joint_vel=True, obj_pose=True, obj_vel=True, fresh=True)
    env.write_state(None, m.astype(bool), reset=True)
    env.write_state(None, dm, fresh=True)
    env.write_state(None, None, reset=True, fresh=True)
    env.reset(dm)
    env.reset(m)
    c = env.L.calls
    assert c[0] == ('write', s.ctypes.data, None, 1, 0)
    assert c[1] == ('write', s.ctypes.data, m.ctypes.data, 2 | 8, 0)
    assert c[2] == ('write', 0x1000, 0x2000, 4 | 16, 1)
    assert c[3] == ('write', 0x1000, 0x3000, 15 | 32, 1)
    assert c[4][1] is None and c[4][2] and c[4][3:] == (16, 0)
    assert c[5] == ('write', None, 0x2000, 32, 1)
    assert c[6] == ('write', None, None, 48, 0)
    assert c[7] == ('write', None, 0x2000, 16, 1)            # reset with a device mask: no host round trip
    assert c[8][0] == 'reset' and c[8][1]                    # a host mask keeps going through rr_reset


_S = np.zeros((6, 61), np.float32)
_M = np.ones(6, np.uint8)


@pytest.mark.parametrize('state, mask, flags, word', [
    (_S.astype(np.float64), None, {'joint_pos': True}, 'state'),                            # dtype
    (_DeviceArray((6, 61), '<f8'), None, {'joint_pos': True}, 'state'),
    (_DeviceArray((6, 61), '<f2'), None, {'joint_pos': True}, 'state'),
    (_S, _M.astype(np.int32), {'joint_pos': True}, 'env_mask'),
    (_S, _M.astype(np.float32), {'joint_pos': True}, 'env_mask'),
    (_DeviceArray((6, 61)), _DeviceArray((6,), '<i4'), {'obj_pose': True}, 'env_mask'),
    (np.zeros((6, 60), np.float32), None, {'joint_pos': True}, 'state'),                      # shape
    (np.zeros((5, 61), np.float32), None, {'joint_pos': True}, 'state'),
    (np.zeros(6 * 61, np.float32), None, {'joint_pos': True}, 'state'),
    (_DeviceArray((61, 6)), None, {'joint_pos': True}, 'state'),
    (_S, np.ones(5, np.uint8), {'joint_pos': True}, 'env_mask'),
    (_S, np.ones((6, 1), np.uint8), {'joint_pos': True}, 'env_mask'),
    (None, _DeviceArray((7,), '|u1'), {'reset': True}, 'env_mask'),
    (np.zeros((6, 122), np.float32)[:, ::2], None, {'joint_pos': True}, 'state'),             # contiguity
    (np.zeros((61, 6), np.float32).T, None, {'joint_pos': True}, 'state'),
    (_DeviceArray((6, 61), '<f4', (488, 4)), None, {'joint_pos': True}, 'state'),
    (_S, np.ones(12, np.uint8)[::2], {'joint_pos': True}, 'env_mask'),
    (None, _DeviceArray((6,), '|u1', (2,)), {'reset': True}, 'env_mask'),
    (_DeviceArray((6, 61)), _M, {'obj_vel': True}, 'same side'),                              # a host mask with a device state
    (_S, _DeviceArray((6,), '|u1'), {'obj_vel': True}, 'same side'),
    (None, None, {'joint_pos': True}, 'state'),                                               # column flags without a state
    (None, _M, {'obj_pose': True, 'reset': True}, 'state'),
    (_S, None, {}, 'none of'),                                                                # nothing to do
    (_S, None, {'reset': True}, 'state'),                                                     # a state nobody reads
])
def test_a_bad_argument_raises_before_the_library_is_called(state, mask, flags, word):
    env = _fake_env()
    with pytest.raises(ValueError) as ei:
        env.write_state(state, mask, **flags)
    assert word in str(ei.value), str(ei.value)
    assert env.L.calls == []
