"""Env forks and snapshot slots without a GPU: rr_snapshot_slots / rr_copy_envs are declared, bound, exported and refuse a NULL
env; the ABI numbers stay; the header says what a record leaves out; the Python layer validates a source index before the library
is called."""
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_both_calls_are_declared_bound_and_exported():
    for name, nargs in (('rr_snapshot_slots', 2), ('rr_copy_envs', 5)):
        m = re.search(r'\bint %s\(([^)]*)\);' % name, HEADER)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert args[0] == 'rr_env *env' and len(args) == nargs
        assert name in nat.SYMBOLS
    L = nat.load_library()
    assert len(L.rr_snapshot_slots.argtypes) == 2 and len(L.rr_copy_envs.argtypes) == 5
    assert L.rr_snapshot_slots(None, 1) == -1
    assert L.rr_copy_envs(None, -1, -1, None, 0) == -1
    assert re.search(r'#define RR_SLOT_LIVE \(-1\)', HEADER) and nat.SLOT_LIVE == -1


def test_abi_numbers_stay():
    assert int(re.search(r'#define RR_ABI_VERSION (\d+)', HEADER).group(1)) == 7 == nat.RR_ABI_VERSION
    assert nat.load_library().rr_abi_version() == 7
    assert int(re.search(r'RR_F_COUNT = (\d+)', HEADER).group(1)) == 16
    assert int(re.search(r'RR_EP_COUNT = (\d+)', HEADER).group(1)) == 8
    assert int(re.search(r'#define RR_NUM_KERNELS (\d+)', HEADER).group(1)) == 9 == nat.NUM_KERNELS


def test_header_names_what_a_record_leaves_out():
    i = HEADER.index('Env forks and snapshot slots')
    lines = HEADER[i:HEADER.index('int rr_copy_envs(', i)].splitlines()
    text = ' '.join(' '.join(re.sub(r'^\s*\*\s', '', line) for line in lines).split())      # (without the comment's line starts)
    for what in ('saveState', 'restoreState', 'NOT part of a record', 'home poses', 'object dynamics', 'pair materials', 'actuators',
                 'cameras', 'appearance', 'settings of the env, not its state', 'episode record', 'rr_set_env_goals',
                 'rr_contact_observations', 'macro plan', 'images', 'fragment lists', 'unspecified', 'bit 8', 'STREAM CONTRACT',
                 'Out of scope', 'two handles'):
        assert what in text, what


class _FakeLib:
    def __init__(self):
        self.calls = []

    def rr_copy_envs(self, h, src_slot, dst_slot, ptr, on_device):
        self.calls.append((src_slot, dst_slot, ptr, on_device))
        return 0


def _fake_env(n=6):
    env = BatchedREALRobotEnv.__new__(BatchedREALRobotEnv)
    env.L, env.h, env.N, env.n_objects = _FakeLib(), None, n, 3
    return env


class _DeviceArray:
    """Something with __cuda_array_interface__ (no device behind it: the Python layer must not touch the memory)."""

    def __init__(self, shape, typestr='<i4', strides=None):
        self.__cuda_array_interface__ = {'shape': shape, 'typestr': typestr, 'data': (0x1000, False), 'version': 2, 'strides': strides}


@pytest.mark.parametrize('idx', [np.zeros(5, np.int32), np.zeros((6, 1), np.int32), np.zeros(6, np.float32), np.zeros(6, bool),
                                 np.array([0, 1, 2, 3, 4, 6]), np.array([0, -2, 2, 3, 4, 5]), [0, 1, 2, 3, 4, 2 ** 40],
                                 _DeviceArray((5,)), _DeviceArray((6,), '<i8'), _DeviceArray((6,), '<f4'),
                                 _DeviceArray((6,), '<i4', (8,))])
@pytest.mark.parametrize('how', ['fork', 'save', 'load', 'copy'])
def test_a_bad_source_index_raises_before_the_library_is_called(idx, how):
    env = _fake_env()
    with pytest.raises(ValueError):
        {'fork': lambda: env.fork(idx), 'save': lambda: env.save_snapshot(0, idx), 'load': lambda: env.load_snapshot(0, idx),
         'copy': lambda: env.copy_envs(idx, 0, 1)}[how]()
    assert env.L.calls == []


def test_slots_and_pointers_reach_the_library():
    env = _fake_env()
    env.fork([1, 0, -1, 5, 5, 5])
    env.save_snapshot(2)
    env.load_snapshot(1, np.full(6, 3, np.int64))
    env.copy_envs(_DeviceArray((6,)), 1, 0)
    c = env.L.calls
    assert c[0][:2] == (-1, -1) and c[0][2] and c[0][3] == 0
    assert c[1] == (-1, 2, None, 0)
    assert c[2][:2] == (1, -1) and c[2][3] == 0
    assert c[3] == (1, 0, 0x1000, 1)
