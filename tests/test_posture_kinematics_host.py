"""Tests of the C boundary of the kinematics at candidate postures (rr_posture_kinematics, include/realrobot.h) that need no GPU: the
header, the enum, the binding and the refusals that need no handle.  The GPU side is tests/test_gpu_posture_kinematics.py."""
import ctypes as C
import os
import re

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_posture_kinematics', 'rr_posture_kinematics_buffer', 'rr_posture_kinematics_copy_to_host')


def test_header_declares_the_enum_and_keeps_abi_7():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    pk = dict((k, int(v)) for k, v in re.findall(r'\b(RR_PK_[A-Z_]+)\s*=\s*(\d+)', h))
    assert pk == dict(RR_PK_LINK_POSE=0, RR_PK_POINT_POS=1, RR_PK_JACOBIAN=2, RR_PK_COUNT=3)
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_KIN_COUNT\s*=\s*(\d+)', h).group(1)) == 7 and int(re.search(r'\bRR_PC_COUNT\s*=\s*(\d+)', h).group(1)) == 4
    assert int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    assert int(re.search(r'#define\s+RR_PC_MAX_POSTURES\s+(\d+)', h).group(1)) == nat.PC_MAX_POSTURES == 32
    assert int(re.search(r'#define\s+RR_KIN_MAX_POINTS\s+(\d+)', h).group(1)) == nat.KIN_MAX_POINTS == 8
    assert re.search(r'\bint\s+rr_posture_kinematics\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*postures\s*(/\*.*?\*/)?\s*,\s*int32_t\s+n_postures\s*,'
                     r'\s*int32_t\s+on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_kinematics_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_posture_kinematics_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    doc = h[h.index('Kinematics at candidate joint postures on the device'):h.index('int rr_posture_kinematics_copy_to_host(')]
    for word in ('rr_kinematic_observations', 'rr_posture_clearance', 'rr_set_kinematic_points', 'NOT validated', 'NOT clamped', 'BIT FOR BIT',
                 'no joint velocity', 'ALONE', 'independent of env e\'s state', 'not an input', 'No effect on the simulation', 'RR_F_PREP',
                 'forms an address', 'unspecified', 'No atomics', 'RR_EINVAL', 'nothing allocated', '85 888', '352 MB', 'pointer ever changes',
                 '0 before the first', 'STREAM CONTRACT', 'Out of scope', 'velocities', 'candidate object poses', 'all 17 links', 'vector env',
                 'ray casts', 'any use by'):
        assert word in doc, word
    # the figure of the header: 32 postures x (17 x 7 + 8 x 3 + 8 x 66) floats per env
    assert nat.PC_MAX_POSTURES * (len(nat.LINK_NAMES) * 7 + nat.KIN_MAX_POINTS * 69) * 4 == 85888


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_posture_kinematics.argtypes) == 4
    assert len(L.rr_posture_kinematics_buffer.argtypes) == 4 and len(L.rr_posture_kinematics_copy_to_host.argtypes) == 4
    assert nat.PK_FIELDS == ('link_pose', 'point_pos', 'jacobian')
    assert all(name in nat.KIN_FIELDS for name in nat.PK_FIELDS)            # the rows of the observations of those names
    # the refusals that need no device: a null env
    assert L.rr_posture_kinematics(None, None, 1, 0) == -1 and 'rr_posture_kinematics: null env' in L.rr_last_error().decode()
    assert L.rr_posture_kinematics_buffer(None, 0, None, None) == -1 and 'rr_posture_kinematics_buffer' in L.rr_last_error().decode()
    assert L.rr_posture_kinematics_copy_to_host(None, 0, None, 0) == -1 and 'rr_posture_kinematics_copy_to_host' in L.rr_last_error().decode()
    for name in ('posture_kinematics', 'posture_kinematics_buffer'):
        assert callable(getattr(BatchedREALRobotEnv, name))
