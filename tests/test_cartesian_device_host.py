"""Tests of the C boundary of the device-resident cartesian actions (rr_step_cartesian, include/realrobot.h) that need no GPU: the
header, the binding, the refusals that need no handle, the Python-side argument checks -- and the conditions on the inputs of the GPU
tests (tests/test_gpu_cartesian_device.py), checked here in float64 with oracle/kinematics.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from oracle.kinematics import ee_residual, ik_candidates, inverse_kinematics
from tests import cartesian_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_step_cartesian', 'rr_cartesian_invalidate', 'rr_cartesian_buffer', 'rr_cartesian_copy_to_host')


def test_header_declares_the_entry_points_and_the_enum():
    h = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'#define\s+RR_NUM_KERNELS\s+(\d+)', h).group(1)) == 9
    assert re.search(r'\bint\s+rr_step_cartesian\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*cartesian\s*(/\*.*?\*/)?\s*,'
                     r'\s*const\s+float\s*\*\s*gripper\s*(/\*.*?\*/)?\s*,\s*const\s+uint8_t\s*\*\s*idle\s*(/\*.*?\*/)?\s*,\s*int32_t\s+on_device\s*,'
                     r'\s*int32_t\s+render_mode\s*,\s*const\s+uint8_t\s*\*\s*render_flags_host\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_cartesian_invalidate\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+uint8_t\s*\*\s*env_mask\s*,\s*int32_t\s+mask_on_device\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_cartesian_buffer\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*bytes\s*\)\s*;', h)
    assert re.search(r'\bint\s+rr_cartesian_copy_to_host\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+bytes\s*\)\s*;', h)
    for k, name in enumerate(('RR_CART_REQUEST', 'RR_CART_SOLUTION', 'RR_CART_RESIDUAL', 'RR_CART_SOLVED', 'RR_CART_COUNT')):
        assert re.search(r'\b%s\s*=\s*%d\b' % (name, k), h), name
    assert (nat.CART_REQUEST, nat.CART_SOLUTION, nat.CART_RESIDUAL, nat.CART_SOLVED) == (0, 1, 2, 3)
    assert nat.CARTESIAN_NAMES == ('request', 'solution', 'residual', 'solved')
    doc = h[h.index('Device-resident cartesian actions'):h.index('int rr_cartesian_copy_to_host(')]
    for word in ('IEEE ==', '-0.0 equals 0.0', 'NaN', 'PRESENT joints', 'RR_SOLVER_IK_SINGLE_SEED', 'zeros(9)', 'last_ik', 'NOT solved again',
                 'WITHOUT a wait', 'not validated', 'mixed set', 'bad render_mode', 'rr_reset', 'rr_write_state', 'rr_copy_envs', 'checkpoint restores',
                 'policy state', 'all or nothing', 'RR_EINVAL', 'gripper[0], gripper[1]', 'maxNumIterations 1000'):
        assert word in doc, word
    # every entry point's text cites the lines of the reference it restates
    for name in NEW:
        at = doc.index('int %s(' % name) if name != NEW[-1] else len(doc)
        assert 'env.py:358-386' in doc[doc.rindex('/*', 0, at):at], name
    # the sentence of rr_posture_ik stays as it was
    assert 'any use by the step (cartesian actions)' in h


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert [len(getattr(L, n).argtypes) for n in NEW] == [7, 3, 4, 4]
    # the refusals that need no device: a null env -- RR_EINVAL with the entry point's name
    assert L.rr_step_cartesian(None, None, None, None, 0, 0, None) == -1 and 'rr_step_cartesian: null env' in L.rr_last_error().decode()
    assert L.rr_cartesian_invalidate(None, None, 0) == -1 and 'rr_cartesian_invalidate: null env' in L.rr_last_error().decode()
    assert L.rr_cartesian_buffer(None, 0, None, None) == -1 and 'rr_cartesian_buffer: bad buffer' in L.rr_last_error().decode()
    buf = (C.c_char * 4)()
    assert L.rr_cartesian_copy_to_host(None, 0, buf, 4) == -1 and 'rr_cartesian_copy_to_host: bad buffer' in L.rr_last_error().decode()
    assert L.rr_cartesian_copy_to_host(None, 0, None, 4) == -1 and 'null destination' in L.rr_last_error().decode()


def test_the_refusals_come_first_and_the_call_never_waits_on_device_arguments():
    """On the source: every refusal stands in front of the first allocation, copy or launch; the launches come in the documented
    order on the main stream, each followed by the error check; the only wait is the staging helper's, which a device caller does
    not take; nothing is read back; the part allocates nothing and reads no environment."""
    src = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_host.inc')).read()
    body = src[src.index('int rr_step_cartesian('):src.index('int rr_cartesian_invalidate(')]
    first_effect = min(body.index(w) for w in ('ensure_cartesian(', 'hipMemcpyAsync', 'hipLaunchKernelGGL', 'st.in('))
    assert body.index('null env') < body.index('null cartesian') < body.index('null gripper') < body.index('bad render_mode') < body.index('same side') < first_effect
    order = [body.index(w) for w in ('st.in(', 'k_cart_decide,', 'k_cart_solve,', 'k_cart_fetch,', 'rr_step(e, e->D.cmd, 1,', 'st.wait()')]
    assert order == sorted(order)
    assert 'hipStreamSynchronize' not in body and 'hipDeviceSynchronize' not in body and 'DeviceToHost' not in body
    assert 'hipStreamCreate' not in body and 'hipEventCreate' not in body
    assert body.count('hipLaunchKernelGGL') == 3 == body.count('HIPCHK(hipGetLastError());')
    assert 'const HostStaging st = {e, !on_device};' in body
    ens = src[src.index('static int ensure_cartesian('):src.index('int rr_step_cartesian(')]
    assert ens.count('ensure_group(') == 1 and 'hipMalloc' not in ens and 'mem_get' not in ens
    ker = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_cart.inc')).read()
    assert 'getenv' not in ker and 'hipMalloc' not in ker
    assert 'atomic' not in ker.replace('No atomics', '')
    # the solver is the existing one, called, not copied
    assert ker.count('ik_dls(') == 1 and ker.count('ik_fk(') == 1 and '__device__' not in ker
    hip = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'realrobot.hip')).read()
    assert hip.index('#include "rr_macro.inc"') < hip.index('#include "rr_cart.inc"') < hip.index('#include "rr_host.inc"')
    # the existing entry points keep their text
    assert 'hipLaunchKernelGGL(k_ik, dim3((N + 63) / 64), dim3(64), 0, e->stream, e->IK, e->P, e->D, e->ik_in, e->ik_out, e->ik_err);' in src


class _FakeDevice:
    """An object that says it is device memory (`__cuda_array_interface__`); never dereferenced: the checks run before the library."""

    def __init__(self, shape, typestr='<f4', strides=None):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x1000, False), version=2, strides=strides)


def test_python_side_arguments_and_refusals_need_no_device():
    N = 5
    args = BatchedREALRobotEnv._cartesian_args
    for c, g in ((np.zeros((N, 7)), np.zeros((N, 2))), (np.zeros((N, 7), np.float32), np.zeros((N, 2), np.int64)), ([[0.0] * 7] * N, [[0, 1]] * N)):
        cp, gp, ip, on_dev, keep = args(N, c, g, None)
        assert on_dev == 0 and ip is None and keep[0].shape == (N, 7) and keep[1].shape == (N, 2)
        assert keep[0].dtype == keep[1].dtype == np.float32 and cp == keep[0].ctypes.data and gp == keep[1].ctypes.data
    idle = np.array([1, 0, 0, 1, 0], np.uint8)
    cp, gp, ip, on_dev, keep = args(N, np.zeros((N, 7)), np.zeros((N, 2)), idle)
    assert on_dev == 0 and ip == keep[2].ctypes.data
    assert args(N, np.zeros((N, 7)), np.zeros((N, 2)), idle.astype(bool))[2] is not None
    assert args(N, _FakeDevice((N, 7)), _FakeDevice((N, 2)), None)[:4] == (0x1000, 0x1000, None, 1)
    view = nat.DeviceBuffer(0x2000, (N, 7), '<f4', None)
    assert args(N, view, _FakeDevice((N, 2)), _FakeDevice((N,), '|u1'))[:4] == (0x2000, 0x1000, 0x1000, 1)
    assert args(N, view, _FakeDevice((N, 2)), _FakeDevice((N,), '|b1'))[:4] == (0x2000, 0x1000, 0x1000, 1)
    ok_c, ok_g = np.zeros((N, 7)), np.zeros((N, 2))
    bad = [
        (np.zeros((N, 6)), ok_g, None),                                          # shape
        (np.zeros((N + 1, 7)), ok_g, None),
        (np.zeros((N, 7, 1)), ok_g, None),
        (np.zeros(7), ok_g, None),
        (ok_c, np.zeros((N, 3)), None),
        (ok_c, np.zeros(2 * N), None),
        (np.zeros((N, 7), complex), ok_g, None),                                 # dtype
        (ok_c, np.array([['a'] * 2] * N), None),
        (ok_c, ok_g, np.zeros(N + 1, np.uint8)),                                 # idle shape
        (ok_c, ok_g, np.zeros(N, np.float32)),                                   # idle dtype
        (_FakeDevice((N, 7), '<f8'), _FakeDevice((N, 2)), None),                 # a device tensor must be float32
        (_FakeDevice((N, 7)), _FakeDevice((N, 2), '<f2'), None),
        (_FakeDevice((N, 6)), _FakeDevice((N, 2)), None),
        (_FakeDevice((N, 7)), _FakeDevice((2,)), None),
        (_FakeDevice((N, 7), '<f4', (32, 4)), _FakeDevice((N, 2)), None),        # not compact
        (_FakeDevice((N, 7)), _FakeDevice((N, 2), '<f4', (16, 4)), None),
        (_FakeDevice((N, 7)), _FakeDevice((N, 2)), _FakeDevice((N,), '<i4')),    # idle dtype on the device
        (_FakeDevice((N, 7)), ok_g, None),                                       # mixed sides
        (ok_c, _FakeDevice((N, 2)), None),
        (_FakeDevice((N, 7)), _FakeDevice((N, 2)), idle),
        (ok_c, ok_g, _FakeDevice((N,), '|u1')),
    ]
    for c, g, i in bad:
        with pytest.raises(ValueError):
            args(N, c, g, i)
    for c, g, i in bad[-4:]:
        with pytest.raises(ValueError, match='same side'):
            args(N, c, g, i)
    # step_cartesian_device raises them before it touches the library: an object without a handle is enough
    ghost = object.__new__(BatchedREALRobotEnv)
    ghost.N, ghost.h, ghost.L = N, None, None
    for c, g, i in bad:
        with pytest.raises(ValueError):
            ghost.step_cartesian_device(c, g, idle=i)
    with pytest.raises(ValueError, match='render flags'):
        ghost.step_cartesian_device(ok_c, ok_g, render=np.zeros(N + 1, np.uint8))
    with pytest.raises(ValueError, match='unknown cartesian buffer'):
        ghost.cartesian_buffer('solutions')
    with pytest.raises(ValueError, match='unknown cartesian buffer'):
        ghost.cartesian_buffer(4)
    with pytest.raises(ValueError, match='unknown cartesian buffer'):
        ghost.cartesian_buffer(True)
    with pytest.raises(ValueError):
        ghost.cartesian_invalidate(np.zeros(N + 1, np.uint8))


def test_signatures_and_the_methods_that_stay():
    assert list(inspect.signature(BatchedREALRobotEnv.step_cartesian_device).parameters)[1:] == ['cartesian_commands', 'gripper_commands', 'idle', 'render']
    assert inspect.signature(BatchedREALRobotEnv.step_cartesian_device).parameters['idle'].default is None
    assert inspect.signature(BatchedREALRobotEnv.step_cartesian_device).parameters['render'].default is False
    assert list(inspect.signature(BatchedREALRobotEnv.cartesian_invalidate).parameters)[1:] == ['env_mask']
    assert inspect.signature(BatchedREALRobotEnv.cartesian_invalidate).parameters['env_mask'].default is None
    assert list(inspect.signature(BatchedREALRobotEnv.cartesian_buffer).parameters)[1:] == ['name', 'host']
    assert inspect.signature(BatchedREALRobotEnv.cartesian_buffer).parameters['host'].default is False
    # ik() and the macro paths are not rerouted
    text = inspect.getsource(BatchedREALRobotEnv.ik)
    assert 'rr_ik(' in text and 'cartesian' not in text
    assert 'rr_step_cartesian' not in inspect.getsource(BatchedREALRobotEnv.step_macro_device)


def test_input_conditions_of_the_gpu_tests():
    """The conditions on the inputs of tests/test_gpu_cartesian_device.py, in float64: every target of the fixed seeds is the forward
    kinematics of a posture within +-0.3 rad of the env's scattered posture; inverse_kinematics converges for every row; at most 5 % of
    the rows have float64 candidates whose elbow heights differ by less than IK_TOL -- the only rows the float64 branch check of the GPU
    test may exempt (it recomputes this set by the same rule)."""
    q0 = ci.postures()
    near, t = ci.separated_targets()
    assert q0.shape == (ci.N, 7) and t.shape == (ci.N, 7) and t.dtype == np.float32 and np.isfinite(t).all()
    assert np.abs(near - q0).max() <= ci.NEAR and np.abs(near - q0).max() > 0.9 * ci.NEAR
    assert np.abs(np.linalg.norm(t[:, 3:], axis=1) - 1).max() < 1e-6
    close = 0
    for i in range(ci.N):
        q11 = np.zeros(11)
        q11[:7] = near[i]
        assert ee_residual(q11, t[i, :3].astype(np.float64), t[i, 3:].astype(np.float64)) < 1e-6, i       # (the float32 rounding of the pose)
        q11[:7] = q0[i]
        pos, quat = t[i, :3].astype(np.float64), t[i, 3:].astype(np.float64)
        best = inverse_kinematics(q11, pos, quat)
        assert ee_residual(best, pos, quat) < 1e-3, i
        cands = ik_candidates(q11, pos, quat)
        assert len(cands) == 2
        close += abs(cands[0][2] - cands[1][2]) < ci.IK_TOL
    assert close <= 0.05 * ci.N, close
    # the larger handles of the bit-for-bit test have the same first 67 postures; their targets are single draws (no float64 check there)
    assert np.array_equal(ci.postures(200)[:ci.N], q0)
    big = ci.targets(200)
    assert big.dtype == np.float32 and np.isfinite(big).all() and np.abs(ci.near_postures(200) - ci.postures(200)).max() <= ci.NEAR
