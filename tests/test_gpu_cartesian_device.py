"""GPU tests (-m gpu) of the device-resident cartesian actions (rr_step_cartesian, include/realrobot.h): the decision of
REALRobotEnv.step_cartesian (env.py:358-386) taken on the device, and the solver over the compact list of needing envs (k_cart_solve),
whose joints and residuals must be k_ik's bit for bit.  N = 67 is neither a multiple of 64 nor of the 32 slots of a solver wave.  The
conditions on the inputs (tests/cartesian_inputs.py) are checked on the CPU by tests/test_cartesian_device_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from oracle.kinematics import ee_residual, ik_candidates
from tests import cartesian_inputs as ci

pytestmark = pytest.mark.gpu
N = ci.N
IK_TOL = ci.IK_TOL
BUFFERS = ('request', 'solution', 'residual', 'solved')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')
    torch.cuda.synchronize()
    return t


def make(n=N, **kw):
    return BatchedREALRobotEnv(n, objects=3, width=64, height=64, **kw)


def scatter_postures(env, seed=ci.POSTURE_SEED):
    """Every env at a posture of its own (and at rest), as in tests/test_gpu_macro_device.py: the solutions depend on the present joints."""
    s = env.state
    s[:, :7] = ci.postures(env.N, seed)
    s[:, 7:22] = 0.0
    env.write_state(s, joint_pos=True, joint_vel=True)


def buffers(env, names=BUFFERS):
    return {k: env.cartesian_buffer(k, host=True) for k in names}


def redraw(rng, n):
    """n targets of the construction of cartesian_inputs.targets (the pose of a posture near a scattered one), other draws"""
    return ci.targets(N, seed=int(rng.integers(1 << 30)))[rng.choice(N, n, replace=False)]


@pytest.mark.parametrize('n,single', [(N, False), (N, True), (1100, False), (4099, False)])
def test_solver_equals_k_ik_bit_for_bit(n, single):
    """k_ik and k_cart_solve on ONE handle from one state (rr_ik writes nothing): joints and residuals bit for bit.  67 envs: a wave per
    listed env; 1100 and 4099: more listed envs than the solver gives a wave each -- two and five envs share a wave, the last wave
    is not full."""
    env = make(n, solver={'ik_single_seed': single})
    scatter_postures(env)
    t = ci.separated_targets()[1] if n == N else ci.targets(n)
    before = env.state
    q, err = env.ik(t)
    assert same_bits(env.state, before)
    assert np.isfinite(q).all() and (err < 1e-2).mean() > 0.9
    env.step_cartesian_device(dev(t), dev(ci.grippers(np.random.default_rng(1), n)))
    got = buffers(env)
    assert got['solved'].all()
    bad = np.flatnonzero((bits(got['solution']) != bits(np.ascontiguousarray(q[:, :7]))).any(axis=1) | (bits(got['residual']) != bits(err)))
    assert not bad.size, (bad[:10], [float(np.abs(got['solution'][i] - q[i, :7]).max()) for i in bad[:5]])
    assert same_bits(got['request'], t)
    if not single and n == N:      # the selection acts: both seeds win somewhere (what a planted `last seed wins` or `>=` would change)
        one = make(n, solver={'ik_single_seed': True})
        scatter_postures(one)
        q1 = one.ik(t)[0]
        first = (bits(np.ascontiguousarray(q1[:, :7])) == bits(got['solution'])).all(axis=1)
        assert 0.05 * n < first.sum() < 0.95 * n, first.sum()
        one.close()
    env.close()


def test_a_list_shorter_than_a_wave():
    """5 of 67 envs need a solve: the others keep the bytes of their solution, the five get k_ik's from their present joints."""
    env = make()
    scatter_postures(env)
    t = ci.separated_targets()[1].copy()
    g = dev(ci.grippers(np.random.default_rng(2)))
    env.step_cartesian_device(dev(t), g)
    first = buffers(env)
    pick = np.array([0, 13, 31, 32, 66])
    t[pick] = redraw(np.random.default_rng(3), len(pick))
    q, err = env.ik(t)
    env.step_cartesian_device(dev(t), g)
    got = buffers(env)
    need = np.zeros(N, np.uint8)
    need[pick] = 1
    assert np.array_equal(got['solved'], need)
    assert same_bits(got['solution'][pick], np.ascontiguousarray(q[pick, :7])) and same_bits(got['residual'][pick], err[pick])
    rest = need == 0
    assert same_bits(got['solution'][rest], first['solution'][rest]) and same_bits(got['residual'][rest], first['residual'][rest])
    assert same_bits(got['request'], t)
    env.close()


def programme():
    """The 40 steps of the twin run: per step (targets [N, 7], gripper [N, 2], idle bool [N])."""
    rng = np.random.default_rng(2)
    t = ci.separated_targets()[1].copy()
    z, u, w = 3, 4, 6                 # z: a component goes 0.0 -> -0.0 at step 4 (no solve); u: never changes; w: a NaN component from step 10 on
    t[z, 1] = 0.0
    others = np.array([i for i in range(N) if i not in (z, u, w)])
    out = []
    for s in range(40):
        if s in (3, 7):
            pick = rng.choice(others, N // 3, replace=False)
            t[pick] = redraw(rng, len(pick))
        if s == 4:
            t[z, 1] = -0.0
        if s == 10:
            t[w, 5] = np.nan
        idle = (rng.random(N) < 0.3) if 5 <= s <= 9 else np.zeros(N, bool)
        idle[[u, w]] = False
        out.append((t.copy(), ci.grippers(rng), idle))
    return out, (z, u, w)


def host_step(env, rec, t, g, idle):
    """One step of the host loop on a numpy record: need -> ik() -> the needing rows -> step(cmd).  rec: dict request / solution / residual."""
    need = ~idle & ~np.all(t == rec['request'], axis=1)
    if need.any():
        q, err = env.ik(t)
        rec['solution'][need], rec['residual'][need], rec['request'][need] = q[need, :7], err[need], t[need]
    cmd = np.concatenate([rec['solution'], g], axis=1).astype(np.float32)
    cmd[idle] = 0.0
    up = dev(cmd)       # (as a device buffer: step() refuses a non-finite host command, which rr_step leaves to the solve -- the NaN env's row)
    env.step(device_ptr=up.data_ptr())
    env.sync()
    return need


@pytest.fixture(scope='module')
def twin_run():
    """Handle A: the host loop; handle B: step_cartesian_device with CUDA tensors; handle Cn: the same programme through numpy arrays.
    Everything the tests compare is recorded per step."""
    steps, marks = programme()
    A, B, Cn = make(), make(), make()
    for e in (A, B, Cn):
        scatter_postures(e)
    rec = dict(request=np.full((N, 7), np.nan, np.float32), solution=np.zeros((N, 7), np.float32), residual=np.zeros(N, np.float32))
    log, keep = [], []
    for s, (t, g, idle) in enumerate(steps):
        need = host_step(A, rec, t, g, idle)
        args = (dev(t), dev(g), dev(idle) if idle.any() else None)
        keep.append(args)
        B.step_cartesian_device(args[0], args[1], idle=args[2])
        Cn.step_cartesian_device(t, g, idle=idle if idle.any() else None)
        log.append(dict(need=need, host={k: v.copy() for k, v in rec.items()}, A=A.state, B=B.state, C=Cn.state, bufB=buffers(B), bufC=buffers(Cn)))
    for e in (A, B, Cn):
        e.close()
    return steps, marks, log


def test_twin_run_host_loop_and_device_path(twin_run):
    """State, `solved`, record, solution and residual of B against the host loop A, bit for bit after every step of the schedule."""
    steps, (z, u, w), log = twin_run
    for s, L in enumerate(log):
        t, g, idle = steps[s]
        assert same_bits(L['A'], L['B']), s
        assert np.array_equal(L['bufB']['solved'], L['need'].astype(np.uint8)), (s, np.flatnonzero(L['bufB']['solved'] != L['need']))
        for k in ('solution', 'residual'):
            assert same_bits(L['bufB'][k], L['host'][k]), (s, k)
        rq, hq = L['bufB']['request'], L['host']['request']
        assert np.array_equal(bits(rq), bits(hq)), s
        if s == 0:
            assert L['need'].all()
        if s in (3, 7):       # (at step 7 some of the redrawn envs are idle: they solve at their first step that is not)
            assert (L['need'].sum() == N // 3 if s == 3 else 0 < L['need'].sum() <= N // 3) and not L['need'][u]
        if s == 4:
            assert not L['need'].any() and np.signbit(t[z, 1]) and not np.signbit(rq[z, 1])        # -0.0 == 0.0: no solve, the record keeps +0.0
        if 5 <= s <= 9 and idle.any():
            prev = log[s - 1]['bufB']
            for k in ('request', 'solution', 'residual'):
                assert same_bits(L['bufB'][k][idle], prev[k][idle]), (s, k)
        if s >= 10:           # a NaN request solves on every step; at step 10 the envs redrawn at 7 and idle since solve too
            assert L['need'][w] and np.isnan(rq[w, 5]) and (L['need'].sum() == 1 or s == 10)
        if s > 0:
            assert not L['need'][u]
    # u was never solved again although its joints moved: its command stays the solution of step 0
    assert same_bits(log[-1]['bufB']['solution'][u], log[0]['bufB']['solution'][u])
    assert np.abs(log[-1]['B'][u, :7] - log[0]['B'][u, :7]).max() > 1e-3
    # the gripper commands changed on every step and caused no solve
    assert all(not np.array_equal(steps[s][1], steps[s - 1][1]) for s in range(1, 40))
    assert sum(int(L['need'].sum()) for L in log[11:]) == len(log) - 11


def test_host_arguments_equal_device_arguments(twin_run):
    steps, marks, log = twin_run
    for s, L in enumerate(log):
        assert same_bits(L['B'], L['C']), s
        for k in BUFFERS:
            assert same_bits(L['bufB'][k], L['bufC'][k]), (s, k)


def test_policy_state_survives_resets_writes_forks_snapshots_and_checkpoints():
    B, T = make(), make()
    for e in (B, T):
        scatter_postures(e)
    assert B.L.rr_cartesian_invalidate(B.h, None, 0) == 0       # a handle that never stepped: a no-op
    B.cartesian_invalidate()
    rng = np.random.default_rng(4)
    t = ci.separated_targets()[1]
    td, gd = dev(t), dev(ci.grippers(rng))
    for e in (B, T):
        e.snapshot_slots(2)
        e.step_cartesian_device(td, gd)
        e.step_cartesian_device(td, gd)
    mask = (rng.random(N) < 0.4).astype(np.uint8)
    src = rng.integers(-1, N, size=N).astype(np.int32)
    moved = B.state
    moved[:, :7] += 0.05
    ckpt = {}

    def ops(e):
        yield 'reset', lambda: e.reset(mask)
        yield 'write_state', lambda: e.write_state(moved, mask, joint_pos=True)
        yield 'fork', lambda: e.fork(src)
        yield 'save_snapshot', lambda: e.save_snapshot(1)
        yield 'load_snapshot', lambda: e.load_snapshot(0)
        yield 'checkpoint', lambda: ckpt.__setitem__(id(e), e.checkpoint())
        yield 'restore', lambda: e.restore(ckpt[id(e)])

    for (name, on_b), (_, on_t) in zip(ops(B), ops(T)):
        before = buffers(B, ('request', 'solution', 'residual'))
        on_b(), on_t()
        after = buffers(B, ('request', 'solution', 'residual'))
        for k in before:
            assert same_bits(before[k], after[k]), (name, k)
        assert same_bits(B.state, T.state), name
        for e in (B, T):
            e.step_cartesian_device(td, gd)
        assert not B.cartesian_buffer('solved', host=True).any(), name
        assert same_bits(B.state, T.state), name
    # invalidate: exactly the masked, non-idle envs solve at the next step -- from their present joints
    for on_device in (True, False):
        m = rng.random(N) < 0.4
        idle = rng.random(N) < 0.2
        B.cartesian_invalidate(dev(m) if on_device else m)
        req = B.cartesian_buffer('request', host=True)
        assert np.isnan(req[m]).all() and same_bits(req[~m], t[~m])
        q, err = B.ik(t)
        B.step_cartesian_device(td, gd, idle=dev(idle))
        got = buffers(B)
        want = m & ~idle
        assert np.array_equal(got['solved'], want.astype(np.uint8)), on_device
        assert same_bits(got['solution'][want], np.ascontiguousarray(q[want, :7])) and same_bits(got['residual'][want], err[want])
        assert np.isnan(got['request'][m & idle]).all()
        B.step_cartesian_device(td, gd)       # the idle ones of the mask now
        assert np.array_equal(B.cartesian_buffer('solved', host=True), (m & idle).astype(np.uint8))
    B.cartesian_invalidate()
    B.step_cartesian_device(td, gd)
    assert B.cartesian_buffer('solved', host=True).all()
    B.close(), T.close()


def test_refusals_leave_everything_untouched():
    env = make()
    scatter_postures(env)
    t = ci.separated_targets()[1]
    td, gd = dev(t), dev(ci.grippers(np.random.default_rng(5)))
    env.step_cartesian_device(td, gd)
    before, state = buffers(env), env.state
    other = np.ascontiguousarray(redraw(np.random.default_rng(6), N))
    od, g_host = dev(other), np.zeros((N, 2), np.float32)
    L, h = env.L, env.h
    EINVAL = -1
    assert L.rr_step_cartesian(h, od.data_ptr(), gd.data_ptr(), None, 1, 3, None) == EINVAL and 'bad render_mode' in L.rr_last_error().decode()
    assert L.rr_step_cartesian(h, od.data_ptr(), gd.data_ptr(), None, 1, 2, None) == EINVAL and 'bad render_mode' in L.rr_last_error().decode()
    assert L.rr_step_cartesian(h, od.data_ptr(), gd.data_ptr(), None, 1, -1, None) == EINVAL
    # a mixed set through the raw entry: one flag, an array on the other side
    assert L.rr_step_cartesian(h, od.data_ptr(), g_host.ctypes.data, None, 1, 0, None) == EINVAL and 'same side' in L.rr_last_error().decode()
    assert L.rr_step_cartesian(h, other.ctypes.data, gd.data_ptr(), None, 0, 0, None) == EINVAL and 'same side' in L.rr_last_error().decode()
    idle = np.zeros(N, np.uint8)
    assert L.rr_step_cartesian(h, od.data_ptr(), gd.data_ptr(), idle.ctypes.data, 1, 0, None) == EINVAL and 'idle' in L.rr_last_error().decode()
    assert L.rr_step_cartesian(h, None, gd.data_ptr(), None, 1, 0, None) == EINVAL and 'null cartesian' in L.rr_last_error().decode()
    assert L.rr_step_cartesian(h, od.data_ptr(), None, None, 1, 0, None) == EINVAL and 'null gripper' in L.rr_last_error().decode()
    with pytest.raises(ValueError, match='same side'):
        env.step_cartesian_device(od, g_host)
    after = buffers(env)
    for k in BUFFERS:
        assert same_bits(before[k], after[k]), k
    assert same_bits(env.state, state)
    buf = (C.c_char * 4)()
    assert L.rr_cartesian_copy_to_host(h, nat.CART_RESIDUAL, buf, 4) == EINVAL and 'size mismatch' in L.rr_last_error().decode()
    assert L.rr_cartesian_buffer(h, 4, None, None) == EINVAL
    # the device views are the buffers the copies read
    view = torch.from_dlpack(env.cartesian_buffer('solution'))
    env.sync()
    assert same_bits(view.cpu().numpy(), after['solution'])
    env.close()


def test_solutions_against_the_float64_checker():
    """Every solved row equals one of oracle.kinematics.ik_candidates to IK_TOL (the rule of tests/test_gpu_ik_macro.py: a candidate, or
    its iterate one update earlier where its residual crossed the threshold within rounding), and the candidate the float64 rule selects
    (converged first, then elbow height) outside the exempt set: the rows whose float64 elbow heights differ by less than IK_TOL, at most
    5 % of the rows (tests/test_cartesian_device_host.py).  The float64 pose residual of every solution is below ik_solve's own
    convergence bound of 1e-2."""
    env = make()
    scatter_postures(env)
    t = ci.separated_targets()[1]
    env.step_cartesian_device(t, ci.grippers(np.random.default_rng(7)))
    got = buffers(env)
    env.close()
    assert got['solved'].all()
    q0 = ci.postures()
    exempt, worst = 0, 0.0
    for i in range(N):
        q11 = np.zeros(11)
        q11[:7] = q0[i]
        pos, quat = t[i, :3].astype(np.float64), t[i, 3:].astype(np.float64)
        cands = ik_candidates(q11, pos, quat)
        d = [min(np.abs(c[0][:7] - got['solution'][i]).max(), np.abs(c[3][:7] - got['solution'][i]).max() if abs(c[4] - 1e-3) < 2e-5 else np.inf)
             for c in cands]
        k = int(np.argmin(d))
        print('row %d: distance to the candidates %s, residual %.3g' % (i, d, got['residual'][i]))
        assert d[k] < IK_TOL, (i, d)
        worst = max(worst, d[k])
        conv = [c[1] < 1e-2 for c in cands]
        chosen = max(range(2), key=lambda j: (conv[j], cands[j][2]))
        if abs(cands[0][2] - cands[1][2]) < IK_TOL:
            exempt += 1
        else:
            assert k == chosen or d[chosen] < IK_TOL, (i, "another branch than the float64 rule's", d, [c[2] for c in cands])
        sol11 = np.zeros(11)
        sol11[:7] = got['solution'][i]
        assert ee_residual(sol11, pos, quat) < 1e-2, i
    assert exempt <= 0.05 * N, exempt
    print("cartesian solutions: %d rows to %.0e rad of a float64 candidate (worst %.2e), %d exempt from the branch check" % (N, IK_TOL, worst, exempt))


def test_mixing_with_joint_steps_and_macro_steps_changes_no_cartesian_buffer():
    env = make()
    scatter_postures(env)
    t = ci.separated_targets()[1]
    td, gd = dev(t), dev(ci.grippers(np.random.default_rng(8)))
    env.step_cartesian_device(td, gd)
    before = buffers(env)
    env.step(np.full((N, 9), 0.1, np.float32))
    for k in BUFFERS:
        assert same_bits(buffers(env)[k], before[k]), ('step', k)
    m = np.random.default_rng(9).uniform([-0.25, -0.5] * 2, [0.05, 0.5] * 2, size=(N, 4)).astype(np.float32)
    env.step_macro_device(dev(m))
    env.ik(t)
    for k in BUFFERS:
        assert same_bits(buffers(env)[k], before[k]), ('step_macro_device', k)
    env.step_cartesian_device(td, gd)
    after = buffers(env)
    assert not after['solved'].any()
    for k in ('request', 'solution', 'residual'):
        assert same_bits(after[k], before[k]), k
    env.close()
