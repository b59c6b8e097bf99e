"""GPU tests (-m gpu) of the step's joint torque inputs (rr_set_joint_torques; k_joint_torque, csrc/rr_torque.inc): one step against
the float64 numpy step with the torque applied (tests/numpy_torque.py), negative controls on the reference side, bit-for-bit
neutrality when unused, the launch point against an in-line twin, gravity compensation from posture_dynamics(), persistence and
masks.  N = 5 is one full 4-env workgroup of the preparation plus a ragged one (and a ragged 16-env workgroup of the torque kernel),
N = 70 several workgroups of both and of the split placements."""
import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_actuators as na
from tests import numpy_dynamics as nd
from tests import numpy_step as ns
from tests import numpy_torque as nt
from tests.test_gpu_contacts_fuzz import state_bounds, SENS_FACTOR, SENS_RUNS, _grasp_script
from tests.test_gpu_numpy_step import edge_states, _dev, force_bound
from tests.test_gpu_round6 import _make, S_QDS, S_OR

pytestmark = pytest.mark.gpu

W = H = 64
NJ = 11
MAX_FORCE = ns.SOLVER_DEFAULTS['motor_max_force']
PLAIN = {'RR_NO_LOOKAHEAD': '1', 'RR_NO_SPLIT': '1'}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def gravity_scale():
    """Per joint: the largest gravity torque of the model over postures uniform within the limits (float64; 256 postures)."""
    lo, hi = nd.limits()
    q = np.random.default_rng(11).uniform(lo, hi, (256, NJ))
    return np.abs(ns.bias(q, np.zeros_like(q))).max(0)


def random_torques(N, seed, zero_rows=()):
    """tau [N, 11] float32, every entry uniform within +-3 x the joint's largest gravity torque; the rows `zero_rows` all zero."""
    g = gravity_scale()
    t = np.random.default_rng(seed).uniform(-3.0, 3.0, (N, NJ)) * g
    t[list(zero_rows)] = 0.0
    return t.astype(np.float32)


def motors_off(N, seed):
    """bool [N, 11]: a random subset of joints per env, at least one and not all."""
    rng = np.random.default_rng(seed)
    off = rng.random((N, NJ)) < 0.4
    for i in range(N):
        off[i, rng.integers(NJ)] = True
        on = rng.integers(NJ)
        off[i, on] = off[i, on] and off[i].sum() == 1
    return off


@pytest.mark.parametrize('N', [5, 70])
def test_one_step_against_the_float64_step_and_the_wrong_features_miss(monkeypatch, N):
    """One step with a torque table from states of tests/test_gpu_numpy_step.py's edge_states, motors off (max_force = 0) on a random
    subset of joints per env and default motors elsewhere, on a RR_NO_LOOKAHEAD handle (the preparation record read after the step is
    this step's).  Env 2 has a zero row.
    (a) RR_F_PREP's qd* of EVERY env against numpy's qd* + dt M^-1 tau at that file's ceiling 2e-4 + 2e-6 |qd| + 5e-5 bterm, bterm
        over dt M^-1 (bias - tau); the zero-row env against numpy's plain qd*.
    (b) The stepped state of the checked envs (all at N = 5; eight at N = 70) against tests/numpy_actuators.step -- numpy_step.step
        with per-joint motor forces -- under numpy_torque.applied, through test_gpu_numpy_step's comparison: state_bounds /
        force_bound, over a flat bound SENS_FACTOR x the reference's own one-ulp spread.
    (c) Negative controls on the reference side -- -tau, M in the place of M^-1, the previous step's table (a torque applied one step
        late) --: each misses the ceiling of (a) on EVERY env with a non-zero row, and the bounds of (b) on every checked one.
    Measured on the MI355X (none raised; NOTEBOOK.md, "Joint torque inputs of the step"): qd* worst ratio 0.081 (N = 5) / 0.170
    (N = 70), state worst deviation / flat bound 0.128 / 0.097; the controls' smallest qd* ratio x3 993 (one step late, N = 70)."""
    env = _make(monkeypatch, {'RR_NO_LOOKAHEAD': '1'}, N, objects=3, width=W, height=H)
    off = motors_off(N, 21)
    max_force = np.where(off, 0.0, MAX_FORCE).astype(np.float32)
    env.set_env_actuators(max_force=max_force)
    tau_prev, tau = random_torques(N, 31, zero_rows=(2,)), random_torques(N, 32, zero_rows=(2,))
    env.state = edge_states(N, 3)
    env.set_joint_torques(tau_prev)
    env.step((synthetic_actions(range(N), 0, seed=3) * 1.6).astype(np.float32))
    cmd = (synthetic_actions(range(N), 1, seed=3) * 1.6).astype(np.float32)
    st0 = env.state
    caches = [env.contacts(i) for i in range(N)]
    env.set_joint_torques(tau)
    assert np.array_equal(_bits(env.joint_torques()), _bits(tau))
    env.step(cmd)
    st1, rec, flags = env.state, env.host(nat.F_PREP).astype(np.float64), env.host(nat.F_ERRFLAGS)
    new = [env.contacts(i) for i in range(N)]
    env.close()
    live = (flags == 0) & np.isfinite(st0).all(1) & np.isfinite(st1).all(1)
    assert live.sum() >= N - (N + 7) // 8, "more than the fastest edge envs diverged: %s" % np.flatnonzero(~live)
    nonzero = np.abs(tau).max(1) > 0
    assert not nonzero[2] and nonzero.sum() == N - 1

    # (a) the record's qd* of every env, vectorised
    dyn = np.broadcast_to(ns.default_dynamics(), (N, 3, 8))
    pr = ns.prep(st0.astype(np.float64), dyn)
    tau64, qd = tau.astype(np.float64), st0[:, 11:22].astype(np.float64)
    ceil = nt.qds_ceiling(pr, qd, tau64)
    got = rec[:, S_QDS:S_OR]
    ratio = lambda mode, t: np.abs(got - (pr['qds'] + nt.torque_term(pr, t, mode))) / ceil
    ra = ratio('applied', tau64)
    print("N=%d: qd* worst |device - numpy| / ceiling %.3f (env %d); the zero-row env %.3f" % (N, ra[live].max(), int(np.argmax(np.where(live, ra.max(1), 0))), ra[2].max()))
    assert ra[live].max() < 1.0, ra.max(1)
    controls = {'negated': ratio('negated', tau64), 'mass for inverse': ratio('mass', tau64), 'one step late': ratio('applied', tau_prev.astype(np.float64))}
    sel = live & nonzero
    for name, r in controls.items():
        print("N=%d: control '%s': qd* worst ratio per env, the smallest over the envs with a non-zero row %.1f" % (N, name, r.max(1)[sel].min()))
        assert (r.max(1)[sel] > 1.0).all(), (name, r.max(1))
        assert r[2].max() < 1.0                      # (the zero-row env: every control is the plain step there)

    # (b) the stepped state of the checked envs, (c) the controls on them
    rng = np.random.default_rng(1)
    robot = [i for i in range(N) if live[i] and ((new[i][:, 0] >= 0) & (new[i][:, 0] < 16)).any()]
    picks = list(range(N)) if N <= 8 else sorted(set([0, 2, N - 1] + sorted(robot, key=lambda i: -len(new[i]))[:3] + [i for i in range(N) if i % 16 == 5]))[:8]
    worst, checked = 0.0, 0
    for i in [i for i in picks if live[i]]:
        cd = new[i]
        kw = dict(dyn=ns.default_dynamics(), prev=caches[i], max_force=max_force[i].astype(np.float64))
        run = lambda t, mode='applied', s=st0[i], c=cd: _applied_step(s, cmd[i], c, t, mode, kw)
        res = run(tau64[i])
        f_np, f_dev = res['lambda_n'] / ns.DT, cd[:, 10].astype(np.float64)
        fmax = float(f_dev.max()) if len(cd) else 0.0
        flat = state_bounds(fmax) + (force_bound(fmax),)
        d = _dev(st1[i], res['state']) + (float(np.abs(f_dev - f_np).max()) if len(cd) else 0.0,)
        bb = flat
        if any(x > y for x, y in zip(d, flat)):
            def ulp(a):
                up = rng.random(a.shape) < 0.5
                return np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf)))
            sp = [0.0] * 4
            for _ in range(SENS_RUNS):
                cdp = cd.copy()
                cdp[:, 3:10] = ulp(cd[:, 3:10])
                r = run(tau64[i], s=ulp(st0[i]), c=cdp)
                dd = _dev(r['state'], res['state']) + (float(np.abs(r['lambda_n'] / ns.DT - f_np).max()) if len(cd) else 0.0,)
                sp = [max(a, b) for a, b in zip(sp, dd)]
            bb = tuple(max(x, SENS_FACTOR * y) for x, y in zip(flat, sp))
        print("  N=%d env %d (%d contacts, motors off on %s): deviation %s, bounds %s" % (N, i, len(cd), np.flatnonzero(off[i]).tolist(), d, bb))
        assert all(x <= y for x, y in zip(d, bb)), (N, i, d, bb)
        worst = max(worst, max(x / y for x, y in zip(d, flat)))
        checked += 1
        # the torque shows in the result: the plain step misses (a motor-less joint takes dt M^-1 tau unopposed)
        wrong = {'no torque': run(np.zeros(NJ)), 'negated': run(tau64[i], 'negated'), 'mass for inverse': run(tau64[i], 'mass'),
                 'one step late': run(tau_prev[i].astype(np.float64))}
        for name, r in wrong.items():
            miss = max(x / y for x, y in zip(_dev(st1[i], r['state']), bb))
            if nonzero[i]:
                assert miss > 1.0, (N, i, name, miss)
            else:
                assert miss <= 1.0, (N, i, name, miss)
    print("N=%d: %d envs stepped against numpy (%d with robot contacts); worst deviation / flat bound %.3f" % (N, checked, len([i for i in picks if i in robot]), worst))
    assert checked >= min(N, 5) - 1


def _applied_step(state, cmd, contacts, tau, mode, kw):
    with nt.applied(tau, mode):
        return na.step(np.asarray(state).astype(np.float64), cmd.astype(np.float64), contacts, **kw)


def test_nothing_changes_when_unused():
    """Handle A is never touched, B gets set_joint_torques(zeros), C a table that is non-zero on env 2 only.  30 steps of
    synthetic_actions: A and B are equal bit for bit after every step, C equals A on every env but env 2 (envs are independent).
    Then set_joint_torques(None) on C and A's checkpoint restored into it -- every env of C, env 2 included, rewritten with A's
    state and contact history: C continues bit for bit with A."""
    N = 5
    A, B, C = (BatchedREALRobotEnv(N, objects=3, width=W, height=H) for _ in range(3))
    B.set_joint_torques(np.zeros((N, NJ), np.float32))
    t = np.zeros((N, NJ), np.float32)
    t[2] = random_torques(1, 5)[0]
    C.set_joint_torques(t)
    fields = (nat.F_STATE, nat.F_TOUCH, nat.F_CONTACT_COUNT, nat.F_ERRFLAGS)
    others = np.arange(N) != 2
    for s in range(30):
        cmd = synthetic_actions(range(N), s, seed=7).astype(np.float32)
        for e in (A, B, C):
            e.step(cmd, render=(s % 10 == 9))
        for f in fields:
            a, b, c = (_bits(e.host(f)) for e in (A, B, C))
            assert np.array_equal(a, b), (s, f)
            assert np.array_equal(a[others], c[others]), (s, f)
    assert not np.array_equal(_bits(A.state[2]), _bits(C.state[2]))           # (the torque acted on env 2)
    assert np.array_equal(A.host(nat.F_RGB), B.host(nat.F_RGB))
    C.set_joint_torques(None)
    assert not C.joint_torques().any()
    C.restore(A.checkpoint())
    for s in range(30, 40):
        cmd = synthetic_actions(range(N), s, seed=7).astype(np.float32)
        for e in (A, C):
            e.step(cmd)
        for f in fields:
            assert np.array_equal(_bits(A.host(f)), _bits(C.host(f))), (s, f)
    for e in (A, B, C):
        e.close()


def test_look_ahead_and_placement_against_the_in_line_twin(monkeypatch):
    """The launch point.  The default handle (look-ahead, split placements, device tensors) and a twin with RR_NO_LOOKAHEAD, RR_NO_SPLIT
    and host arrays get the same torque sequence, a new table every step, N = 70 with every fourth env closing the gripper on the
    cube (the fuzz tests' grasp script: heavy envs, so split placements occur), motors off on random joints (a position motor would
    take the torque up and leave a misplaced kernel to the last bits), render on for a third of the steps: the state is equal bit
    for bit after every step.  A torque kernel that ran before the look-ahead had landed, or beside a solve, shows here."""
    N, T = 70, 40
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b = _make(monkeypatch, PLAIN, N, objects=3, width=W, height=H)
    script = _grasp_script()
    grasp = np.arange(N) % 4 == 1
    t0 = 280                                    # the script closes the gripper on the cube from step 270 on
    assert len(script) >= t0 + T
    # (bring the grasp envs to the cube without torques, both handles alike)
    for s in range(t0):
        cmd = (synthetic_actions(range(N), s, seed=3) * 1.6).astype(np.float32)
        cmd[grasp] = script[s]
        a.step(cmd)
        b.step(cmd)
    assert np.array_equal(_bits(a.state), _bits(b.state))
    # motors off on some joints, so that the torques decide where those joints go (a position motor takes a feed-forward torque up);
    # the grasp envs keep their arm and fingers and free the last arm joint alone
    off = motors_off(N, 23)
    off[grasp] = False
    off[grasp, 6] = True
    for e in (a, b):
        e.set_env_actuators(max_force=np.where(off, 0.0, MAX_FORCE).astype(np.float32))
    classes = set()
    scale = gravity_scale() / 3.0               # (a third of the gravity torques: the grasp survives)
    rng = np.random.default_rng(9)
    for s in range(t0, t0 + T):
        cmd = (synthetic_actions(range(N), s, seed=3) * 1.6).astype(np.float32)
        cmd[grasp] = script[s]
        tau = (rng.uniform(-1, 1, (N, NJ)) * scale).astype(np.float32)
        tau[rng.random(N) < 0.2] = 0.0          # zero rows come and go
        dev = _cuda(tau)
        a.set_joint_torques(dev)
        b.set_joint_torques(tau)
        render = s % 3 == 0
        a.step(cmd, render=render)
        b.step(cmd, render=render)
        sa, sb = a.state, b.state
        assert np.array_equal(_bits(sa), _bits(sb)), (s, np.flatnonzero((_bits(sa) != _bits(sb)).any(1)))
        assert np.array_equal(_bits(a.host(nat.F_TOUCH)), _bits(b.host(nat.F_TOUCH))), s
        classes |= set(a.host(nat.F_ENV_CLASS).tolist())
        del dev
    assert np.array_equal(a.host(nat.F_RGB), b.host(nat.F_RGB))
    assert len(classes) >= 2, classes           # (heavy envs were in play: the split placements ran)
    a.close()
    b.close()


def test_holding_against_gravity_with_the_bias_of_posture_dynamics():
    """tests/test_numpy_torque.py's hold condition on the device: N = 5 at the three mid-range postures, motors off on all joints, zero
    joint damping; each of 50 steps sets tau = posture_dynamics()['bias'] (the [N, 1, 11] device view, in place).  The compensated
    drift is at most 0.05 x the drift of a second handle stepped with tau = 0.  Measured on the MI355X: the held arm does not move at
    all (drift exactly 0: the query's bias has the preparation's bits and the kernel sums in its order), the free one by 0.86 to 2.9
    rad."""
    N = 5
    q0 = nt.HOLD_POSTURES[np.arange(N) % len(nt.HOLD_POSTURES)].astype(np.float32)
    drifts = []
    for hold in (True, False):
        env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
        env.set_env_actuators(max_force=0.0, damping=0.0)
        st = env.state
        st[:, :NJ], st[:, NJ:2 * NJ] = q0, 0.0
        env.write_state(st, joint_pos=True, joint_vel=True)
        worst = np.zeros(N)
        for s in range(nt.HOLD_STEPS):
            if hold:
                env.set_joint_torques(env.posture_dynamics()['bias'])
            env.step(None)
            worst = np.maximum(worst, np.abs(env.state[:, :NJ] - q0).max(1))
        assert (env.host(nat.F_ERRFLAGS) == 0).all()
        if hold:
            robot = sum(int(((c[:, 0] >= 0) & (c[:, 0] < 16)).any()) for c in (env.contacts(i) for i in range(N)))
            assert robot == 0, "a held arm touches something: the postures are chosen free"
        drifts.append(worst)
        env.close()
    held, free = drifts
    print("drift over %d steps: held %s, free %s, ratio %s" % (nt.HOLD_STEPS, held, free, held / free))
    assert (free > 0.1).all()
    assert (held <= nt.HOLD_RATIO * free).all(), (held, free)


def test_persistence_masks_and_the_zero_copy_buffer():
    """The table survives reset, a device-mask reset, fork, load_snapshot and an episode's auto-reset; env_mask changes only its envs;
    joint_torques() reads back what was set; a device-side write into joint_torque_buffer, made in stream order, acts in the next
    step; the vector env forwards "joint_torques"."""
    import torch
    from tests.test_gpu_episode import _home, _table
    N = 5
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    assert not env.joint_torques().any()                               # a fresh handle
    tau = random_torques(N, 41)
    env.set_joint_torques(tau)
    same = lambda: np.array_equal(_bits(env.joint_torques()), _bits(tau))
    assert same()
    cmd = lambda s: synthetic_actions(range(N), s, seed=5).astype(np.float32)
    env.step(cmd(0))
    assert same()                                                      # nothing clears the table after a step
    env.reset()
    assert same()
    env.reset(_cuda(np.array([1, 0, 1, 0, 0], np.uint8)))
    env.reset(np.array([0, 1, 0, 0, 1], np.uint8))
    assert same()
    env.snapshot_slots(1)
    env.step(cmd(1))
    env.fork(np.array([1, 1, -1, 0, 3], np.int32))
    assert same()
    env.load_snapshot(0)
    assert same()
    env.state = env.state
    env.write_state(_cuda(env.state), joint_pos=True)
    assert same()
    env.restore(env.checkpoint())
    assert same()
    start, final, flags, _ = _table(_home(env), images=False)
    env.set_goals(start, final, flags)
    env.set_env_goals((np.arange(N) % 5).astype(np.int32))
    env.set_episode(3, 1)
    for s in range(4):
        env.step(cmd(2 + s))
        env.episode_update(reset_done=True)
    assert (env.episode_buffer('episode', host=True) > 0).any()         # (an auto-reset happened)
    assert same()
    env.set_episode(0, 1)
    # masks: only the masked rows change, from either side; None zeroes the masked rows
    t2 = random_torques(N, 42)
    m = np.array([0, 1, 1, 0, 0], np.uint8)
    env.set_joint_torques(t2, env_mask=m)
    tau[m != 0] = t2[m != 0]
    assert same()
    t3 = random_torques(N, 43)
    m = np.array([1, 0, 0, 0, 1], bool)
    env.set_joint_torques(_cuda(t3), env_mask=_cuda(m))
    tau[m] = t3[m]
    assert same()
    env.set_joint_torques(None, env_mask=np.array([0, 0, 1, 0, 0], np.uint8))
    tau[2] = 0.0
    assert same()
    # refusals change nothing
    bad = t2.copy()
    bad[3, 4] = np.inf
    with pytest.raises(ValueError):
        env.set_joint_torques(bad)
    assert env.L.rr_set_joint_torques(env.h, bad.ctypes.data, 0, None, 0) == -1 and 'not finite' in env.L.rr_last_error().decode()
    assert env.L.rr_set_joint_torques(env.h, bad.ctypes.data, 0, m.astype(np.uint8).ctypes.data, 1) == -1 and 'same side' in env.L.rr_last_error().decode()
    assert same()
    # (the non-finite row outside the mask is not looked at)
    env.set_joint_torques(bad, env_mask=np.array([1, 0, 0, 0, 0], np.uint8))
    tau[0] = bad[0]
    assert same()

    # the zero-copy buffer: a device-side write in stream order acts in the next step, like the same table set by the call
    twin = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    for e in (env, twin):
        e.set_episode(0, 1)
        e.reset()
        e.set_env_actuators(max_force=np.where(motors_off(N, 3), 0.0, MAX_FORCE).astype(np.float32))
    t4 = random_torques(N, 44, zero_rows=(1,))
    twin.set_joint_torques(t4)
    env.sync()
    view = torch.from_dlpack(env.joint_torque_buffer)
    assert tuple(view.shape) == (N, NJ) and view.dtype == torch.float32
    view.copy_(torch.from_numpy(t4).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(env.joint_torques()), _bits(t4))
    for s in range(3):
        env.step(cmd(10 + s))
        twin.step(cmd(10 + s))
    assert np.array_equal(_bits(env.state), _bits(twin.state))
    plain = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    plain.set_env_actuators(max_force=np.where(motors_off(N, 3), 0.0, MAX_FORCE).astype(np.float32))
    for s in range(3):
        plain.step(cmd(10 + s))
    diff = (_bits(plain.state) != _bits(env.state)).any(1)
    assert diff[[0, 2, 3, 4]].all() and not diff[1]                     # the torque acted; the zero-row env is the plain step
    # the [N, 1, 11] view of posture_dynamics() is taken in place: the table then holds the bias
    bias = env.posture_dynamics()['bias']
    env.set_joint_torques(bias)
    assert np.array_equal(_bits(env.joint_torques()), _bits(env.posture_dynamics_buffer('bias', host=True)[:, 0]))
    for e in (env, twin, plain):
        e.close()


def test_vector_env_forwards_joint_torques():
    from real_robots_amd.vector import REALRobotVectorEnv
    N = 5
    v = REALRobotVectorEnv(N, eye_width=W, eye_height=H, render_every_step=False, joint_torque_actions=True)
    assert v.action_space.spaces['joint_torques'].shape == (N, NJ) and v.single_action_space.spaces['joint_torques'].shape == (NJ,)
    v.reset()
    tau = random_torques(N, 51)
    act = {"joint_command": np.zeros((N, 9), np.float32), "joint_torques": tau}
    v.step(act)
    assert np.array_equal(_bits(v._be.joint_torques()), _bits(tau))
    v.step({"joint_command": np.zeros((N, 9), np.float32)})             # absent: the table is kept
    assert np.array_equal(_bits(v._be.joint_torques()), _bits(tau))
    v.step(np.zeros((N, 9), np.float32))
    assert np.array_equal(_bits(v._be.joint_torques()), _bits(tau))
    v.close()
    d = REALRobotVectorEnv(N, eye_width=W, eye_height=H, render_every_step=False)
    assert list(d.action_space.spaces) == ['joint_command', 'render'] and list(d.single_action_space.spaces) == ['joint_command', 'render']
    d.close()
