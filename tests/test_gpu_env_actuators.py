"""Per-env actuators (rr_set_env_actuators / rr_get_env_actuators; setJointMotorControl2 gains and force, jointDamping).

The core check: a batch whose envs carry different motor gains, motor forces and joint dampings steps every env exactly -- bit for
bit, contacts, touch and images included -- as a handle that got that env's values through `solver=` (gains, force) or through a
model blob with `body_damping` patched does.  Then one step against the float oracle created with each set, the macro sensitivity
table of tests/golden/macro_sensitivity.json out of ONE batch, lifetime / masks / checkpoints / validation, the facade and the
vector env.

The sets keep the rate limit on and kd >= 1 (tests/test_gpu_solver_params.py: kd < 1, or kp 0.5 without the rate limit, diverge
under full-range commands in the float64 oracle too); the float64 oracle was run with each scalar set over the drive below for
six envs per set and every state stayed finite (largest joint velocity 16 rad/s for `stiff`, 3 for `soft`, 6 for `damped`).
"""
import json
import os

import numpy as np
import pytest

import oracle.oracle as oracle_mod
from oracle.kinematics import generate_plan
from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from real_robots_amd.mathutil import quat_from_euler
from tests.test_gpu_contacts_fuzz import oracle_sensitivity, state_bounds, SENS_FACTOR
from tests.test_gpu_object_dynamics import PATHS, _arr, _compare, _drive, _entries
from tests.test_gpu_solver_params import CHECK_T, HOME, HOME2

pytestmark = pytest.mark.gpu

W = H = 64
N_MIX = 96
NJ = 11
SETS = ('default', 'stiff', 'soft', 'damped')
# what the uniform handle of every set gets through `solver=` ...
SOLVER = ({}, {'motor_kp': 0.3, 'motor_kd': 1.2, 'motor_max_force': 300.0}, {'motor_kp': 0.05, 'motor_max_force': 50.0}, {})
DAMP_SCALE = (1.0, 1.0, 1.0, 3.0)      # ... and through the blob's body_damping


def blob_damping():
    base = nat.model_blob()
    return _arr(base, _entries(base), 'body_damping', (NJ,)).copy()


def damping_blob(damping):
    """The default blob with body_damping replaced (float32 [11])."""
    base = nat.model_blob()
    _, off, _ = _entries(base)['body_damping']
    b = bytearray(base)
    b[off: off + 4 * NJ] = np.asarray(damping, np.float32).tobytes()
    return bytes(b)


def set_rows(k):
    """Set k as rows [11, 4] {kp, kd, max_force, damping}, constant over the joints (the damping: the blob's times the set's scale)."""
    s = dict(nat.SOLVER_DEFAULTS, **SOLVER[k])
    rows = np.zeros((NJ, 4), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = s['motor_kp'], s['motor_kd'], s['motor_max_force']
    rows[:, 3] = blob_damping() * np.float32(DAMP_SCALE[k])
    return rows


def mixed_rows(n):
    return np.stack([set_rows(i % len(SETS)) for i in range(n)])


def apply_rows(env, rows, env_mask=None):
    env.set_env_actuators(kp=rows[..., 0], kd=rows[..., 1], max_force=rows[..., 2], damping=rows[..., 3], env_mask=env_mask)


def uniform_handle(monkeypatch, k, n=N_MIX):
    with monkeypatch.context() as m:
        if DAMP_SCALE[k] != 1.0:
            m.setattr(nat, 'model_blob', lambda b=damping_blob(set_rows(k)[:, 3]): b)
        return BatchedREALRobotEnv(n, objects=3, width=W, height=H, solver=SOLVER[k] or None)


def raw(env):
    out = np.empty((env.N, NJ, 4), np.float32)
    nat.check(env.L.rr_get_env_actuators(env.h, out.ctypes.data))
    return out


@pytest.mark.parametrize('path', list(PATHS))
def test_mixed_batch_equals_uniform_handles_bit_for_bit(monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    mixed = BatchedREALRobotEnv(N_MIX, objects=3, width=W, height=H)
    assert np.array_equal(raw(mixed), np.tile(set_rows(0), (N_MIX, 1, 1))), "defaults: the handle's scalars and the blob's damping"
    apply_rows(mixed, mixed_rows(N_MIX))
    assert np.array_equal(raw(mixed), mixed_rows(N_MIX))
    uniform = [uniform_handle(monkeypatch, k) for k in range(len(SETS))]
    for k, u in enumerate(uniform):
        assert np.array_equal(raw(u), np.tile(set_rows(k), (N_MIX, 1, 1))), "the uniform handle's own table is set %s" % SETS[k]
    members = [np.arange(k, N_MIX, len(SETS)) for k in range(len(SETS))]
    cls_seen = np.zeros(N_MIX, np.int64)

    def check(t, render):
        cls_seen[:] = np.maximum(cls_seen, mixed.host(nat.F_ENV_CLASS))
        if render:
            for k in range(len(SETS)):
                _compare(mixed, uniform[k], members[k], with_contacts=(t % 50 == 49))
    _drive([mixed] + uniform, 300, seed=7, on_step=check)
    for k in range(1, len(SETS)):
        assert (cls_seen[members[k]] >= 1).any() and (cls_seen[members[k]] == 2).any(), \
            "set %s never reached the heavy / very heavy solve" % SETS[k]
    assert (mixed.host(nat.F_ERRFLAGS) & ~np.uint32(8) == 0).all()
    # the mixed batch is not the default batch: every set really changed something
    for k in range(1, len(SETS)):
        assert not np.array_equal(mixed.state[members[k]], uniform[0].state[members[k]]), SETS[k]
    for e in [mixed] + uniform:
        e.close()


def test_one_step_differentials_against_the_oracle_with_each_set(monkeypatch):
    mixed = BatchedREALRobotEnv(N_MIX, objects=3, width=W, height=H)
    apply_rows(mixed, mixed_rows(N_MIX))
    _drive([mixed], 160, seed=3)
    rng = np.random.default_rng(1)
    cmd = (synthetic_actions(range(N_MIX), 160, seed=3) * 1.6).astype(np.float32)
    st0 = mixed.state
    ncs = np.array([len(mixed.contacts(i)) for i in range(N_MIX)])
    picks = {k: int(max(range(k, N_MIX, 4), key=lambda i: ncs[i])) for k in range(1, 4)}
    caches = {i: mixed.contacts(i) for i in picks.values()}
    mixed.step(cmd)
    st1 = mixed.state
    for k, i in picks.items():
        assert ncs[i] > 0
        with monkeypatch.context() as m:
            m.setattr(oracle_mod, 'model_blob', lambda b=damping_blob(set_rows(k)[:, 3]): b)
            o = oracle_mod.Oracle(3, W, H, f32=True, **oracle_mod.params_from_solver(SOLVER[k]))
        o.state = st0[i].astype(np.float64)
        o.set_contact_cache(caches[i])
        o.step(cmd[i].astype(np.float64))
        cd, co = mixed.contacts(i), o.contacts()
        keep = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]          # everything but the normal force, mu included
        assert cd.shape == co.shape and np.array_equal(cd[:, keep], co[:, keep].astype(np.float32)), "contact list of set %s" % SETS[k]
        ref = o.state.copy()
        fmax = float(cd[:, 10].max()) if len(cd) else 0.0
        bj, bo, bv = state_bounds(fmax)
        dj = float(np.abs(st1[i][:22] - ref[:22]).max())
        dobj = np.abs(st1[i][22:61] - ref[22:61]).reshape(3, 13)
        do, dv = float(dobj[:, :7].max()), float(dobj[:, 7:].max())
        print("set %s env %d: %d contacts, joints %.2e (bound %.2e) objects %.2e (%.2e) velocities %.2e (%.2e)"
              % (SETS[k], i, ncs[i], dj, bj, do, bo, dv, bv))
        if dj > bj or do > bo or dv > bv:
            sj, so, sv = oracle_sensitivity(o, st0[i], caches[i], cmd[i], ref, 3, rng)
            assert dj <= max(bj, SENS_FACTOR * sj) and do <= max(bo, SENS_FACTOR * so) and dv <= max(bv, SENS_FACTOR * sv), \
                (SETS[k], dj, do, dv, sj, so, sv)
    mixed.close()


def test_macro_sensitivity_table_in_one_batch():
    """72 envs = the 36 pairs of tests/golden/macro_sensitivity.json x {kp 0.1, kp 0.5} in ONE handle (rate limit on), driven like
    `_script_on_device` of tests/test_gpu_solver_params.py: the distance tables match the fixture's float64 tables at the five check
    steps to that test's 1e-4 m, and the verdict at t = 849 (0 / 36 within 1 cm at kp 0.1, 36 / 36 at kp 0.5) comes out of one run."""
    fx = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'macro_sensitivity.json')))
    pairs = [tuple(map(tuple, p)) for p in fx['pairs']]
    assert len(pairs) == 36 and fx['check_steps'] == list(CHECK_T)
    plans = [generate_plan(np.zeros(11), p) for p in pairs]
    TOL = 1e-4
    N = 72
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    kp = np.repeat(np.float32([0.1, 0.5]), 36)
    env.set_env_actuators(kp=kp[:, None])
    for i in range(N):
        for o, y in enumerate((0.0, -0.3, 0.3)):
            env.set_object_pose(i, o, [0.2, y, 0.75, 0, 0, 0, 1])
    assert np.array_equal(env.env_actuators()['kp'], np.tile(kp[:, None], (1, NJ))), "teleports keep the table"
    base = nat.LINK_NAMES.index('base')
    got = np.zeros((N, len(CHECK_T)))
    for t in range(1000):
        env.step(np.stack([plans[i % 36][t] for i in range(N)]).astype(np.float32))
        if t in CHECK_T:
            lp = env.link_poses()[:, base, :3].astype(np.float64)
            for i in range(N):
                p1, p2 = pairs[i % 36]
                tg = {199: [p1[0], p1[1], 0.6], 249: [p1[0], p1[1], 0.46], 749: [p2[0], p2[1], 0.46], 849: HOME2, 999: HOME}[t]
                got[i, CHECK_T.index(t)] = np.linalg.norm(lp[i] - np.asarray(tg))
    assert (env.host(nat.F_ERRFLAGS) == 0).all() and (env.host(nat.F_TIMESTEP) == 1000).all()
    env.close()
    for half, k in enumerate((0.1, 0.5)):
        key = "kp=%g,rate_limit=on" % k
        want, g = np.array(fx['distance_m'][key]), got[36 * half: 36 * half + 36]
        worst = np.abs(g - want).max()
        print("%s: device vs fixture, worst %.2e m; pairs within 1 cm per check point %s (fixture %s)"
              % (key, worst, (g < 0.01).sum(0).tolist(), fx['pairs_within_tolerance'][key]))
        assert worst < TOL, (key, worst, np.unravel_index(np.abs(g - want).argmax(), g.shape))
    i849 = CHECK_T.index(849)
    assert (got[:36, i849] < 0.01).sum() == 0 and (got[36:, i849] < 0.01).sum() == 36


def _steps(envs, n, seed, t0=0, render_last=True):
    for t in range(t0, t0 + n):
        cmd = synthetic_actions(range(envs[0].N), t, seed=seed).astype(np.float32)
        for e in envs:
            e.step(cmd, render=(render_last and t == t0 + n - 1))


def test_masked_update_leaves_the_other_envs_bit_identical():
    N = 32
    a, b = (BatchedREALRobotEnv(N, objects=3, width=W, height=H) for _ in range(2))
    _steps([a, b], 20, seed=5)                        # (the update lands in the middle of a run: the look-ahead is in flight)
    mask = (np.arange(N) % 3 == 1)
    rows = np.tile(set_rows(0), (N, 1, 1))
    rows[:, :, 0] = np.linspace(0.3, 0.05, NJ)
    rows[:, 2, 2] = 2.0
    rows[:, :, 3] *= np.linspace(0.0, 2.0, NJ, dtype=np.float32)
    garbage = rows.copy()
    garbage[~mask] = np.nan                           # rows of the other envs are not read
    nat.check(a.L.rr_set_env_actuators(a.h, garbage.ctypes.data, mask.astype(np.uint8).ctypes.data))
    want = np.tile(set_rows(0), (N, 1, 1))
    want[mask] = rows[mask]
    assert np.array_equal(raw(a), want)
    _steps([a, b], 300, seed=5, t0=20)
    others = np.flatnonzero(~mask)
    _compare(a, b, others, with_contacts=True)
    assert np.isfinite(a.state).all() and not np.array_equal(a.state[mask], b.state[mask])
    # NULL table: the masked envs return to the handle's values; the others keep theirs
    half = mask & (np.arange(N) < N // 2)
    nat.check(a.L.rr_set_env_actuators(a.h, None, half.astype(np.uint8).ctypes.data))
    want[half] = set_rows(0)
    assert np.array_equal(raw(a), want)
    a.set_env_actuators()
    assert np.array_equal(raw(a), raw(b))
    a.close()
    b.close()


def test_lifetime_checkpoints_and_validation():
    N = 16
    rows = mixed_rows(N)
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    apply_rows(a, rows)
    _steps([a], 30, seed=9)
    a.reset()
    assert np.array_equal(raw(a), rows), "reset keeps the table"
    a.state = a.state
    a.set_object_pose(1, 0, [0.0, 0.1, 0.6, 0, 0, 0, 1])
    a.set_object_poses(a.host(nat.F_OBJ_POSE))
    assert np.array_equal(raw(a), rows), "set_state and teleports keep the table"
    _steps([a], 60, seed=9)
    ck = a.checkpoint()
    b = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b.set_env_actuators(kp=0.2, damping=0.0)
    _steps([b], 25, seed=2)
    b.restore(ck)
    assert np.array_equal(raw(b), rows), "a restore puts the checkpoint's table in force"
    _steps([a, b], 100, seed=9, t0=60)
    _compare(a, b, np.arange(N), with_contacts=True)
    # a checkpoint of other handle scalars is still rejected
    c = BatchedREALRobotEnv(N, objects=3, width=W, height=H, solver={'motor_kp': 0.3})
    with pytest.raises(nat.NativeError, match='other step parameters'):
        c.restore(ck)
    c.close()
    # validation through the raw C call: RR_EINVAL, the message names env and joint, nothing changes
    before = raw(a)
    for bad, env_i, joint in ((np.nan, 3, 4), (-0.5, 0, 10), (np.inf, 15, 0)):
        for col in range(4):
            r = before.copy()
            r[env_i, joint, col] = bad
            assert a.L.rr_set_env_actuators(a.h, r.ctypes.data, None) == -1
            msg = a.L.rr_last_error().decode()
            assert 'env %d' % env_i in msg and 'joint %d' % joint in msg, msg
            assert np.array_equal(raw(a), before)
    with pytest.raises(ValueError):
        a.set_env_actuators(kp=np.ones((N, NJ + 1)))
    assert np.array_equal(raw(a), before)
    # 0 is a literal zero: with its motors off env 1 does not follow a command for joint 0 (vertical axis: no gravity torque on it)
    z = BatchedREALRobotEnv(2, objects=3, width=W, height=H)
    z.set_env_actuators(max_force=0.0, env_mask=[0, 1])
    cmd = np.zeros((2, 9), np.float32)
    cmd[:, 0] = 1.0
    for _ in range(60):
        z.step(cmd)
    q = z.state[:, :11]
    assert q[0, 0] > 0.01 and abs(q[1, 0]) < 0.1 * q[0, 0], q
    for e in (a, b, z):
        e.close()


def test_facade_equals_env_0_of_a_batched_handle():
    from real_robots_amd.envs.env import REALRobotEnv
    kp = np.linspace(0.3, 0.05, NJ)
    damping = blob_damping() * np.linspace(0.0, 2.0, NJ, dtype=np.float32)
    f = REALRobotEnv(objects=3, eye_width=W, eye_height=H)
    f.reset()
    f.set_actuators(kp=kp, kd=1.1, max_force=40.0, damping=damping)
    got = f.actuators()
    assert np.array_equal(got['kp'], kp.astype(np.float32)) and np.all(got['kd'] == np.float32(1.1)) and got['damping'].shape == (NJ,)
    be = BatchedREALRobotEnv(3, objects=3, width=W, height=H)
    be.set_env_actuators(kp=kp, kd=1.1, max_force=40.0, damping=damping, env_mask=[1, 0, 0])
    fac = f._backend()
    be.state = np.tile(fac.state, (3, 1))             # the facade's start (its reset places the objects itself)
    for i, name in enumerate(f.robot.used_objects[1:]):
        p = f.robot.object_poses[name]
        be.set_object_home(None, i, np.concatenate([p[:3], quat_from_euler(*p[3:])]))
    rng = np.random.default_rng(2)
    for t in range(100):
        a = rng.uniform(f.robot.min_joints, f.robot.max_joints).astype(np.float32)
        f.step({'joint_command': a, 'render': False})
        be.step(np.tile(a, (3, 1)))
    sf, sb = fac.state, be.state
    assert np.isfinite(sb).all() and np.array_equal(sf[0].view(np.uint32), sb[0].view(np.uint32))
    assert not np.array_equal(sb[0], sb[1]) and np.array_equal(sb[1], sb[2])
    with pytest.raises(ValueError):
        f.set_actuators(kp=np.ones(9))
    f.set_actuators()
    assert np.array_equal(f.actuators()['kp'], be.default_env_actuators()['kp'][0])
    f.close()
    be.close()


def test_vector_env_actuator_randomization():
    from real_robots_amd.vector import REALRobotVectorEnv
    rand = {'kp': (0.8, 1.2), 'kd': (1.0, 1.2), 'max_force': (0.5, 1.0), 'damping': (0.5, 2.0)}
    v = REALRobotVectorEnv(8, eye_width=W, eye_height=H, max_episode_steps=5, render_every_step=False, actuator_randomization=rand,
                           solver={'motor_kp': 0.2})
    _, info = v.reset(seed=11)
    base = v._be.default_env_actuators()
    assert np.all(base['kp'] == np.float32(0.2))
    for k, (lo, hi) in rand.items():
        got = info['actuators'][k]
        assert np.array_equal(got, v._be.env_actuators()[k])
        ratio = got.astype(np.float64) / base[k]
        assert (ratio >= lo - 1e-6).all() and (ratio <= hi + 1e-6).all() and len(np.unique(ratio)) == 8 * NJ
    v._steps[:] = [0, 3, 0, 0, 3, 0, 0, 0]
    first = {k: x.copy() for k, x in info['actuators'].items()}
    for _ in range(2):
        _, _, _, trunc, info = v.step(np.zeros((8, 9), np.float32))
    assert trunc.tolist() == [False, True, False, False, True, False, False, False] and info['_actuators'].tolist() == trunc.tolist()
    for k in rand:
        assert np.array_equal(info['actuators'][k], v._be.env_actuators()[k])
        assert np.all(info['actuators'][k] == first[k], axis=1).tolist() == (~trunc).tolist()
    v.close()


def per_joint_rows():
    """Rows that differ between the joints: kp falling from 0.3 at joint 0 to 0.05 at the fingers, kd 1 .. 1.2, arm joint 1 (the
    shoulder, which carries the arm against gravity) with a motor force low enough to saturate, the blob's damping x 0 .. x 2.  (x 0 .. x 4 together with these gains
    diverges within 45 steps of free motion under the drive's commands in the float64 helper too -- each of the four columns alone
    does not: the joint damping is integrated explicitly -- so the set was changed, not the check.)"""
    rows = set_rows(0)
    rows[:, 0] = np.concatenate([np.linspace(0.3, 0.1, 7), np.full(4, 0.05)])
    rows[:, 1] = np.linspace(1.0, 1.2, NJ)
    rows[:, 2] = 300.0
    rows[1, 2] = 2.0
    rows[:, 3] = blob_damping() * np.linspace(0.0, 2.0, NJ, dtype=np.float32)
    return rows


@pytest.mark.parametrize('prep', ['p16'])
def test_per_joint_rows_against_the_numpy_helper(monkeypatch, prep):
    """One step with rows that differ between the joints, from states with and without robot contacts: device vs
    tests/numpy_actuators.step fed with the device's contact list, at the bounds tests/test_gpu_numpy_step.py applies to the same
    comparison with scalar parameters (state_bounds, force_bound; over a flat bound: SENS_FACTOR x the helper's own spread under
    one-ulp perturbations of its float32 inputs, as there); and RR_F_PREP's unconstrained joint velocities against the helper's
    qd* under the per-joint damping at that file's ceiling for qd*, on the in-line preparation."""
    from tests import numpy_actuators as na
    from tests import numpy_step as ns
    from tests.test_gpu_contacts_fuzz import SENS_RUNS
    from tests.test_gpu_numpy_step import PREP_PATHS, _dev, force_bound
    from tests.test_gpu_round6 import S_QDS, S_OR
    for k, v in PREP_PATHS[prep].items():
        monkeypatch.setenv(k, v)
    N = 48
    rows = per_joint_rows()
    kw = dict(kp=rows[:, 0].astype(np.float64), kd=rows[:, 1].astype(np.float64), max_force=rows[:, 2].astype(np.float64),
              damping=rows[:, 3].astype(np.float64))
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    apply_rows(env, np.tile(rows, (N, 1, 1)))
    _drive([env], 160, seed=3)
    rng = np.random.default_rng(1)
    dyn = ns.default_dynamics(3)
    checked = with_robot = without = saturated = 0
    worst = 0.0
    for t in (160, 175, 190):
        for s in range(t - 14 if t > 160 else t, t):
            env.step((synthetic_actions(range(N), s, seed=3) * 1.6).astype(np.float32))
        cmd = (synthetic_actions(range(N), t, seed=3) * 1.6).astype(np.float32)
        st0 = env.state
        caches = [env.contacts(i) for i in range(N)]
        env.step(cmd)
        st1, rec = env.state, env.host(nat.F_PREP).astype(np.float64)
        assert (env.host(nat.F_ERRFLAGS) == 0).all()
        new = [env.contacts(i) for i in range(N)]
        robot = [i for i in range(N) if ((new[i][:, 0] >= 0) & (new[i][:, 0] < 16)).any()]
        free = [i for i in range(N) if i not in robot]
        picks = sorted(robot, key=lambda i: -len(new[i]))[:3] + free[:2]
        for i in picks:
            cd = new[i]
            res = na.step(st0[i].astype(np.float64), cmd[i].astype(np.float64), cd, dyn=dyn, prev=caches[i], **kw)
            # RR_F_PREP of an in-line preparation (no look-ahead on these paths) describes the state the step started from
            qd = np.abs(st0[i][11:22].astype(np.float64)).max()
            bterm = np.abs(ns.DT * res['prep']['Minv'] @ res['prep']['bias']).max()
            rq = np.abs(rec[i, S_QDS:S_OR] - res['qds']) / (2e-4 + 2e-6 * qd + 5e-5 * bterm)
            print("  t %d env %d (%d contacts): qd* worst / ceiling %.3f" % (t, i, len(cd), rq.max()))
            assert rq.max() < 1.0, (prep, t, i, rq)
            assert np.abs(res['qds'] - res['prep']['qds']).max() > 1e-3 or qd < 1e-2, "the per-joint damping does not show in qd*"
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
                    r = na.step(ulp(st0[i]).astype(np.float64), cmd[i].astype(np.float64), cdp, dyn=dyn, prev=caches[i], **kw)
                    dd = _dev(r['state'], res['state']) + (float(np.abs(r['lambda_n'] / ns.DT - f_np).max()) if len(cd) else 0.0,)
                    sp = [max(a, b) for a, b in zip(sp, dd)]
                bb = tuple(max(x, SENS_FACTOR * y) for x, y in zip(flat, sp))
            print("  t %d env %d: deviation %s, bounds %s" % (t, i, d, bb))
            assert all(x <= y for x, y in zip(d, bb)), (prep, t, i, d, bb)
            worst = max(worst, max(x / y for x, y in zip(d, flat)))
            checked += 1
            with_robot += i in robot
            without += i in free
            # joint 1's motor sits on its own, lower clamp in the helper: the per-joint clamp is exercised
            clamp = kw['max_force'] * ns.DT
            saturated += abs(abs(res['lam'][1]) - clamp[1]) == 0.0
            assert (np.abs(res['lam'][:NJ]) <= clamp).all()
    print("%s: %d checks (%d with robot contacts, %d without), joint 1 saturated in %d; worst deviation / flat bound %.3f"
          % (prep, checked, with_robot, without, saturated, worst))
    assert with_robot >= 3 and without >= 3 and saturated >= 1
    env.close()
