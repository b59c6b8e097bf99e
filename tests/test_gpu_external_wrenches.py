"""GPU tests (-m gpu) of the step's external wrenches (rr_set_external_wrenches; k_ext_wrench, csrc/rr_wrench.inc): one step against the
float64 numpy step with the wrench applied (tests/numpy_wrench.py), negative controls on the reference side, bit-for-bit neutrality
when unused, the launch point against an in-line twin, hovering objects, weight cancellation on the arm, persistence and masks.
N = 5 is one ragged 16-env workgroup of the wrench kernel (and a full plus a ragged 4-env workgroup of the preparation), N = 70
several workgroups of both and of the split placements."""
import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_actuators as na
from tests import numpy_collide as ncl
from tests import numpy_step as ns
from tests import numpy_torque as nt
from tests import numpy_wrench as nw
from tests.test_gpu_contacts_fuzz import state_bounds, SENS_FACTOR, SENS_RUNS, _grasp_script
from tests.test_gpu_joint_torques import motors_off, gravity_scale
from tests.test_gpu_numpy_step import random_dynamics, _dev, force_bound
from tests.test_gpu_round6 import _make, S_BR, S_QDS, S_OR, S_OVS, S_OWS, S_OP, S_TOTAL
from tests.test_numpy_wrench import nw_controls, control_ratio

pytestmark = pytest.mark.gpu

W = H = 64
NJ, NB = 11, 11
XW = nat.XW_BODIES
MAX_FORCE = ns.SOLVER_DEFAULTS['motor_max_force']
PLAIN = {'RR_NO_LOOKAHEAD': '1', 'RR_NO_SPLIT': '1'}
ALL = dict(joint_pos=True, joint_vel=True, obj_pose=True, obj_vel=True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _record_fields(rec):
    """qd* [N, 11], v* [N, 3, 3], w* [N, 3, 3] of RR_F_PREP rows."""
    N = len(rec)
    return dict(qds=rec[:, S_QDS:S_OR], ovs=rec[:, S_OVS:S_OVS + 9].reshape(N, 3, 3), ows=rec[:, S_OWS:S_OWS + 9].reshape(N, 3, 3))


def _applied_step(state, cmd, contacts, w, dyn, mode, kw):
    with nw.applied(w, dyn, mode):
        return na.step(np.asarray(state).astype(np.float64), cmd.astype(np.float64), contacts, **kw)


@pytest.mark.parametrize('N', [5, 70])
def test_one_step_against_the_float64_step_and_the_wrong_features_miss(monkeypatch, N):
    """One step with a wrench table (numpy_wrench.case_inputs: forces within +-3 x the body's weight, torques within +-3 x weight x
    0.05 m; env 2 all zero, env 3 robot rows only, env 4 one object row only) from states of test_gpu_numpy_step's edge_states with
    per-env object dynamics (random_dynamics), motors off on a random subset of joints per env, on a RR_NO_LOOKAHEAD handle (the
    preparation record read after the step is this step's).  A twin handle that never sets a wrench is given the same state.
    (a) RR_F_PREP's qd* against numpy's qd* + dt M^-1 tau at numpy_torque.qds_ceiling with the generalised force in tau's place; v* and
        w* at test_gpu_numpy_step's 1e-6 (1 + |v|) widened to 1e-6 (1 + |v| + |added term|).  The untouched targets -- everything of
        env 2, v* / w* of env 3, qd* and the other objects of env 4, and every field the kernel does not write, of every env -- are
        equal BIT FOR BIT to the twin's record.
    (b) The stepped state of the checked envs (all at N = 5; eight at N = 70) against tests/numpy_actuators.step under
        numpy_wrench.applied, through test_gpu_numpy_step's comparison: state_bounds / force_bound, over a flat bound SENS_FACTOR x
        the reference's own one-ulp spread; at most (N + 7) // 8 edge envs may have diverged, as in test_gpu_joint_torques.py.
    (c) Every control of numpy_wrench (negated, mass, no_arm, no_ancestors, model_mass) and the previous step's table ("one step
        late") misses (a) on every env whose relevant rows are non-zero.
    Measured on the MI355X (none raised; NOTEBOOK.md, "External wrenches on robot bodies and objects"), N = 5 / 70: qd* 0.107 / 0.223,
    v* 0.046 / 0.070, w* 0.104 / 0.190 of the ceilings; the controls' smallest ratio x322 (no_ancestors, N = 70)."""
    envs = [_make(monkeypatch, {'RR_NO_LOOKAHEAD': '1'}, N, objects=3, width=W, height=H) for _ in range(2)]
    env, twin = envs
    st_in, dyn, w_prev, w = nw.case_inputs(N)
    off = motors_off(N, 21)
    max_force = np.where(off, 0.0, MAX_FORCE).astype(np.float32)
    cmd0 = (synthetic_actions(range(N), 0, seed=3) * 1.6).astype(np.float32)
    cmd = (synthetic_actions(range(N), 1, seed=3) * 1.6).astype(np.float32)
    for e in envs:
        e.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(dyn))
        e.set_env_actuators(max_force=max_force)
        e.state = st_in
    env.set_external_wrenches(w_prev)
    env.step(cmd0)
    twin.step(cmd0)
    st0 = env.state
    caches = [env.contacts(i) for i in range(N)]
    env.set_external_wrenches(w)
    assert np.array_equal(_bits(env.external_wrenches()), _bits(w))
    twin.write_state(st0, **ALL)                      # (the twin's own contact history stays: the preparation does not read it)
    env.step(cmd)
    twin.step(cmd)
    st1, rec32, flags = env.state, env.host(nat.F_PREP), env.host(nat.F_ERRFLAGS)
    rec_twin = twin.host(nat.F_PREP)
    new = [env.contacts(i) for i in range(N)]
    for e in envs:
        e.close()
    live = (flags == 0) & np.isfinite(st0).all(1) & np.isfinite(st1).all(1)
    assert live.sum() >= N - (N + 7) // 8, "more than the fastest edge envs diverged: %s" % np.flatnonzero(~live)
    robot, obj = (w[:, :NB] != 0).any((1, 2)), (w[:, NB:] != 0).any(2)
    assert not robot[2] and not obj[2].any() and robot[3] and not obj[3].any() and not robot[4] and obj[4].tolist() == [False, True, False]

    # (a) bit for bit where nothing was to be added
    bt, bm = _bits(rec_twin), _bits(rec32)
    assert rec32.shape == (N, S_TOTAL)
    for lo, hi in ((S_BR, S_QDS), (S_OR, S_OVS), (S_OP, S_TOTAL)):
        assert np.array_equal(bm[live, lo:hi], bt[live, lo:hi]), (lo, hi)
    assert np.array_equal(bm[live & ~robot, S_QDS:S_OR], bt[live & ~robot, S_QDS:S_OR])
    for i in range(3):
        keep = live & ~obj[:, i]
        for s in (S_OVS, S_OWS):
            assert np.array_equal(bm[keep, s + 3 * i:s + 3 * i + 3], bt[keep, s + 3 * i:s + 3 * i + 3]), (i, s)
    assert not np.array_equal(bm[live & robot, S_QDS:S_OR], bt[live & robot, S_QDS:S_OR])
    # (a) the touched fields against float64, vectorised
    d64, w64 = dyn.astype(np.float64), w.astype(np.float64)
    pr = ns.prep(st0.astype(np.float64), d64)
    want = nw.add_to(pr, w64, d64)
    ceil = nw.prep_ceilings(pr, st0, w64, d64)
    got = _record_fields(rec32.astype(np.float64))
    rq, rv, rw = (np.abs(got[k] - want[k]) / c for k, c in zip(('qds', 'ovs', 'ows'), ceil))
    print("N=%d: worst |device - numpy| / ceiling: qd* %.3f, v* %.3f, w* %.3f" % (N, rq[live].max(), rv[live].max(), rw[live].max()))
    assert rq[live].max() < 1.0 and rv[live].max() < 1.0 and rw[live].max() < 1.0, (rq.max(1), rv.max((1, 2)), rw.max((1, 2)))
    # (c) the controls miss (a) on every env whose relevant rows are non-zero
    for name, rel in nw_controls(robot, obj.any(1)).items():
        late = name == 'one step late'
        other = nw.add_to(pr, w_prev.astype(np.float64) if late else w64, d64, 'applied' if late else name)
        r = control_ratio(got, other, ceil)
        print("N=%d: control '%s': worst ratio per env, the smallest over its envs %.1f" % (N, name, r[live & rel].min()))
        assert (r[live & rel] > 1.0).all(), (name, np.flatnonzero(live & rel & (r <= 1.0)))

    # (b) the stepped state of the checked envs
    rng = np.random.default_rng(1)
    touching = [i for i in range(N) if live[i] and ((new[i][:, 0] >= 0) & (new[i][:, 0] < 16)).any()]
    picks = list(range(N)) if N <= 8 else sorted(set([0, 2, 3, 4, N - 1] + sorted(touching, key=lambda i: -len(new[i]))[:3] + [i for i in range(N) if i % 16 == 5]))[:8]
    worst, checked, shown = 0.0, 0, 0
    for i in [i for i in picks if live[i]]:
        cd = new[i]
        kw = dict(dyn=d64[i], prev=caches[i], max_force=max_force[i].astype(np.float64))
        run = lambda t, mode='applied', s=st0[i], c=cd: _applied_step(s, cmd[i], c, t, d64[i], mode, kw)
        res = run(w64[i])
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
                r = run(w64[i], s=ulp(st0[i]), c=cdp)
                dd = _dev(r['state'], res['state']) + (float(np.abs(r['lambda_n'] / ns.DT - f_np).max()) if len(cd) else 0.0,)
                sp = [max(a, b) for a, b in zip(sp, dd)]
            bb = tuple(max(x, SENS_FACTOR * y) for x, y in zip(flat, sp))
        print("  N=%d env %d (%d contacts): deviation %s, bounds %s" % (N, i, len(cd), d, bb))
        assert all(x <= y for x, y in zip(d, bb)), (N, i, d, bb)
        worst = max(worst, max(x / y for x, y in zip(d, flat)))
        checked += 1
        # the plain step is the result where no row is set; elsewhere the wrench shows in it (unless a contact takes it up: an object
        # pressed onto the table moves no more than without the force -- the record's fields, (c), are where every env is judged)
        miss = max(x / y for x, y in zip(_dev(st1[i], run(np.zeros((XW, 6)))['state']), bb))
        if robot[i] or obj[i].any():
            shown += miss > 1.0
        else:
            assert miss <= 1.0, (N, i, miss)
    print("N=%d: %d envs stepped against numpy (%d with robot contacts); worst deviation / flat bound %.3f" % (N, checked, len([i for i in picks if i in touching]), worst))
    assert checked >= min(N, 5) - 1 and shown >= 2


def test_nothing_changes_when_unused():
    """Four handles, 30 steps of synthetic_actions: A never calls the feature, B set a table and cleared it, C holds an all-zero
    table with the feature on, D a non-zero table masked to env 2 alone.  A, B and C agree bit for bit in state, images and contact
    records after every step; D agrees on every env but env 2 (envs are independent), where the wrench shows."""
    N = 5
    A, B, C, D = (BatchedREALRobotEnv(N, objects=3, width=W, height=H) for _ in range(4))
    table = nw.random_wrenches(N, 5)
    B.set_external_wrenches(table)
    B.set_external_wrenches(None)
    assert not B.external_wrenches().any()
    C.set_external_wrenches(np.zeros((N, XW, 6), np.float32))
    C.set_external_wrenches(-np.zeros(6, np.float32), env_mask=np.array([0, 1, 0, 0, 1], np.uint8))        # (negative zeros are zeros)
    D.set_external_wrenches(table, env_mask=np.array([0, 0, 1, 0, 0], np.uint8))
    fields = (nat.F_STATE, nat.F_TOUCH, nat.F_CONTACT_COUNT, nat.F_CONTACTS, nat.F_ERRFLAGS)
    others = np.arange(N) != 2
    for s in range(30):
        cmd = synthetic_actions(range(N), s, seed=7).astype(np.float32)
        render = s % 10 == 9
        for e in (A, B, C, D):
            e.step(cmd, render=render)
        for f in fields + ((nat.F_RGB, nat.F_DEPTH) if render else ()):
            a, b, c, d = (np.ascontiguousarray(e.host(f)) for e in (A, B, C, D))
            a, b, c, d = (x.reshape(N, -1).view(np.uint8) for x in (a, b, c, d))
            assert np.array_equal(a, b), (s, f)
            assert np.array_equal(a, c), (s, f)
            if f != nat.F_CONTACTS:               # (rows past an env's count are not part of its record)
                assert np.array_equal(a[others], d[others]), (s, f)
    assert not np.array_equal(_bits(A.state[2]), _bits(D.state[2]))           # (the wrench acted on env 2)
    for i in np.flatnonzero(others):
        assert np.array_equal(_bits(A.contacts(i)), _bits(D.contacts(i)))
    for e in (A, B, C, D):
        e.close()


def test_look_ahead_and_placement_against_the_in_line_twin(monkeypatch):
    """The launch point.  The default handle (look-ahead, split placements) and a twin with RR_NO_LOOKAHEAD and RR_NO_SPLIT get the
    same table sequence, rewritten every step for 20 steps, alternately from host arrays and through the device buffer (the default
    handle; the twin from host arrays), N = 70 with every fourth env closing the gripper on the cube (the fuzz tests' grasp script:
    heavy envs, so split placements occur), motors off on random joints, render on for a third of the steps: state, touch sensors
    and contact records are equal bit for bit after every step.  Then 20 more steps with joint torques also on.  (RR_F_PREP itself
    cannot be compared between the two: after a step the look-ahead handle's record is already the NEXT step's preparation.)  A
    wrench kernel that ran before the look-ahead had landed, or beside a solve, shows here."""
    import torch
    N, T = 70, 20
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b = _make(monkeypatch, PLAIN, N, objects=3, width=W, height=H)
    script = _grasp_script()
    grasp = np.arange(N) % 4 == 1
    t0 = 280                                    # the script closes the gripper on the cube from step 270 on
    assert len(script) >= t0 + 2 * T
    for s in range(t0):
        cmd = (synthetic_actions(range(N), s, seed=3) * 1.6).astype(np.float32)
        cmd[grasp] = script[s]
        a.step(cmd)
        b.step(cmd)
    assert np.array_equal(_bits(a.state), _bits(b.state))
    off = motors_off(N, 23)
    off[grasp] = False
    off[grasp, 6] = True
    for e in (a, b):
        e.set_env_actuators(max_force=np.where(off, 0.0, MAX_FORCE).astype(np.float32))
    a.set_external_wrenches(np.zeros((N, XW, 6), np.float32))      # the feature on: the buffer writes below count
    view = torch.from_dlpack(a.external_wrench_buffer)
    assert tuple(view.shape) == (N, XW, 6) and view.dtype == torch.float32
    ptr = view.data_ptr()
    classes = set()
    scale = gravity_scale() / 3.0
    rng = np.random.default_rng(9)
    for s in range(t0, t0 + 2 * T):
        cmd = (synthetic_actions(range(N), s, seed=3) * 1.6).astype(np.float32)
        cmd[grasp] = script[s]
        w = (nw.random_wrenches(N, 1000 + s) / 9.0).astype(np.float32)          # (within a third of the weights: the grasp survives)
        w[rng.random(N) < 0.2] = 0.0              # zero envs come and go
        w[rng.random(N) < 0.2, :NB] = 0.0         # ... and envs with object rows only
        if s % 2:
            a.sync()
            view.copy_(torch.from_numpy(w).cuda())
            torch.cuda.synchronize()
        else:
            a.set_external_wrenches(w)
        b.set_external_wrenches(w)
        if s >= t0 + T:                           # joint torques too: the torque term first, then the wrench term, on both
            tau = (rng.uniform(-1, 1, (N, NJ)) * scale).astype(np.float32)
            a.set_joint_torques(tau)
            b.set_joint_torques(tau)
        render = s % 3 == 0
        a.step(cmd, render=render)
        b.step(cmd, render=render)
        sa, sb = a.state, b.state
        assert np.array_equal(_bits(sa), _bits(sb)), (s, np.flatnonzero((_bits(sa) != _bits(sb)).any(1)))
        assert np.array_equal(_bits(a.host(nat.F_TOUCH)), _bits(b.host(nat.F_TOUCH))), s
        assert np.array_equal(a.host(nat.F_CONTACT_COUNT), b.host(nat.F_CONTACT_COUNT)), s
        for i in (1, 5, N - 1):
            assert np.array_equal(_bits(a.contacts(i)), _bits(b.contacts(i))), (s, i)
        assert np.array_equal(_bits(a.external_wrenches()), _bits(w)), s
        classes |= set(a.host(nat.F_ENV_CLASS).tolist())
    assert torch.from_dlpack(a.external_wrench_buffer).data_ptr() == ptr        # the pointer never changes
    assert np.array_equal(a.host(nat.F_RGB), b.host(nat.F_RGB))
    assert len(classes) >= 2, classes           # (heavy envs were in play: the split placements ran)
    a.close()
    b.close()


HOVER_STEPS = 50
HOVER_POS = np.array([[0.0, -0.35, 1.5], [0.0, 0.0, 1.5], [0.0, 0.35, 1.5]])


def _hover_state(st):
    st = st.copy()
    ob = st[:, 22:61].reshape(len(st), 3, 13)
    ob[:, :, :3], ob[:, :, 3:7], ob[:, :, 7:] = HOVER_POS, [0, 0, 0, 1], 0.0
    st[:, 22:61] = ob.reshape(len(st), 39)
    return st


@pytest.mark.parametrize('N', [5, 70])
def test_objects_hover_under_their_own_weight_and_not_under_the_models(N):
    """Weight cancellation on the objects.  The three objects are teleported to rest in free space (1.5 m up over the table, 0.55 m beside the arm's axis: the
    float64 reference -- tests/numpy_collide.collide on the states of a 50-step numpy rollout under the same wrench -- reports no
    contact of an object there, checked below on the CPU), per-env masses x 0.2-5 (random_dynamics), F = float32(m_env g) z.
    Over 50 steps every object's displacement stays below 1e-4 of the reference's free-fall distance 1/2 g (50 dt)^2 = 0.3066 m,
    i.e. below 3.07e-5 m.  Why float32 reaches that with room to spare: per step the preparation subtracts fl(dt g) and the kernel
    adds fl(fl(dt F) / m), each within a few units of 6e-8 relative of dt g = 0.049: a velocity residue of at most ~1e-8 m/s per
    step, < 5e-7 m/s after 50 steps, hence < 50 x 0.005 x 5e-7 = 1.3e-7 m -- more than 100 times below the ceiling.
    A second handle given the MODEL's mass (F = float32(m_model g)) drifts past that ceiling on every object of every env: 1/2 g
    |m_model / m_env - 1| (50 dt)^2."""
    dyn = random_dynamics(N, 15)
    g = ns.GRAVITY
    ceiling = 1e-4 * 0.5 * g * (HOVER_STEPS * ns.DT) ** 2
    model_mass = ns.default_dynamics()[:, 0]
    drift = {}
    cmd = np.zeros((N, 9), np.float32)
    for which in ('env', 'model'):
        env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
        env.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(dyn))
        st0 = _hover_state(env.state)
        env.write_state(st0, obj_pose=True)
        mass = dyn[:, :, 0].astype(np.float64) if which == 'env' else np.broadcast_to(model_mass, (N, 3))
        w = {name: np.stack([np.zeros(N), np.zeros(N), (mass[:, i] * g).astype(np.float32)] + [np.zeros(N)] * 3, 1) for i, name in enumerate(env.object_names)}
        env.set_external_wrenches(w)
        if which == 'env':
            table = env.external_wrenches()
            assert np.array_equal(_bits(table[:, NB:, 2]), _bits((dyn[:, :, 0].astype(np.float64) * g).astype(np.float32))) and not table[:, :NB].any()
        worst = np.zeros((N, 3))
        for s in range(HOVER_STEPS):
            env.step(cmd)
            worst = np.maximum(worst, np.abs(env.state[:, 22:61].reshape(N, 3, 13)[:, :, :3] - HOVER_POS).max(2))
        assert (env.host(nat.F_ERRFLAGS) == 0).all()
        if which == 'env':
            assert not any((env.contacts(i)[:, :2] >= 16).any() for i in range(N)), "a hovering object touches something"
            first_state, table0 = st0[0], table[0]
        drift[which] = worst
        env.close()
    print("N=%d hover: worst displacement %.3g m = %.3g of the ceiling %.3g m; with the model's mass the smallest %.3g m = %.1f ceilings"
          % (N, drift['env'].max(), drift['env'].max() / ceiling, ceiling, drift['model'].min(), drift['model'].min() / ceiling))
    assert (drift['env'] < ceiling).all(), drift['env'].max(1)
    differs = np.abs(dyn[:, :, 0] / model_mass - 1.0) > 1e-3
    assert differs.all()
    assert (drift['model'][differs] > ceiling).all(), drift['model'].min(1)
    # the place is free in the float64 reference: env 0's rollout under its wrench, collided at every step
    s = first_state.astype(np.float64)
    for _ in range(HOVER_STEPS):
        rec = ncl.collide(s)['records']
        assert not (rec[:, :2] >= 16).any(), "the reference reports a contact of a hovering object"
        with nw.applied(table0.astype(np.float64), dyn[0].astype(np.float64)):
            s = ns.step(s, np.zeros(9), rec, dyn=dyn[0].astype(np.float64))['state']
    assert np.abs(s[22:61].reshape(3, 13)[:, :3] - HOVER_POS).max() < ceiling / 100


def test_weight_cancellation_holds_the_arm(monkeypatch):
    """F_b = m_b g z on all eleven robot bodies is gravity compensation at every posture.  N = 5 at numpy_torque.HOLD_POSTURES, motors
    off on all joints (set_env_actuators(max_force=0)): over HOLD_STEPS steps the arm's drift is at most HOLD_RATIO x the drift of a
    second handle without wrenches.  And after one step on RR_NO_LOOKAHEAD handles the record's qd* agrees, within
    numpy_torque.qds_ceiling, with a twin driven by set_joint_torques(posture_dynamics()['gravity'])."""
    N = 5
    q0 = nt.HOLD_POSTURES[np.arange(N) % len(nt.HOLD_POSTURES)].astype(np.float32)
    weights = (ns.model()['body_mass'] * ns.GRAVITY).astype(np.float32)
    w = np.zeros((N, XW, 6), np.float32)
    w[:, :NB, 2] = weights

    def posed(env):
        st = env.state
        st[:, :NJ], st[:, NJ:2 * NJ] = q0, 0.0
        env.write_state(st, joint_pos=True, joint_vel=True)
        return st
    drifts = []
    for hold in (True, False):
        env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
        env.set_env_actuators(max_force=0.0)
        posed(env)
        if hold:
            env.set_external_wrenches(w)
        worst = np.zeros(N)
        for s in range(nt.HOLD_STEPS):
            env.step(None)
            worst = np.maximum(worst, np.abs(env.state[:, :NJ] - q0).max(1))
        assert (env.host(nat.F_ERRFLAGS) == 0).all()
        if hold:
            touching = sum(int(((c[:, 0] >= 0) & (c[:, 0] < 16)).any()) for c in (env.contacts(i) for i in range(N)))
            assert touching == 0, "a held arm touches something: the postures are chosen free"
        drifts.append(worst)
        env.close()
    held, free = drifts
    print("drift over %d steps: held %s, free %s, worst ratio %.3g" % (nt.HOLD_STEPS, held, free, (held / free).max()))
    assert (free > 0.1).all()
    assert (held <= nt.HOLD_RATIO * free).all(), (held, free)
    # one step: the wrench's generalised force is the gravity torque
    recs = []
    for how in ('wrench', 'torque'):
        env = _make(monkeypatch, {'RR_NO_LOOKAHEAD': '1'}, N, objects=3, width=W, height=H)
        env.set_env_actuators(max_force=0.0)
        st = posed(env)
        if how == 'wrench':
            env.set_external_wrenches(w)
        else:
            env.set_joint_torques(env.posture_dynamics()['gravity'])
        env.step(None)
        recs.append(env.host(nat.F_PREP)[:, S_QDS:S_OR].astype(np.float64))
        env.close()
    pr = ns.prep(st.astype(np.float64), np.broadcast_to(ns.default_dynamics(), (N, 3, 8)))
    tau = nw.generalised_force(pr, w.astype(np.float64))
    assert np.abs(tau - pr['bias']).max() < 1e-4 * np.abs(pr['bias']).max()          # (at rest the bias is the gravity torque)
    ceil = nt.qds_ceiling(pr, np.zeros((N, NJ)), tau)
    r = np.abs(recs[0] - recs[1]) / ceil
    print("one step, wrench against gravity torques: worst |qd* - qd*| / ceiling %.3f" % r.max())
    assert r.max() < 1.0, r.max(1)


def test_persistence_masks_and_the_zero_copy_buffer():
    """The table survives reset, a device-mask reset, write_state, fork, save_snapshot / load_snapshot, restore and an episode's
    auto-reset; env_mask changes only its envs; external_wrenches() returns the bits given; a non-finite host row raises and changes
    nothing; a device tensor is taken in place; a device-side write into external_wrench_buffer, made in stream order, acts in the
    next step like the same table set by the call; the vector env forwards "external_wrenches"."""
    import torch
    from tests.test_gpu_episode import _home, _table
    N = 5
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    assert env.L.rr_set_external_wrenches(env.h, None, 0, None, 0) == 0        # zeroing a table that never was
    assert not env.external_wrenches().any()                                    # a fresh handle
    assert env.wrench_row_names()[NB:] == ['cube', 'tomato', 'mustard'] and len(env.wrench_row_names()) == XW
    tab = nw.random_wrenches(N, 41)
    env.set_external_wrenches(tab)
    same = lambda: np.array_equal(_bits(env.external_wrenches()), _bits(tab))
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
    env.save_snapshot(0)
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
    # masks: only the masked envs' rows change, from either side; None zeroes the masked rows
    t2 = nw.random_wrenches(N, 42)
    m = np.array([0, 1, 1, 0, 0], np.uint8)
    env.set_external_wrenches(t2, env_mask=m)
    tab[m != 0] = t2[m != 0]
    assert same()
    t3 = nw.random_wrenches(N, 43)
    m = np.array([1, 0, 0, 0, 1], bool)
    env.set_external_wrenches(_cuda(t3), env_mask=_cuda(m))
    tab[m] = t3[m]
    assert same()
    env.set_external_wrenches(None, env_mask=np.array([0, 0, 1, 0, 0], np.uint8))
    tab[2] = 0.0
    assert same()
    env.set_external_wrenches({'tomato': [1, 2, 3, 4, 5, 6], 3: -np.ones(6)}, env_mask=np.array([0, 0, 0, 1, 0], np.uint8))
    tab[3] = 0.0
    tab[3, 12], tab[3, 3] = [1, 2, 3, 4, 5, 6], -1.0
    assert same()
    # refusals change nothing
    bad = t2.copy()
    bad[3, 12, 4] = np.inf
    with pytest.raises(ValueError):
        env.set_external_wrenches(bad)
    assert env.L.rr_set_external_wrenches(env.h, bad.ctypes.data, 0, None, 0) == -1
    assert 'env 3, row 12, entry 4' in env.L.rr_last_error().decode() and 'not finite' in env.L.rr_last_error().decode()
    assert env.L.rr_set_external_wrenches(env.h, bad.ctypes.data, 0, m.astype(np.uint8).ctypes.data, 1) == -1 and 'same side' in env.L.rr_last_error().decode()
    assert same()
    # (the non-finite row outside the mask is not looked at)
    env.set_external_wrenches(bad, env_mask=np.array([1, 0, 0, 0, 0], np.uint8))
    tab[0] = bad[0]
    assert same()

    # the zero-copy buffer: a device-side write in stream order acts in the next step, like the same table set by the call
    twin = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    plain = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    for e in (env, twin, plain):
        e.set_episode(0, 1)
        e.reset()
        e.set_env_actuators(max_force=np.where(motors_off(N, 3), 0.0, MAX_FORCE).astype(np.float32))
    t4 = nw.random_wrenches(N, 44)
    t4[1] = 0.0
    dev = _cuda(t4)
    twin.set_external_wrenches(dev)                                    # a device tensor, taken in place
    env.sync()
    view = torch.from_dlpack(env.external_wrench_buffer)
    ptr = view.data_ptr()
    assert tuple(view.shape) == (N, XW, 6) and view.dtype == torch.float32
    view.copy_(dev)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(env.external_wrenches()), _bits(t4)) and np.array_equal(_bits(twin.external_wrenches()), _bits(t4))
    for s in range(3):
        for e in (env, twin, plain):
            e.step(cmd(10 + s))
    assert np.array_equal(_bits(env.state), _bits(twin.state))
    diff = (_bits(plain.state) != _bits(env.state)).any(1)
    assert diff[[0, 2, 3, 4]].all() and not diff[1]                     # the wrench acted; the zero env is the plain step
    env.set_external_wrenches(None)                                      # off: the buffer stays where it is, its writes wait
    assert torch.from_dlpack(env.external_wrench_buffer).data_ptr() == ptr and not env.external_wrenches().any()
    for e in (env, twin, plain):
        e.close()


def test_vector_env_forwards_external_wrenches():
    from real_robots_amd.vector import REALRobotVectorEnv
    N = 5
    v = REALRobotVectorEnv(N, eye_width=W, eye_height=H, render_every_step=False, external_wrench_actions=True)
    assert v.action_space.spaces['external_wrenches'].shape == (N, XW, 6) and v.single_action_space.spaces['external_wrenches'].shape == (XW, 6)
    v.reset()
    tab = nw.random_wrenches(N, 51)
    v.step({"joint_command": np.zeros((N, 9), np.float32), "external_wrenches": tab})
    assert np.array_equal(_bits(v._be.external_wrenches()), _bits(tab))
    v.step({"joint_command": np.zeros((N, 9), np.float32)})             # absent: the table is kept
    v.step(np.zeros((N, 9), np.float32))
    assert np.array_equal(_bits(v._be.external_wrenches()), _bits(tab))
    v.close()
    d = REALRobotVectorEnv(N, eye_width=W, eye_height=H, render_every_step=False)
    assert list(d.action_space.spaces) == ['joint_command', 'render'] and list(d.single_action_space.spaces) == ['joint_command', 'render']
    d.close()
