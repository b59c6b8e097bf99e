"""GPU tests (-m gpu) of the device-resident macro actions (rr_step_macro, include/realrobot.h): the re-plan decision of
REALRobotEnv.step_macro taken on the device, and the planner over the compact list of needing envs (k_macro_replan), whose plans must be
k_plan_macro's bit for bit.  N = 67 is neither a multiple of 64 nor of the 16 slots of a planner wave."""
import numpy as np
import pytest
import torch

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.vector import REALRobotVectorEnv
from oracle.kinematics import generate_plan, ik_candidates, plan_way_points, quat_from_euler

pytestmark = pytest.mark.gpu
N = 67
LOW, HIGH = np.array([-0.25, -0.5] * 2, np.float32), np.array([0.05, 0.5] * 2, np.float32)      # macro_space, env.py:49-52
ORIENT = quat_from_euler(0, 3.14, -1.57)
IK_TOL = 1e-3       # tests/test_gpu_ik_macro.py: device (float32) vs checker (float64) on the same branch, both converged


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')
    torch.cuda.synchronize()
    return t


def requests(rng, n=N):
    return rng.uniform(LOW, HIGH, size=(n, 4)).astype(np.float32)


def make(n=N, **kw):
    return BatchedREALRobotEnv(n, objects=3, width=64, height=64, **kw)


def scatter_postures(env, seed):
    """Every env at a posture of its own (and at rest), so that the plans depend on the env's present joints."""
    rng = np.random.default_rng(seed)
    s = env.state
    s[:, :7] = rng.uniform(-0.8, 0.8, size=(env.N, 7)).astype(np.float32)
    s[:, 7:22] = 0.0
    env.write_state(s, joint_pos=True, joint_vel=True)


def perimeter_requests(n=N):
    """The 36 perimeter pairs of tests/test_gpu_ik_macro.py (the six with p1 == p2 among them), the two farthest corners of macro_space
    in both directions (the 21-piece sweep), two more p1 == p2 points, and seeded draws up to N."""
    perimeter = [(a, b) for a in (-0.25, 0.05) for b in (-0.5, 0.0, 0.5)]
    pairs = [p1 + p2 for p1 in perimeter for p2 in perimeter]
    pairs += [(-0.25, -0.5, 0.05, 0.5), (0.05, 0.5, -0.25, -0.5), (-0.25, 0.5, 0.05, -0.5), (-0.1, 0.2, -0.1, 0.2), (0.0, -0.3, 0.0, -0.3)]
    m = np.array(pairs, np.float32)
    return np.concatenate([m, requests(np.random.default_rng(11), n - len(m))])


def test_twin_run_host_path_and_device_path():
    """Handle A: step_macro (host bookkeeping); handle B: step_macro_device with CUDA tensors.  State, positions and `replanned` bit for
    bit after every step; every env's plan after the steps that planned."""
    A, B = make(), make()
    for e in (A, B):
        scatter_postures(e, 5)
    rng = np.random.default_rng(2)
    m = requests(rng)
    z, u = 3, 4                       # z: a component goes 0.0 -> -0.0 at step 4 (no re-plan); u: never changes
    m[z, 1] = 0.0
    others = np.array([i for i in range(N) if i not in (z, u)])
    keep = []
    for t in range(40):
        if t in (3, 7):
            pick = rng.choice(others, N // 3, replace=False)
            m[pick] = requests(rng, len(pick))
        if t == 4:
            m[z, 1] = -0.0
            assert np.signbit(m[z, 1])
        idle = (rng.random(N) < 0.3) if 5 <= t <= 9 else np.zeros(N, bool)
        if 5 <= t <= 9:
            idle[u] = False
        if t == 0:
            need = ~idle
        else:
            need = ((~np.all(m.astype(np.float64) == A._macro_req, axis=1)) | (A._macro_step >= 1000)) & ~idle
        A.step_macro([None if idle[i] else m[i].reshape(2, 2) for i in range(N)] if idle.any() else m.reshape(N, 2, 2).copy())
        md, idl = dev(m.reshape(N, 2, 2)), dev(idle) if idle.any() else None
        keep.append((md, idl))
        B.step_macro_device(md, idle=idl)
        assert same_bits(A.state, B.state), t
        assert np.array_equal(B.macro_buffer('position', host=True), A._macro_step.astype(np.int32)), t
        rp = B.macro_buffer('replanned', host=True)
        assert np.array_equal(rp, need.astype(np.uint8)), (t, np.flatnonzero(rp != need))
        if t == 0:
            assert rp.all()
        if t == 4:
            assert rp[z] == 0 and not need.any()
        if t in (3, 7):
            assert 0 < rp.sum() < N and rp[u] == 0
        if t in (0, 3, 7):
            pb = B.macro_buffer('plan', host=True)
            for i in range(N):
                assert same_bits(A.get_plan(i), pb[i]), (t, i)
                assert same_bits(B.get_plan(i), pb[i]), (t, i)
    req = B.macro_buffer('request', host=True)
    assert same_bits(req, m) or (np.array_equal(req, m) and np.signbit(req[z, 1]) != np.signbit(m[z, 1]))      # z keeps the +0.0 it planned for
    assert not np.signbit(req[z, 1])
    A.close(), B.close()


@pytest.mark.parametrize('n,single', [(N, False), (N, True), (1100, False), (4099, False)])
def test_replan_kernel_equals_plan_macro_bit_for_bit(n, single):
    """k_plan_macro and k_macro_replan on ONE handle from identical states (a snapshot slot): all plans bit for bit.  67 envs: a wave
    per listed env; 1100 and 4099: more listed envs than the planner gives a wave each -- two and five envs share a wave, the last
    wave is not full."""
    N = n
    env = make(N, solver={'ik_single_seed': single})
    scatter_postures(env, 9)
    env.snapshot_slots(1)
    m = perimeter_requests(N)
    env.plan_macro(m.reshape(N, 2, 2))
    ref = env.macro_buffer('plan', host=True)
    for i in (0, 40, N - 1):
        assert same_bits(env.get_plan(i), ref[i])
    assert np.isfinite(ref).all()
    # the plan buffer is shared: clobber it, so that every row read below was written by the device path
    env.sync()
    torch.from_dlpack(env.macro_buffer('plan')).fill_(float('nan'))
    torch.cuda.synchronize()
    assert np.isnan(env.get_plan(N - 1)).all()
    env.load_snapshot(0)
    env.macro_invalidate()
    md = dev(m)
    env.step_macro_device(md)
    got = env.macro_buffer('plan', host=True)
    assert env.macro_buffer('replanned', host=True).all()
    bad = np.flatnonzero((bits(got) != bits(ref)).reshape(N, -1).any(axis=1))
    assert not bad.size, (bad, [float(np.abs(got[i] - ref[i]).max()) for i in bad[:5]])
    # the requests exercise what they are there for: 1, 7 (the 0.3 m pairs), 11 .. and 21 sweep pieces
    runs = [1 + int((bits(ref[i][250:750])[1:] != bits(ref[i][250:750])[:-1]).any(axis=1).sum()) for i in range(67)]
    assert min(runs) == 1 and max(runs) == 21 and 7 in runs
    # a second call with the same requests plans nothing and leaves the plans alone
    env.step_macro_device(md)
    assert not env.macro_buffer('replanned', host=True).any()
    assert same_bits(env.macro_buffer('plan', host=True), got)
    env.close()


def test_device_plans_against_the_float64_checker():
    """The check tests/test_gpu_ik_macro.py applies to rr_plan_macro, on the plans rr_step_macro made: the default's plan of the first
    pair against generate_plan to IK_TOL; the single-seed plans at one row of every IK segment, wherever the float64 solve converged
    before update 500."""
    pairs = [((-0.25, -0.5), (0.05, 0.0)), ((0.05, 0.0), (-0.25, 0.5)), ((-0.25, 0.5), (-0.25, -0.5)), ((0.05, 0.5), (0.05, -0.5)),
             ((-0.25, 0.0), (0.05, 0.5)), ((0.05, -0.5), (-0.25, 0.0))]
    n = len(pairs)
    macro = np.array(pairs, dtype=np.float32)
    plans = {}
    for single in (False, True):
        env = BatchedREALRobotEnv(n, objects=1, width=64, height=64, solver={'ik_single_seed': single})
        env.step_macro_device(dev(macro))
        plans[single] = env.macro_buffer('plan', host=True)
        env.close()
    host = generate_plan(np.zeros(11), pairs[0])
    assert np.abs(plans[False][0][:100] - host[:100]).max() < 1e-6
    assert np.abs(plans[False][0] - host).max() < IK_TOL
    rows = [150, 225, 300, 500, 740, 775]
    n_cmp = 0
    for i in range(n):
        way = plan_way_points(macro[i].astype(np.float64))
        for r in rows:
            first, target = [w for w in way if w[0] <= r][-1]
            q, err, _, _, _, updates = ik_candidates(np.zeros(11), target, ORIENT, single_seed=True)[0]
            if not updates < 500:
                continue
            assert np.abs(plans[True][i][r] - q[:9]).max() < IK_TOL, (pairs[i], r)
            n_cmp += 1
    assert n_cmp >= 0.7 * 6 * n, n_cmp
    assert np.abs(plans[True] - plans[False]).max() > 0.1


def test_an_exhausted_plan_is_replanned_from_the_present_joints():
    n = 5
    env = make(n)
    scatter_postures(env, 3)
    md = dev(requests(np.random.default_rng(8), n))
    seen = []
    for t in range(1001):
        env.step_macro_device(md)
        seen.append(env.macro_buffer('replanned', host=True))
        if t == 0:
            first = env.macro_buffer('plan', host=True)
        if t == 999:
            assert (env.macro_buffer('position', host=True) == 1000).all()
    seen = np.stack(seen)
    assert seen[0].all() and seen[1000].all() and not seen[1:1000].any()
    assert (env.macro_buffer('position', host=True) == 1).all()
    second = env.macro_buffer('plan', host=True)
    for r0, r1 in ((0, 100), (800, 1000)):
        assert same_bits(first[:, r0:r1], second[:, r0:r1])
    for i in range(n):      # another posture at step 1000 (home, not the scattered start): other IK rows
        assert not np.array_equal(first[i, 100:800], second[i, 100:800]), i
    env.close()


def test_idle_envs_step_with_zeros_and_keep_record_plan_and_position():
    n = 5
    A, B = make(n), make(n)
    m = requests(np.random.default_rng(1), n)
    md = dev(m)
    for e in (A, B):
        scatter_postures(e, 4)
        for _ in range(3):
            e.step_macro_device(md)
    before = {k: B.macro_buffer(k, host=True) for k in ('request', 'position', 'plan')}
    # some envs idle, with a request that would otherwise re-plan: the twin takes the existing idle path over the same plans
    idle = np.array([1, 0, 1, 0, 0], np.uint8)
    other = dev(requests(np.random.default_rng(2), n))
    m2 = np.where(idle[:, None] != 0, other.cpu().numpy(), m)
    B.step_macro_device(dev(m2), idle=dev(idle))
    A.step_plan(idle=idle)
    assert same_bits(A.state, B.state)
    after = {k: B.macro_buffer(k, host=True) for k in ('request', 'position', 'plan')}
    assert not B.macro_buffer('replanned', host=True).any()
    on = idle != 0
    for k in before:
        assert same_bits(before[k][on], after[k][on]), k
    assert np.array_equal(after['position'], before['position'] + (1 - idle))
    # every env idle (host arrays this time): the step is a step with zeros(9)
    B.step_macro_device(m, idle=np.ones(n, bool))
    A.step(np.zeros((n, 9), np.float32))
    assert same_bits(A.state, B.state)
    assert same_bits(B.macro_buffer('position', host=True), after['position'])
    A.close(), B.close()


def test_invalidate_and_nan_requests():
    env = make()
    m = requests(np.random.default_rng(6))
    md = dev(m)
    env.step_macro_device(md)
    env.step_macro_device(md)
    assert not env.macro_buffer('replanned', host=True).any()
    rng = np.random.default_rng(7)
    for on_device in (True, False):
        mask = rng.random(N) < 0.4
        env.macro_invalidate(dev(mask) if on_device else mask)
        req = env.macro_buffer('request', host=True)
        assert np.isnan(req[mask]).all() and same_bits(req[~mask], m[~mask])
        pos = env.macro_buffer('position', host=True)
        env.step_macro_device(md)
        assert np.array_equal(env.macro_buffer('replanned', host=True), mask.astype(np.uint8)), on_device
        assert np.array_equal(env.macro_buffer('position', host=True), np.where(mask, 1, pos + 1))
        assert same_bits(env.macro_buffer('request', host=True), m)
    env.macro_invalidate()
    env.step_macro_device(m.reshape(N, 2, 2))                # (a host array)
    assert env.macro_buffer('replanned', host=True).all()
    # a NaN request never equals its record: that env plans on every step
    m[5, 2] = np.nan
    md = dev(m)
    for _ in range(3):
        env.step_macro_device(md)
        rp = env.macro_buffer('replanned', host=True)
        assert rp[5] == 1 and rp.sum() == 1
        assert env.macro_buffer('position', host=True)[5] == 1
    env.close()


def test_mixing_with_plan_macro_and_step_plan():
    """rr_plan_macro and rr_step_plan share plan and position and do not know the record: the three buffers alone define the result."""
    env = make()
    m = requests(np.random.default_rng(12))
    md = dev(m)
    for _ in range(2):
        env.step_macro_device(md)
    req0, pos0, plan0 = (env.macro_buffer(k, host=True) for k in ('request', 'position', 'plan'))
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    m2 = requests(np.random.default_rng(13))
    env.plan_macro(m2.reshape(N, 2, 2), mask)               # new plans and position 0 for the masked envs; the record is not told
    env.step_plan()
    req1, pos1, plan1 = (env.macro_buffer(k, host=True) for k in ('request', 'position', 'plan'))
    assert same_bits(req1, req0)
    assert np.array_equal(pos1, np.where(mask != 0, 1, pos0 + 1))
    assert same_bits(plan1[mask == 0], plan0[mask == 0])
    assert all(not np.array_equal(plan1[i], plan0[i]) for i in np.flatnonzero(mask))
    # the old request again: the record still equals it, so nobody plans and the masked envs go on with rr_plan_macro's plans
    twin_cmd = plan1[np.arange(N), pos1]
    env.snapshot_slots(1)
    env.step_macro_device(md)
    assert not env.macro_buffer('replanned', host=True).any()
    assert np.array_equal(env.macro_buffer('position', host=True), pos1 + 1)
    assert same_bits(env.macro_buffer('plan', host=True), plan1)
    got = env.state
    env.load_snapshot(0)
    env.step(twin_cmd)                                      # the expectation from the buffers before: row `position` of each plan
    assert same_bits(env.state, got)
    env.close()


def _low_dim(obs):
    return {k: np.array(obs[k]) for k in ('joint_positions', 'touch_sensors', 'object_positions')}


@pytest.mark.parametrize('replan', [False, True])
def test_vector_env_macro_actions(replan):
    n, horizon = 5, 12
    venv = REALRobotVectorEnv(n, additional_obs=True, eye_width=64, eye_height=64, max_episode_steps=horizon, render_every_step=False,
                              action_type='macro_action', macro_replan_on_reset=replan)
    be = BatchedREALRobotEnv(n, objects=3, width=64, height=64)
    assert set(venv.action_space.spaces) == {'macro_action', 'render'} and venv.action_space['macro_action'].shape == (n, 2, 2)
    obs, _ = venv.reset(seed=0)
    be.reset()

    def hand_obs():
        return {'joint_positions': be.host(nat.F_JOINTS), 'touch_sensors': be.host(nat.F_TOUCH), 'object_positions': be.host(nat.F_OBJ_POSE)}

    for k, v in hand_obs().items():
        assert same_bits(np.array(obs[k]), v), k
    rng = np.random.default_rng(21)
    m = requests(rng, n).reshape(n, 2, 2)
    steps = np.zeros(n, np.int64)
    prev_trunc = np.zeros(n, bool)
    for t in range(30):
        changed = np.zeros(n, bool)
        if t in (5, 17):
            changed[[1, 3]] = True
            m[changed] = requests(rng, 2).reshape(2, 2, 2)
        act = dev(m) if t % 2 else m.copy()                  # device tensors and host arrays alike
        obs, rew, term, trunc, infos = venv.step({'macro_action': act, 'render': False})
        be.step_macro_device(act)
        steps += 1
        want_trunc = steps >= horizon
        if want_trunc.any():
            be.reset(want_trunc.astype(np.uint8))
            if replan:
                be.macro_invalidate(want_trunc.astype(np.uint8))
            steps[want_trunc] = 0
        assert np.array_equal(trunc, want_trunc) and not np.any(term) and not np.any(rew), t
        for k, v in hand_obs().items():
            assert same_bits(np.array(obs[k]), v), (t, k)
        rp = venv._be.macro_buffer('replanned', host=True)
        want = (np.ones(n, bool) if t == 0 else changed) | (prev_trunc if replan else False)
        assert np.array_equal(rp, want.astype(np.uint8)), (t, rp)
        prev_trunc = want_trunc
    assert prev_trunc.sum() == 0 and (steps == 30 % horizon).all()
    venv.close(), be.close()


def test_a_handle_that_used_the_device_path_once_runs_like_one_that_never_did():
    """The on-demand memory does not leak into other paths: step() / plan_macro / step_plan() after one step_macro_device and a
    macro_invalidate() are bit for bit what they are on a handle that planned the same step with plan_macro + step_plan."""
    A, B = make(), make()
    for e in (A, B):
        scatter_postures(e, 14)
    m = requests(np.random.default_rng(15))
    A.plan_macro(m.reshape(N, 2, 2))
    A.step_plan()
    B.step_macro_device(dev(m))
    B.macro_invalidate()
    assert same_bits(A.state, B.state)
    rng = np.random.default_rng(16)
    m2 = requests(rng)
    mask = (rng.random(N) < 0.5).astype(np.uint8)
    for t in range(12):
        for e in (A, B):
            if t == 4:
                e.plan_macro(m2.reshape(N, 2, 2), mask)
            if t % 3 == 2:
                e.step(np.full((N, 9), 0.1 * t, np.float32))
            else:
                e.step_plan(idle=mask if t == 7 else None)
        assert same_bits(A.state, B.state), t
    for i in (0, 1, N - 1):
        assert same_bits(A.get_plan(i), B.get_plan(i))
    for f in (nat.F_JOINTS, nat.F_TOUCH, nat.F_OBJ_POSE, nat.F_TIMESTEP, nat.F_ERRFLAGS):
        assert same_bits(A.host(f), B.host(f)), f
    A.close(), B.close()
