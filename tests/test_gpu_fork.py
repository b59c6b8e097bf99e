"""GPU tests (-m gpu) of env forks and snapshot slots on the device (rr_snapshot_slots / rr_copy_envs, rr_fork.inc):
* a fork continues its source's run bit for bit -- state, contact lists with forces, touch, images -- for an index with a swap, a
  cycle, a chain, self copies, kept envs and a broadcast from an overwritten env, where a plain state copy does not;
* slots: save / load, the records of allocation time, one saved env into all running ones, slot-to-slot permutations;
* one env; a device-resident index and its out-of-range entries; settings and the episode record stay with the destination;
* refused calls change nothing; the look-ahead is invalidated.
The workload is the one of the checkpoint test (tests/test_gpu_round3.py), where the contact history is known to matter."""

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions

pytestmark = pytest.mark.gpu

N_RUN, T_FORK = 96, 120
_cmd_cache = []


def _cmds():
    """Commands of the run, [200][96, 9]: keyed by env id, so the first n columns are the commands of an n-env batch."""
    if not _cmd_cache:
        _cmd_cache.extend(synthetic_actions(range(N_RUN), t, seed=5).astype(np.float32) for t in range(200))
    return _cmd_cache


def _make(monkeypatch, env_vars, *args, **kw):
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    try:
        return BatchedREALRobotEnv(*args, **kw)
    finally:
        for k in env_vars:
            monkeypatch.delenv(k, raising=False)


def _snapshot(env):
    return (env.state, env.host(nat.F_TOUCH), env.host(nat.F_CONTACT_COUNT), env.host(nat.F_RGB), env.host(nat.F_DEPTH),
            env.host(nat.F_MASK), env.host(nat.F_JOINTS), env.host(nat.F_OBJ_POSE), env.host(nat.F_ERRFLAGS), env.host(nat.F_TIMESTEP))


def _all_contacts(env):
    return [env.contacts(i) for i in range(env.N)]


def _assert_same(a, b, src, label):
    """every part of snapshot a at env i equals b's at env src[i], bitwise"""
    for j, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y[src], equal_nan=True), (label, j, np.flatnonzero([not np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y[src])]))


def _assert_contacts(ca, cb, src, label):
    for i, s in enumerate(src):
        assert np.array_equal(ca[i], cb[s]), (label, i, s)


def _warm_up(envs, n, steps=T_FORK):
    for t in range(steps):
        for e in envs:
            e.step(_cmds()[t][:n], render=(t % 7 == 0))


def _fork_index(count, N):
    """swap, cycle, chain through an overwritten env, self copy, kept envs, a broadcast of the env with the most contacts, a seeded
    draw with repeats for the rest"""
    k = int(np.argmax(count))
    assert count[k] > 0                     # (the run has contact history to carry)
    idx = np.random.default_rng(17).integers(0, N, N).astype(np.int32)
    draw = idx.copy()
    idx[0], idx[1] = 1, 0
    idx[2], idx[3], idx[4] = 3, 4, 2
    idx[5], idx[6] = 6, 7
    idx[8] = 8
    idx[9:16] = -1
    idx[16:48] = k
    if idx[k] == -1:                        # the broadcast's source has to be written by the copy itself: when the env with the most
        idx[k] = draw[k] if draw[k] != k else (k + 1) % N      # contacts is one of 9..15 (it is 10 in this run), it takes its draw instead of staying
    assert idx[k] != -1 and (idx[9:16] == -1).sum() >= 6
    return idx, k


def _check_right_after_fork(A, B, idx):
    src = np.where(idx < 0, np.arange(A.N), idx)
    for f in (nat.F_STATE, nat.F_TOUCH, nat.F_TIMESTEP, nat.F_CONTACT_COUNT, nat.F_JOINTS, nat.F_OBJ_POSE, nat.F_ERRFLAGS):
        assert np.array_equal(A.host(f), B.host(f)[src], equal_nan=True), f
    _assert_contacts(_all_contacts(A), _all_contacts(B), src, 'fork')
    return src


def test_fork_continues_bit_for_bit_with_in_place_hazards():
    N = N_RUN
    A, B, Cn = (BatchedREALRobotEnv(N, objects=3, width=64, height=64) for _ in range(3))
    _warm_up((A, B, Cn), N)
    idx, k = _fork_index(B.host(nat.F_CONTACT_COUNT), N)
    A.fork(idx)
    src = _check_right_after_fork(A, B, idx)
    assert (A.host(nat.F_CONTACT_COUNT)[16:48] == B.host(nat.F_CONTACT_COUNT)[k]).all()
    Cn.state = B.state[src]                 # the negative control: the 61 floats without the contact history
    for t in range(1, 61):
        cmd = _cmds()[T_FORK + t - 1]
        B.step(cmd, render=True)
        A.step(cmd[src], render=True)
        Cn.step(cmd[src], render=True)
        if t in (1, 2, 20, 40, 60):
            _assert_same(_snapshot(A), _snapshot(B), src, t)
            _assert_contacts(_all_contacts(A), _all_contacts(B), src, t)
    assert (A.host(nat.F_ERRFLAGS) == 0).all()
    assert not np.array_equal(Cn.state, A.state)        # the history is what the fork adds
    for e in (A, B, Cn):
        e.close()


def test_slots_save_load_broadcast_and_permute():
    N = 70                                  # crosses a 64-env group and is no multiple of it
    cm = [c[:N] for c in _cmds()]
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    st0 = env.state
    env.snapshot_slots(2)
    for t in range(100):
        env.step(cm[t], render=(t % 7 == 0))
    env.save_snapshot(1)
    st_save, cnt_save = env.state, env.host(nat.F_CONTACT_COUNT)
    k = int(np.argmax(cnt_save))
    assert cnt_save[k] > 0
    for t in range(100, 140):
        env.step(cm[t], render=True)
    ref, ref_c = _snapshot(env), _all_contacts(env)
    ident = np.arange(N)

    env.load_snapshot(1)
    assert np.array_equal(env.state, st_save, equal_nan=True) and (env.host(nat.F_TIMESTEP) == 100).all()
    for t in range(100, 140):
        env.step(cm[t], render=True)
    _assert_same(_snapshot(env), ref, ident, 'load')
    _assert_contacts(_all_contacts(env), ref_c, ident, 'load')

    env.load_snapshot(0)                    # slot 0 still holds the records of allocation time
    assert (env.host(nat.F_TIMESTEP) == 0).all() and np.array_equal(env.state, st0) and (env.host(nat.F_CONTACT_COUNT) == 0).all()

    env.load_snapshot(1, src_index=np.full(N, k))       # one saved env into every running one
    for t in range(100, 140):
        env.step(np.tile(cm[t][k], (N, 1)), render=True)
    _assert_same(_snapshot(env), ref, np.full(N, k), 'broadcast')
    _assert_contacts(_all_contacts(env), ref_c, np.full(N, k), 'broadcast')

    perm = np.random.default_rng(3).permutation(N)
    env.copy_envs(perm, 1, 0)               # slot to slot
    env.load_snapshot(0)
    assert np.array_equal(env.state, st_save[perm], equal_nan=True) and (env.host(nat.F_TIMESTEP) == 100).all()
    for t in range(100, 140):
        env.step(cm[t][perm], render=True)
    _assert_same(_snapshot(env), ref, perm, 'permuted')
    _assert_contacts(_all_contacts(env), ref_c, perm, 'permuted')
    env.copy_envs(perm, 0, 0)               # within one slot: staged
    env.load_snapshot(0)
    assert np.array_equal(env.state, st_save[perm][perm], equal_nan=True)
    assert np.array_equal(env.host(nat.F_CONTACT_COUNT), cnt_save[perm][perm])

    env.snapshot_slots(0)
    with pytest.raises(nat.NativeError):
        env.load_snapshot(0)
    env.close()


def test_one_env():
    env, twin = (BatchedREALRobotEnv(1, objects=3, width=64, height=64) for _ in range(2))
    cm = [c[:1] for c in _cmds()]
    _warm_up((env, twin), 1, 40)
    env.snapshot_slots(1)
    t = 40
    for what in ('fork', 'keep', 'save_load'):
        if what == 'fork':
            env.fork([0])
        elif what == 'keep':
            env.fork([-1])
        else:
            env.save_snapshot(0)
            env.load_snapshot(0)
        for _ in range(2):
            env.step(cm[t], render=True)
            twin.step(cm[t], render=True)
            t += 1
        _assert_same(_snapshot(env), _snapshot(twin), np.arange(1), what)
        _assert_contacts(_all_contacts(env), _all_contacts(twin), [0], what)
    env.close()
    twin.close()


def test_device_index_and_its_out_of_range_entries():
    import torch
    N = 70
    cm = [c[:N] for c in _cmds()]
    A, B = (BatchedREALRobotEnv(N, objects=3, width=64, height=64) for _ in range(2))
    _warm_up((A, B), N, 60)
    idx = np.random.default_rng(5).integers(-1, N, N).astype(np.int32)
    idx[:3] = (1, 2, 0)
    dev = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    A.fork(idx)
    B.fork(dev)
    ident = np.arange(N)
    _assert_same(_snapshot(B), _snapshot(A), ident, 'device index')
    _assert_contacts(_all_contacts(B), _all_contacts(A), ident, 'device index')
    # entries that are no env keep their env, the rest is copied
    before, before_c = _snapshot(B), _all_contacts(B)
    idx2 = np.random.default_rng(6).integers(0, N, N).astype(np.int32)
    idx2[[4, 65]] = N
    idx2[[9, 69]] = -7
    idx2[20] = -1
    dev2 = torch.from_numpy(idx2).cuda()
    torch.cuda.synchronize()
    B.fork(dev2)
    src = np.where((idx2 < 0) | (idx2 >= N), ident, idx2)
    after = _snapshot(B)
    for j in (0, 1, 2, 6, 7, 8, 9):         # (the images stay with their env)
        assert np.array_equal(after[j], before[j][src], equal_nan=True), j
    for j in (3, 4, 5):
        assert np.array_equal(after[j], before[j]), j
    _assert_contacts(_all_contacts(B), before_c, src, 'out of range')
    for e in (A, B):
        e.step(cm[60], render=True)
    assert (B.host(nat.F_ERRFLAGS) == 0).all()
    for e in (A, B):
        e.close()


def test_settings_and_the_episode_record_stay_with_the_destination():
    from real_robots_amd.mathutil import look_at, perspective
    from real_robots_amd.model import load_model
    N, W = 16, 64
    cm = [c[:N] for c in _cmds()]
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=W)
    mass = np.tile(np.array([1.0, 0.5, 0.8], np.float32), (N, 1)) * (1.0 + 0.25 * np.arange(N, dtype=np.float32))[:, None]
    env.set_object_dynamics(mass=mass, friction=np.linspace(0.3, 0.9, N)[:, None])
    env.set_env_actuators(kp=(0.1 + 0.02 * np.arange(N))[:, None], max_force=(500.0 + 10.0 * np.arange(N))[:, None])
    home = np.array([-0.1, 0.2, 0.55, 0, 0, 0, 1], np.float32)
    env.set_object_home(3, 0, home)
    cam_mask = np.zeros(N, np.uint8)
    cam_mask[5] = 1
    view = look_at((0.6, 0.5, 1.0), np.asarray(load_model()['table_pos'], np.float64), (0.0, 0.0, 1.0))
    env.set_env_cameras(np.asarray(view, np.float32), np.asarray(perspective(70.0, 1.0, 0.1, 100.0), np.float32), cam_mask)
    G = 4
    final = np.random.default_rng(1).uniform(-0.2, 0.2, (G, 3, 3)).astype(np.float32) + np.array([-0.1, 0.0, 0.45], np.float32)
    env.set_goals(np.full((G, 3, 7), np.nan, np.float32), final, np.full((G, 3), nat.GOAL_SCORED, np.uint8))
    env.set_env_goals((np.arange(N) % G).astype(np.int32))
    for t in range(60):
        env.step(cm[t], render=(t % 7 == 0))
    env.episode_update(False)
    dyn, act = env._dynamics_raw(), env._actuators_raw()
    ep = [env.episode_buffer(n, host=True) for n in ('score', 'goal_index', 'episode', 'reward', 'done', 'goal_pos')]
    st = env.state
    idx = np.zeros(N, np.int32)             # every env becomes env 0 ...
    idx[0] = -1
    env.fork(idx)
    assert np.array_equal(env.state, np.tile(st[0], (N, 1)), equal_nan=True)
    assert np.array_equal(env._dynamics_raw(), dyn) and np.array_equal(env._actuators_raw(), act)
    for a, n in zip(ep, ('score', 'goal_index', 'episode', 'reward', 'done', 'goal_pos')):
        assert np.array_equal(env.episode_buffer(n, host=True), a, equal_nan=True), n
    env.render()                            # ... seen through its own camera
    rgb = env.host(nat.F_RGB)
    assert np.array_equal(rgb[1], rgb[0]) and np.array_equal(rgb[7], rgb[0]) and not np.array_equal(rgb[5], rgb[0])
    for t in range(60, 90):                 # ... and steps with its own mass, friction and gains
        env.step(np.tile(cm[t][0], (N, 1)))
    st2 = env.state
    assert (env.host(nat.F_ERRFLAGS) == 0).all() and (env.host(nat.F_TIMESTEP) == 90).all()
    assert all(not np.array_equal(st2[i], st2[0]) for i in range(1, N))
    m = np.zeros(N, np.uint8)
    m[[3, 4]] = 1
    env.reset(m)                            # the home poses are the destination's own
    pose = env.host(nat.F_OBJ_POSE)
    assert np.array_equal(pose[3, 0], home) and not np.array_equal(pose[4, 0], home)
    env.close()


def test_refused_calls_change_nothing():
    N = 16
    cm = [c[:N] for c in _cmds()]
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    for t in range(40):
        env.step(cm[t], render=(t % 7 == 0))
    env.snapshot_slots(1)
    st, ck = env.state, env.checkpoint()
    bad = np.arange(N, dtype=np.int32)
    bad[0], bad[11] = 5, N

    def refused(call, needle=None):
        with pytest.raises(nat.NativeError) as ei:
            call()
        if needle:
            assert needle in str(ei.value), str(ei.value)
        assert np.array_equal(env.state, st, equal_nan=True) and np.array_equal(env.checkpoint(), ck)

    for s, d in ((-1, -1), (0, -1), (-1, 0)):       # (past the Python layer's own check: the library's)
        refused(lambda: nat.check(env.L.rr_copy_envs(env.h, s, d, bad.ctypes.data, 0)), 'env 11')
    bad[11] = -2
    refused(lambda: nat.check(env.L.rr_copy_envs(env.h, -1, -1, bad.ctypes.data, 0)), 'env 11')
    refused(lambda: env.load_snapshot(1))
    refused(lambda: env.save_snapshot(1))
    refused(lambda: env.load_snapshot(-2))
    refused(lambda: env.copy_envs(None, 0, 7))
    refused(lambda: env.snapshot_slots(-1))
    refused(lambda: env.snapshot_slots(65))
    env.load_snapshot(0)                    # the slot of before is still there
    assert np.array_equal(env.state, st, equal_nan=True)
    env.close()


def test_fork_invalidates_the_lookahead(monkeypatch):
    N = N_RUN
    A = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    D = _make(monkeypatch, {'RR_NO_LOOKAHEAD': '1'}, N, objects=3, width=64, height=64)
    _warm_up((A, D), N)
    idx, _ = _fork_index(A.host(nat.F_CONTACT_COUNT), N)
    ident = np.arange(N)
    _assert_same(_snapshot(A), _snapshot(D), ident, 'before')
    for e in (A, D):
        e.fork(idx)
    _assert_same(_snapshot(A), _snapshot(D), ident, 'fork')
    src = np.where(idx < 0, ident, idx)
    for t in range(20):
        for e in (A, D):
            e.step(_cmds()[T_FORK + t][src], render=True)
        if t in (0, 1, 19):
            _assert_same(_snapshot(A), _snapshot(D), ident, t)
    _assert_contacts(_all_contacts(A), _all_contacts(D), ident, 'end')
    for e in (A, D):
        e.close()
