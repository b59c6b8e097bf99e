"""GPU tests (-m gpu): the device's contact lists (rr_get_contacts) against the float64 numpy narrow phase (tests/numpy_collide.py).

tests/test_gpu_contacts_fuzz.py holds k_collide to the oracle bit for bit -- the same algorithm written twice by the same hand.  Here
the reference is the cull-free numpy restatement run on the device state from which the list was made (state before the step, list
after it): the shape_roff pair cull, the sphere-beyond-one-plane cull and the six-plane vertex prefilter of the device have no
counterpart in it, so a cull that dropped a contact shows as a missing one.  The stable / set-aside rule, THRESHOLD, TOLERANCE and the
10 % cap are those fixed on the float32 oracle build in tests/test_numpy_collide.py; nothing here is tuned on the device.
The coverage counts are taken from the reference's result for the lists that passed the comparison -- what the device produced.
The device raises no error flag at the 48-contact cap: RR_F_ERRFLAGS must be clean for every env whose state is finite.
"""
import time

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_collide as nc
from tests import numpy_step as ns
from tests.test_gpu_contacts_fuzz import state_bounds, _grasp_script, SENS_FACTOR
from tests.test_gpu_numpy_step import _perturbed_spread, _dev, force_bound
from tests.test_gpu_round6 import _make
from tests.test_numpy_collide import THRESHOLD, TOLERANCE, SET_ASIDE_CAP, states as cpu_states

pytestmark = pytest.mark.gpu

COV = {}                                                    # coverage over the whole file, asserted by the last test
TOTAL = dict(pairs=0, aside=0, contacts=0, worst=0.0)


def _new_stats():
    return dict(pairs=0, aside=0, contacts=0, worst=0.0)


def _check_envs(env, st0, picks, nobj, edges, stats, where):
    """The lists of the picked envs after a step against numpy_collide on their states before it."""
    bad = []
    for i in picks:
        if not np.isfinite(st0[i]).all():
            continue
        ref = nc.collide(st0[i].astype(np.float64), nobj, edges=bool(edges), ext=nc.EXT)
        b = nc.check_list(env.contacts(int(i)), ref, THRESHOLD, TOLERANCE, stats, where + (int(i),))
        if not b:
            nc.coverage(ref, COV)
        bad += b
    return bad


def _finish(name, stats, bad, t0, checked):
    share = stats['aside'] / max(stats['pairs'], 1)
    print("\n%s: %d lists, %d pairs compared, %d contacts compared, set-aside share %.3f, worst share of the tolerance used %.2f; %.1f s"
          % (name, checked, stats['pairs'], stats['contacts'], share, stats['worst'], time.time() - t0))
    for k in ('pairs', 'aside', 'contacts'):
        TOTAL[k] += stats[k]
    TOTAL['worst'] = max(TOTAL['worst'], stats['worst'])
    assert not bad, bad[:10]
    assert share <= SET_ASIDE_CAP, share


def _errflags_clean(env):
    assert (env.host(nat.F_ERRFLAGS)[np.isfinite(env.state).all(1)] == 0).all()


def _picks(env, N, rng, per_class):
    """The envs with the most contacts of every RR_F_ENV_CLASS of the step, and a random one."""
    cnt, cls = env.host(nat.F_CONTACT_COUNT), env.host(nat.F_ENV_CLASS)
    out = [int(rng.integers(0, N))]
    for c in sorted(set(cls.tolist())):
        members = np.flatnonzero(cls == c)
        out += members[np.argsort(-cnt[members], kind='stable')][:per_class].tolist()
    return sorted(set(out)), set(cls.tolist())


RUNS = [pytest.param(1, 1, 1, None, 'commands', id='N1'), pytest.param(3, 2, 1, '0', 'macro', id='N3-macro-pool0'),
        pytest.param(130, 3, 1, '900', 'commands', id='N130-pool900'), pytest.param(130, 3, 0, None, 'commands', id='N130-no_edges'),
        pytest.param(130, 2, 0, '0', 'macro', id='N130-macro-no_edges-pool0'), pytest.param(3, 1, 1, None, 'grasp', id='grasp'),
        pytest.param(4096, 3, 1, None, 'commands', id='N4096')]


@pytest.mark.parametrize('N,nobj,edges,pool,drive', RUNS)
def test_device_lists_match_the_numpy_narrow_phase(monkeypatch, N, nobj, edges, pool, drive):
    """Random commands at full range (links pressed into the table), macro pushes and the grasp; batch sizes 1, 3, 130 and 4096
    (a dozen envs covering every class the run used); 1 to 3 objects; edge pass on and off; full, shrunken and empty row pool."""
    t0 = time.time()
    envv = dict(({'RR_SOLVER_POOL': pool} if pool is not None else {}), **({} if edges else {'RR_NO_EDGE_CONTACTS': '1'}))
    env = _make(monkeypatch, envv, N, objects=nobj, width=64, height=64)
    rng = np.random.default_rng(N + 7 * nobj)
    stats, bad, checked, used, seen = _new_stats(), [], 0, set(), set()
    script = _grasp_script()
    if drive == 'macro':
        env.plan_macro(rng.uniform([-0.25, -0.5], [0.05, 0.5], size=(N, 2, 2)))
    if drive == 'grasp':
        for _ in range(100):
            env.step(None)
    T = dict(commands=300, macro=800, grasp=len(script))[drive]
    every = dict(commands=50, macro=100, grasp=8)[drive]
    if N == 4096:
        T, every = 200, 100
    for t in range(T):
        chk = t % every == every - 1 and (drive != 'grasp' or t >= 262)
        if chk:
            st0 = env.state
        if drive == 'macro':
            env.step_plan(render=False)
        elif drive == 'grasp':
            env.step(np.tile(script[t], (N, 1)))
        else:
            env.step((synthetic_actions(range(N), t, seed=5)).astype(np.float32))
        if chk:
            picks, cls = _picks(env, N, rng, 4 if N == 4096 else 2)
            cl = env.host(nat.F_ENV_CLASS)
            used |= cls
            seen |= {int(cl[i]) for i in picks}
            bad += _check_envs(env, st0, picks, nobj, edges, stats, (drive, t))
            checked += len(picks)
    assert seen == used, (seen, used)
    if N == 4096:
        assert len(used) >= 2 and checked >= 12
    _errflags_clean(env)
    env.close()
    _finish("N=%d objects=%d edges=%d pool=%s %s" % (N, nobj, edges, pool, drive), stats, bad, t0, checked)


def test_the_list_does_not_depend_on_the_solver_row_pool(monkeypatch):
    """The same run with the full, the shrunken and the empty pool: the lists of the first step (same state) bit for bit."""
    lists = {}
    for pool in (None, '900', '0'):
        env = _make(monkeypatch, {'RR_SOLVER_POOL': pool} if pool else {}, 34, objects=3, width=64, height=64)
        st = np.stack([s for tag, n, s in cpu_states() if n == 3][:34]).astype(np.float32)
        env.state = st
        env.step(None)
        lists[pool] = [env.contacts(i) for i in range(34)]
        env.close()
    for pool in ('900', '0'):
        for a, b in zip(lists[None], lists[pool]):
            assert a.shape == b.shape and np.array_equal(a[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]], b[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]]), pool
    assert sum(len(a) for a in lists[None]) > 300


@pytest.mark.parametrize('edges', [1, 0], ids=['edges', 'no_edges'])
def test_a_step_after_a_change_from_outside_uses_the_new_state(monkeypatch, edges):
    """A step right after reset(mask), set_object_pose(s), env.state = ... and a checkpoint restore: the list is that of the state
    the step started from (the look-ahead's list, made for the state before the change, must have been discarded).  The states set
    from outside are the CPU test's seeded ones: random postures and poses, the sunk cube, the bottle around the wrist (the
    128-candidate cap), the pile on the gripper (the 48-contact cap), and -- one object -- the edge-crossing poses."""
    t0 = time.time()
    stats, bad, checked = _new_stats(), [], 0
    envv = {} if edges else {'RR_NO_EDGE_CONTACTS': '1'}
    for nobj in (3, 1):
        sts = [s for tag, n, s in cpu_states() if n == nobj and tag in ('random', 'sunk', 'wrist', 'pile', 'edge', 'grasp')]
        if not edges:
            sts = sts[::3] + sts[-5:]
        N = len(sts)
        env = _make(monkeypatch, envv, N, objects=nobj, width=64, height=64)
        rng = np.random.default_rng(3)
        for t in range(60):
            env.step(synthetic_actions(range(N), t, seed=9).astype(np.float32))
        # env.state = ...
        env.state = np.stack(sts).astype(np.float32)
        st0 = env.state
        env.step(None)
        bad += _check_envs(env, st0, range(N), nobj, edges, stats, ('set_state', nobj))
        checked += N
        some = list(range(0, N, max(1, N // 8)))
        # reset(mask)
        for t in range(20):
            env.step(synthetic_actions(range(N), t, seed=9).astype(np.float32))
        env.reset((np.arange(N) % 2 == 0).astype(np.uint8))
        st0 = env.state
        env.step(None)
        bad += _check_envs(env, st0, some + [i + 1 for i in some if i + 1 < N], nobj, edges, stats, ('reset', nobj))
        # set_object_pose / set_object_poses
        for t in range(20):
            env.step(None)
        env.set_object_pose(some[0], 0, np.array([-0.15, 0.1, 0.32, 0, 0, 0, 1], np.float32))
        poses = np.ascontiguousarray(env.state[:, 22:22 + 13 * nobj].reshape(N, nobj, 13)[..., :7])
        poses[:, :, :3] += rng.normal(0, 0.01, size=(N, nobj, 3)).astype(np.float32)
        env.set_object_poses(poses, (np.arange(N) % 2 == 1).astype(np.uint8))
        st0 = env.state
        env.step(None)
        bad += _check_envs(env, st0, some + [i + 1 for i in some if i + 1 < N], nobj, edges, stats, ('set_object_pose', nobj))
        # checkpoint restore
        ck = env.checkpoint()
        for t in range(15):
            env.step(synthetic_actions(range(N), t, seed=11).astype(np.float32))
        env.restore(ck)
        st0 = env.state
        env.step(None)
        bad += _check_envs(env, st0, some, nobj, edges, stats, ('restore', nobj))
        checked += 5 * len(some)
        _errflags_clean(env)
        env.close()
    _finish("changes from outside, edges=%d" % edges, stats, bad, t0, checked)


def test_one_whole_independent_step(monkeypatch):
    """numpy_collide feeds numpy_step: the only device inputs are the state before the step and the previous list (warm start).
    Held to the bounds of tests/test_gpu_numpy_step.py (state_bounds, force_bound; over a flat bound: SENS_FACTOR x numpy's own
    one-ulp spread) on envs whose pairs are all stable and whose points come out in the device's order."""
    t0 = time.time()
    N, k = 64, 3
    env = _make(monkeypatch, {}, N, objects=k, width=64, height=64)
    rng = np.random.default_rng(2)
    checked, worst, pairs = 0, [0.0, 0.0, 0.0, 0.0], set()
    cls_name = lambda b: 'object' if b >= 16 else 'robot' if b >= 0 else 'static'
    for t in range(260):
        cmd = (synthetic_actions(range(N), t, seed=3) * 1.6).astype(np.float32)
        if t < 120 or t % 35:
            env.step(cmd)
            continue
        st0 = env.state
        caches = [env.contacts(i) for i in range(N)]
        env.step(cmd)
        st1 = env.state
        cnt = env.host(nat.F_CONTACT_COUNT)
        for i in np.argsort(-cnt, kind='stable')[:10]:
            if not (np.isfinite(st0[i]).all() and np.isfinite(st1[i]).all()):
                continue
            ref = nc.collide(st0[i].astype(np.float64), k)
            cd = env.contacts(int(i))
            if min(p['margin'] for _, _, _, p in ref['pairs']) <= THRESHOLD or len(cd) != len(ref['records']) or (
                    len(cd) and np.abs(cd[:, 3:10] - ref['records'][:, 3:10]).max() > TOLERANCE):
                continue                                  # (a set-aside pair, or the same points in another order)
            res = ns.step(st0[i].astype(np.float64), cmd[i].astype(np.float64), ref['records'], prev=caches[i], nobj=k)
            f_np, f_dev = res['lambda_n'] / ns.DT, cd[:, 10].astype(np.float64)
            fmax = float(f_dev.max()) if len(cd) else 0.0
            flat = state_bounds(fmax) + (force_bound(fmax),)
            d = _dev(st1[i], res['state'], k) + (float(np.abs(f_dev - f_np).max()) if len(cd) else 0.0,)
            bb = flat
            if any(x > y for x, y in zip(d, flat)):
                sp = _perturbed_spread(st0[i], cmd[i].astype(np.float64), ref['records'].astype(np.float32), caches[i],
                                       ns.default_dynamics(k), 50, (res['state'], f_np), rng, k)
                bb = tuple(max(x, SENS_FACTOR * y) for x, y in zip(flat, sp))
            assert all(x <= y for x, y in zip(d, bb)), (t, int(i), fmax, d, bb)
            worst = [max(w, x / y) for w, x, y in zip(worst, d, flat)]
            pairs |= {(cls_name(int(c[0])), cls_name(int(c[1]))) for c, l in zip(cd, res['lambda_n']) if l > 0}
            checked += 1
    env.close()
    print("\nwhole independent step: %d envs checked; worst deviation / flat bound: joints %.3f, object pose %.3f, object velocity %.3f, "
          "normal force %.3f; loaded pairs %s; %.1f s" % ((checked,) + tuple(worst) + (sorted(pairs), time.time() - t0)))
    assert checked >= 10 and {('object', 'static'), ('robot', 'object')} <= pairs, (checked, pairs)


def test_coverage_of_what_the_device_produced():
    """Over the whole file (run after the tests above): the coverage counts of tests/test_numpy_collide.py on the device's lists."""
    print("\ndevice lists in all: %d pairs compared, %d contacts compared, set-aside share %.3f, worst share of the tolerance used %.2f"
          % (TOTAL['pairs'], TOTAL['contacts'], TOTAL['aside'] / max(TOTAL['pairs'], 1), TOTAL['worst']))
    print("coverage: " + ', '.join('%s %d' % kv for kv in sorted(COV.items())))
    need = nc.COVERAGE_KEYS + ['finger or skin on object %d' % i for i in range(3)]
    missing = [k for k in need if not COV.get(k)]
    assert not missing, missing
    assert TOTAL['pairs'] > 1000 and TOTAL['contacts'] > 3000
