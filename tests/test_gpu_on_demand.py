"""GPU test (-m gpu): every on-demand allocation group of a handle alive at once, in either order of arrival (rr_mem.inc owns them).
Two handles of 5 envs (not a multiple of 4: tails are live), 3 objects, 32 x 32 images.  Handle A calls every entry point that
allocates on first use once -- contact observations, goal scores with a mask, a macro plan and one plan step, per-env cameras, per-env
appearance, a goal table with images / env goals / an episode update, snapshot slots and an in-place fork through a host index, the
mapped observation and image blocks --, handle B the same calls in the reverse order on the same seeded inputs; both then take the same
three rendered steps.  Everything a caller can read must agree bit for bit, and every device pointer handed out before the steps must be
the one handed out after them.

The calls are arranged so that their ORDER cannot matter to the values: the two envs the fork swaps (2 and 4) get the same commands and
the same macro action up to there, so they are copies of each other whenever the swap happens; the cameras (envs 1, 3) and appearances
(envs 0, 3) are settings that stay with an env; nothing renders before the common steps.  The contact-observation fields and the episode
score hold what their LAST call computed (A's and B's first calls saw different moments of the run), so both are computed once more
after the steps -- into the buffers that exist by then, which the pointer check covers."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from real_robots_amd.mathutil import look_at, perspective

pytestmark = pytest.mark.gpu

N, K, W, H = 5, 3, 32, 32
T0 = 100          # steps before the calls: the objects rest on the table by then (tests/test_gpu_contact_obs.py)
FIELDS = (nat.F_JOINTS, nat.F_TOUCH, nat.F_OBJ_POSE, nat.F_RGB, nat.F_DEPTH, nat.F_MASK, nat.F_TIMESTEP, nat.F_ERRFLAGS, nat.F_STATE,
          nat.F_CONTACT_COUNT, nat.F_ENV_CLASS, nat.F_CONTACTS, nat.F_BODY_FORCE, nat.F_BODY_PARTNERS)


def _inputs():
    rng = np.random.default_rng(41)
    x = {}
    x['eval_pos'] = rng.uniform(-0.4, 0.4, (N, K, 3)).astype(np.float32)
    x['eval_mask'] = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 0], [0, 0, 1], [1, 1, 0]], np.uint8)
    macro = rng.uniform(-0.3, 0.3, (N, 2, 2)).astype(np.float32)
    macro[4] = macro[2]
    x['macro'] = macro
    a = W / H
    x['views'] = np.stack([look_at((-0.05 + 0.02 * i, 0.1, 0.5 + 0.1 * i), (0.3, -0.05, 0.2), (0.0, 0.0, 1.0)) for i in range(N)]).astype(np.float32)
    x['projs'] = np.stack([perspective(70.0 + 5 * i, a, 0.1, 100.0) for i in range(N)]).astype(np.float32)
    x['cam_mask'] = np.array([0, 1, 0, 1, 0], np.uint8)
    x['light'] = rng.normal(size=(N, 3)).astype(np.float32)
    x['app_mask'] = np.array([1, 0, 0, 1, 0], np.uint8)
    G = 2
    start = rng.uniform(-0.2, 0.2, (G, K, 7)).astype(np.float32)
    start[..., 2] = 0.5
    start[..., 3:] = (0, 0, 0, 1)
    x['goals'] = (start, rng.uniform(-0.3, 0.3, (G, K, 3)).astype(np.float32), np.full((G, K), nat.GOAL_SCORED | nat.GOAL_HAS_START, np.uint8),
                  rng.integers(0, 256, (G, H, W, 3)).astype(np.uint8))
    x['goal_index'] = np.array([0, 1, -1, 1, 0], np.int32)
    x['swap'] = np.array([-1, -1, 4, -1, 2], np.int32)
    return x


def _cmd(t):
    return synthetic_actions(range(N), t, seed=9).astype(np.float32)


def _calls(env, x, got):
    """The on-demand entry points in handle A's order; `got` collects what the calls return."""
    def colours():
        c = env.default_env_appearance()['colours']
        c[:, :, 0] = 0.25 + 0.1 * np.arange(N, dtype=np.float32)[:, None]
        return c

    def goals():
        env.set_goals(*x['goals'])
        env.set_env_goals(x['goal_index'])
        env.episode_update(reset_done=False)

    def plan():
        env.plan_macro(x['macro'])
        env.step_plan(render=False)

    def fork():
        env.snapshot_slots(2)
        env.fork(x['swap'])

    def maps():
        got['mirror'] = env.map_observations()
        got['img_mirror'] = env.map_images()

    return [lambda: env.contact_observations(),
            lambda: got.__setitem__('eval', env.evaluate_goals(x['eval_pos'], x['eval_mask'])),
            plan,
            lambda: env.set_env_cameras(x['views'], x['projs'], env_mask=x['cam_mask']),
            lambda: env.set_env_appearance(colours=colours(), light_dirs=x['light'], env_mask=x['app_mask']),
            goals, fork, maps]


def _pointers(env):
    out = []
    for f in FIELDS:
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_get_buffer(env.h, f, C.byref(p), C.byref(n)))
        out.append(('field', f, p.value, n.value))
    for which in range(len(nat.EP_NAMES)):
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(env.L.rr_episode_buffer(env.h, which, C.byref(p), C.byref(n)))
        out.append(('episode', which, p.value, n.value))
    return out


def test_every_on_demand_group_in_either_order_of_arrival():
    x = _inputs()
    envs = [BatchedREALRobotEnv(N, objects=K, width=W, height=H) for _ in range(2)]
    got = [{}, {}]
    for t in range(T0):                                  # history first (the objects land: contacts to observe); envs 2 and 4 stay copies
        c = _cmd(t)
        c[4] = c[2]
        for e in envs:
            e.step(c, render=False)
    for e, g, order in zip(envs, got, (1, -1)):
        for call in _calls(e, x, g)[::order]:
            call()
    ptrs = [_pointers(e) for e in envs]
    for p in ptrs:
        assert all(addr for _, _, addr, _ in p) and len({addr for _, _, addr, _ in p}) == len(p)      # every buffer exists, no two share an address
    for t in range(T0, T0 + 3):
        for e in envs:
            e.step(_cmd(t), render=True)
    out = []
    for e, g in zip(envs, got):
        e.episode_update(reset_done=False)
        co = e.contact_observations(host=True)
        e.sync()
        r = {'state': e.state, 'rgb': e.host(nat.F_RGB), 'depth': e.host(nat.F_DEPTH), 'mask': e.host(nat.F_MASK),
             'contacts': co['contacts'], 'count': co['count'], 'body_force': co['body_force'], 'body_partners': co['body_partners'],
             'score': e.episode_buffer('score', host=True), 'goal_pos': e.episode_buffer('goal_pos', host=True),
             'goal_rgb': e.episode_buffer('goal_rgb', host=True), 'goal_index': e.episode_buffer('goal_index', host=True)}
        r.update({'mirror_' + k: v.copy() for k, v in g['mirror'].items()})
        r.update({'img_mirror_%d' % i: v.copy() for i, v in enumerate(g['img_mirror'])})
        out.append(r)
    a, b = out
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k      # bit for bit (NaN: the goal position of an env without a goal)
    # ... and the values are those of a run, not of two handles that both did nothing
    assert (a['count'] > 0).any() and a['rgb'].std() > 0
    assert np.array_equal(a['goal_index'], x['goal_index'])
    assert np.array_equal(a['goal_rgb'][[0, 1, 3, 4]], x['goals'][3][[0, 1, 1, 0]]) and not a['goal_rgb'][2].any()
    assert np.isnan(a['goal_pos'][2]).all() and np.array_equal(a['goal_pos'][0], x['goals'][1][0])
    assert np.array_equal(a['mirror_joints'], envs[0].host(nat.F_JOINTS)) and np.array_equal(a['img_mirror_0'], a['rgb'])
    assert np.array_equal(a['img_mirror_1'], a['depth']) and np.array_equal(a['img_mirror_2'], a['mask'])
    # the per-env settings took: an env with a camera or an appearance of its own does not show what its neighbour with the model's shows
    assert not np.array_equal(a['rgb'][1], a['rgb'][2]) and not np.array_equal(a['rgb'][0], a['rgb'][2])
    # the pointers handed out before the steps are the ones handed out after them
    for e, p in zip(envs, ptrs):
        assert _pointers(e) == p
    for e in envs:
        e.close()
