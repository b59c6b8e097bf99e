"""GPU tests (-m gpu) of per-env cameras (rr_set_env_cameras): env i of a per-env handle is byte for byte env i of a handle whose
one camera is env i's (every step path, incremental updates and vacated pixels included); drawn cameras against the float64
ray caster of tests/numpy_camera.py; the mask, validation and lifetime rules; the vector env's camera_randomization."""
import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from real_robots_amd.mathutil import look_at, perspective, view_from_yaw_pitch_roll
from real_robots_amd.model import load_model
from tests import numpy_camera as nc
from tests.test_numpy_camera import compare

pytestmark = pytest.mark.gpu

IMG = (nat.F_RGB, nat.F_DEPTH, nat.F_MASK)


def cameras(W, H):
    """The default eye's matrices, a close look-at whose near plane cuts the table, a 120-degree eye inside the arm, a tilted one."""
    a = W / H
    return [(look_at((0.01, 0.0, 1.2), np.asarray(load_model()['table_pos'], np.float64), (0.0, 0.0, 1.0)), perspective(80.0, a, 0.1, 100.0)),
            (look_at((-0.05, 0.1, 0.34), (0.3, -0.05, 0.2), (0.0, 0.0, 1.0)), perspective(80.0, a, 0.1, 100.0)),
            (look_at((-0.55, 0.0, 0.30), (-0.55, 0.05, 1.2), (1.0, 0.0, 0.0)), perspective(120.0, a, 0.1, 100.0)),
            (view_from_yaw_pitch_roll((0.05, 0.0, 0.35), 0.9, 40.0, -35.0, 15.0), perspective(70.0, a, 0.1, 100.0))]


def stack(cams, N):
    return (np.stack([cams[i % len(cams)][0] for i in range(N)]).astype(np.float32),
            np.stack([cams[i % len(cams)][1] for i in range(N)]).astype(np.float32))


def images(env):
    return [env.host(f) for f in IMG]


def assert_env_equal(a, b, envs, label):
    for f, x, y in zip(IMG, a, b):
        for i in envs:
            assert np.array_equal(x[i], y[i]), (label, f, i)


@pytest.mark.parametrize('W,H', [(128, 128), (320, 240)])
def test_per_env_cameras_equal_shared_handles_bitwise(W, H):
    """12 envs on 4 cameras against 4 shared handles: identical states and identical bytes in every env over 30 steps of
    per-env render flags, after the cameras changed on handles that had rendered already (stale envs, full copy)."""
    N, T = 12, 30
    cams = cameras(W, H)
    views, projs = stack(cams, N)
    pe = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    sh = [BatchedREALRobotEnv(N, objects=3, width=W, height=H) for _ in cams]
    every = [pe] + sh
    for t in range(3):
        for e in every:
            e.step(synthetic_actions(range(N), t, seed=21), render=True)
    pe.set_env_cameras(views, projs)
    for k, (v, p) in enumerate(cams):
        sh[k].set_camera(v, p)
    rng = np.random.default_rng(3)
    for t in range(3, 3 + T):
        flags = (rng.random(N) < 0.6).astype(np.uint8)
        cmd = synthetic_actions(range(N), t, seed=21)
        for e in every:
            e.step(cmd, render=flags)
        st = pe.state
        for e in sh:
            assert np.array_equal(st, e.state, equal_nan=True), t
        a = images(pe)
        for k, e in enumerate(sh):
            assert_env_equal(a, images(e), range(k, N, len(cams)), 'step %d camera %d' % (t, k))
    for e in every:
        e.close()


def _classes_run(env_list, N, steps, seed):
    """Steps every handle with the same full-range commands, rendering every step; returns the classes of the last step."""
    for t in range(steps):
        cmd = synthetic_actions(range(N), t, seed=seed)
        for e in env_list:
            e.step(cmd, render=True)
    return env_list[0].host(nat.F_ENV_CLASS)


def test_every_step_path_at_4096_envs():
    """4096 envs on the full-range workload, per-env cameras against shared handles at the same N: envs of every solver class
    (k_render_setup, the light solve's fused set-up, the heavy renders).  States are compared first; if the placement made them
    differ, the shared handles are given the per-env handle's state and rendered, and the images are compared then."""
    N, W, H = 4096, 128, 128
    cams = cameras(W, H)
    views, projs = stack(cams, N)
    pe = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    sh = [BatchedREALRobotEnv(N, objects=3, width=W, height=H) for _ in cams]
    pe.set_env_cameras(views, projs)
    for k, (v, p) in enumerate(cams):
        sh[k].set_camera(v, p)
    classes = set()
    for rnd in range(4):
        cls = _classes_run([pe] + sh, N, 25, seed=33)
        classes |= set(np.unique(cls).tolist())
        pick = {0, N - 1, 1, 2, 3}
        for c in np.unique(cls):
            pick |= set(np.flatnonzero(cls == c)[:8].tolist())
        st = pe.state
        same = all(np.array_equal(st, e.state, equal_nan=True) for e in sh)
        print('round %d: classes %s, states %s' % (rnd, np.bincount(cls, minlength=3).tolist(), 'equal' if same else 'DIFFER'))
        if not same:
            for e in sh:
                e.state = st
                e.render()
            pe.render()
        a = images(pe)
        for k, e in enumerate(sh):
            assert_env_equal(a, images(e), sorted(i for i in pick if i % len(cams) == k), 'round %d camera %d' % (rnd, k))
    print('classes seen:', sorted(classes))
    assert {0, 1} <= classes
    for e in [pe] + sh:
        e.close()


def draw_cameras(N, W, H, seed):
    rng = np.random.default_rng(seed)
    v0 = cameras(W, H)[0][0]
    views, projs = [], []
    for i in range(N):
        ang = np.radians(rng.uniform(-3, 3, 3))
        cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, rng.uniform(-0.03, 0.03, 3)
        views.append(T @ v0)
        projs.append(perspective(rng.uniform(75, 85), W / H, 0.1, 100.0))
    return np.array(views, np.float32), np.array(projs, np.float32)


def check_ray_caster(env, envs, views, projs, W, H, label):
    st = env.state
    rgb, dep, msk = images(env)
    err = env.host(nat.F_ERRFLAGS)
    for i in envs:
        assert err[i] & 8 == 0, (label, i)
        h = nc.render(st[i].astype(np.float64), 3, W, H, views[i].astype(np.float64), projs[i].astype(np.float64))
        rr = h['rows']
        compare((rgb[i][rr], dep[i][rr], msk[i][rr]), h, '%s env %d' % (label, i))


def test_drawn_cameras_against_the_ray_caster_at_4096_envs():
    N, W, H = 4096, 128, 128
    views, projs = draw_cameras(N, W, H, seed=5)
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    env.set_env_cameras(views, projs)
    for t in range(60):
        env.step(synthetic_actions(range(N), t, seed=9), render=True)
    cls = env.host(nat.F_ENV_CLASS)
    pick = [int(np.flatnonzero(cls == c)[0]) for c in np.unique(cls)]         # every class, then random envs up to 16
    for i in np.random.default_rng(1).choice(N, 32, replace=False).tolist():
        if len(pick) < 16 and i not in pick:
            pick.append(i)
    check_ray_caster(env, pick, views, projs, W, H, '4096 drawn')
    env.close()


def test_masked_semantics_lifetime_and_validation():
    N, W, H = 8, 128, 128
    cams = cameras(W, H)
    views, projs = stack(cams[1:], N)
    mask = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.uint8)
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    ref = BatchedREALRobotEnv(N, objects=3, width=W, height=H)       # never in per-env mode
    for t in range(5):
        for e in (env, ref):
            e.step(synthetic_actions(range(N), t, seed=2), render=True)
    before = images(env)
    count0 = env.host(nat.F_FRAG_COUNT)
    env.set_env_cameras(views, projs, env_mask=mask)
    after = images(env)
    assert_env_equal(before, after, range(N), 'no render yet')        # every env keeps its last frame
    count1 = env.host(nat.F_FRAG_COUNT)
    assert np.array_equal(count0[mask == 0], count1[mask == 0])
    # a non-finite matrix of a masked env raises and changes nothing; one of an unmasked env is not read
    bad = views.copy()
    bad[2, 1, 1] = np.nan
    with pytest.raises(nat.NativeError):
        env.set_env_cameras(bad, projs, env_mask=mask)
    env.set_env_cameras(bad, projs, env_mask=np.zeros(N, np.uint8))
    assert_env_equal(before, images(env), range(N), 'after refused call')
    # the next frames: unmasked envs as on the handle never put in per-env mode, masked envs as on shared handles of their camera
    sh = {}
    for k in range(3):
        sh[k] = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
        for t in range(5):
            sh[k].step(synthetic_actions(range(N), t, seed=2), render=True)
        sh[k].set_camera(*cams[1 + k])
    for t in range(5, 12):
        flags = np.ones(N, np.uint8) if t > 6 else np.array([1, 0, 1, 0, 1, 0, 1, 0], np.uint8)
        for e in [env, ref] + list(sh.values()):
            e.step(synthetic_actions(range(N), t, seed=2), render=flags)
        a = images(env)
        assert_env_equal(a, images(ref), np.flatnonzero(mask == 0), 'unmasked step %d' % t)
        for i in np.flatnonzero(mask):
            if flags[i]:
                assert_env_equal(a, images(sh[i % 3]), [i], 'masked step %d' % t)
            else:
                assert_env_equal(a, before, [i], 'masked, not rendered, step %d' % t)
    # cameras are handle settings: reset, state, teleports and restore keep them
    ck = env.checkpoint()
    env.reset(np.array([1, 1, 0, 0, 0, 0, 0, 0], np.uint8))
    env.state = env.state
    env.set_object_poses(env.host(nat.F_OBJ_POSE).reshape(N, 3, 7), env_mask=np.ones(N, np.uint8))
    env.restore(ck)
    for e in [ref] + list(sh.values()):
        e.restore(e.checkpoint())
    for t in range(12, 15):
        for e in [env, ref] + list(sh.values()):
            e.step(synthetic_actions(range(N), t, seed=2), render=True)
    a = images(env)
    assert_env_equal(a, images(ref), np.flatnonzero(mask == 0), 'unmasked after restore')
    for i in np.flatnonzero(mask):
        assert_env_equal(a, images(sh[i % 3]), [i], 'masked after restore')
    # set_camera(None, None) then a full render: a fresh handle at the same state
    env.set_camera(None, None)
    env.render()
    fresh = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    fresh.state = env.state
    fresh.render()
    assert_env_equal(images(env), images(fresh), range(N), 'back to the shared camera')
    for e in [env, ref, fresh] + list(sh.values()):
        e.close()


def test_vector_env_camera_randomization_against_the_ray_caster():
    from real_robots_amd.vector import REALRobotVectorEnv
    W, H, n = 128, 96, 6
    v = REALRobotVectorEnv(n, eye_width=W, eye_height=H, max_episode_steps=4, additional_obs=True,
                           camera_randomization={'translation': 0.03, 'rotation': 3.0, 'fov': (75, 85)})
    obs, info = v.reset(seed=11)
    cam = info['camera']
    check = [0, 3, 5]

    def against(obs, cam, label):
        st = v._be.state
        for i in check:
            h = nc.render(st[i].astype(np.float64), 3, W, H, cam['view'][i].astype(np.float64), cam['proj'][i].astype(np.float64))
            rr = h['rows']
            compare((obs['retina'][i][rr], obs['depth'][i][rr], obs['mask'][i][rr]), h, '%s env %d' % (label, i))
    against(obs, cam, 'reset')
    rng = np.random.default_rng(0)
    for t in range(4):
        obs, _, _, trunc, info = v.step(rng.uniform(-0.3, 0.3, (n, 9)).astype(np.float32))
    assert trunc.all() and info['_camera'].all()
    assert not np.array_equal(info['camera']['view'], cam['view'])
    against(obs, info['camera'], 'autoreset')
    v.close()
