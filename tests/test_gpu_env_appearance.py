"""GPU tests (-m gpu) of per-env appearance (rr_set_env_appearance): drawn colours and lights against the float64 ray caster of
tests/numpy_camera.py with that env's colours and light patched in (and a negative control: the neighbour's appearance breaks the
RGB bound only); a known answer on the cube's top face; the default appearance set explicitly changes no byte; an env reads its
own record only (permuted handles); a change followed by render() equals a fresh handle; physics untouched; mask, validation and
lifetime rules; the vector env's appearance_randomization; the facade's changeVisualShape."""
import functools

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_camera as nc
from tests.test_gpu_env_cameras import assert_env_equal, cameras, images
from tests.test_numpy_camera import compare

pytestmark = pytest.mark.gpu

IMG = (nat.F_RGB, nat.F_DEPTH, nat.F_MASK)
NI = len(nc.model()['owner'])
# the cases of the ray-caster comparison: name -> (W, H, index into cameras(W, H): 0 the eye, 1 the close look-at across the table)
CASES = {'eye128': (128, 128, 0), 'eye320x240': (320, 240, 0), 'close128': (128, 128, 1)}
N_RC, STEPS_RC, SEED_APP, SEED_ACT = 8, 40, 17, 9


def draw_appearance(N, seed, lo=0.2, hi=1.0):
    """Colours uniform in [lo, hi] per channel and instance, lights uniform on the upper hemisphere (z >= 0.05)."""
    rng = np.random.default_rng(seed)
    col = rng.uniform(lo, hi, size=(N, NI, 3)).astype(np.float32)
    v = rng.normal(size=(N, 3))
    v[:, 2] = np.abs(v[:, 2])
    v /= np.linalg.norm(v, axis=1)[:, None]
    v[:, 2] = np.maximum(v[:, 2], 0.05)
    return col, v.astype(np.float32)


def patched_render(monkeypatch, state, nobj, W, H, view, proj, colours, light):
    """nc.render of one env with its colours (float32 values, as the device holds them) and its light (normalised in float64)."""
    M = dict(nc.model())
    M['color'] = np.asarray(colours, np.float64).copy()
    l = np.asarray(light, np.float64)
    monkeypatch.setattr(nc, '_M', M)
    monkeypatch.setattr(nc, 'LIGHT', l / np.linalg.norm(l))
    return nc.render(np.asarray(state, np.float64), nobj, W, H, None if view is None else np.asarray(view, np.float64),
                     None if proj is None else np.asarray(proj, np.float64))


@functools.lru_cache(maxsize=None)
def rc_frames(case):
    """8 envs with drawn appearance after 40 steps of synthetic_actions, rendered: (state, rgb, depth, mask, colours, lights, view, proj)."""
    W, H, k = CASES[case]
    view, proj = cameras(W, H)[k]
    col, light = draw_appearance(N_RC, SEED_APP)
    env = BatchedREALRobotEnv(N_RC, objects=3, width=W, height=H)
    if k:
        env.set_camera(view, proj)
    env.set_env_appearance(colours=col, light_dirs=light)
    for t in range(STEPS_RC):
        env.step(synthetic_actions(range(N_RC), t, seed=SEED_ACT), render=(t == STEPS_RC - 1))
    out = (env.state, *images(env), env.env_appearance()['colours'], light, np.float32(view), np.float32(proj))
    assert (env.host(nat.F_ERRFLAGS) & 8 == 0).all()
    env.close()
    return out


@pytest.mark.parametrize('case', list(CASES))
def test_drawn_appearance_against_the_ray_caster(case, monkeypatch):
    """Every env's frame against the float64 ray caster with that env's colours and light, the project's bounds unchanged
    (tests/test_numpy_camera.py compare: mask identical, RGB within 1, depth bounds, undecided caps 0.5 % mask / 2 % RGB).
    The patched caster alone on the CPU, on the oracle's states of this workload (8 envs, 40 steps of synthetic_actions seed 9,
    appearance seed 17, colours uniform in [0.2, 1]): worst undecided share 0.13 % (mask) and 0.19 % (RGB) at eye 128 x 128,
    0.25 % and 0.29 % at eye 320 x 240, 0.01 % and 0.38 % at the close camera -- under the caps with the proposed ranges."""
    W, H, k = CASES[case]
    st, rgb, dep, msk, col, light, view, proj = rc_frames(case)
    assert np.array_equal(col, draw_appearance(N_RC, SEED_APP)[0])
    for i in range(N_RC):
        h = patched_render(monkeypatch, st[i], 3, W, H, view, proj, col[i], light[i])
        compare((rgb[i], dep[i], msk[i]), h, '%s env %d' % (case, i))


def test_negative_control_neighbours_appearance_breaks_rgb_only(monkeypatch):
    """Env i's frame against env (i + 1)'s colours and light: the RGB bound breaks, mask and depth stay within theirs."""
    case = 'eye128'
    W, H, k = CASES[case]
    st, rgb, dep, msk, col, light, view, proj = rc_frames(case)
    for i in range(N_RC):
        j = (i + 1) % N_RC
        h = patched_render(monkeypatch, st[i], 3, W, H, view, proj, col[j], light[j])
        broken = compare((rgb[i], dep[i], msk[i]), h, None)
        print('env %d against the appearance of env %d:' % (i, j), broken)
        assert 'rgb' in broken and not {'mask', 'depth_far', 'depth_near', 'und_mask', 'und_bad'} & set(broken), (i, broken)


KNOWN = [((0.9, 0.5, 0.25), (0.0, 0.0, 1.0)), ((0.3, 1.0, 0.7), (0.6, -0.3, 0.5)), ((1.2, 0.6, 0.45), (-0.2, 0.7, 0.25))]


@pytest.mark.parametrize('c,l', KNOWN)
def test_known_answer_cube_top_face(c, l):
    """The cube upright under a camera looking straight down: its top face has n = +z, so with colour c and unit light l every
    pixel of it is floor(texel * c * (0.6 + 0.35 max(l_z, 0) + 0.05 s)), s = max(r_z, 0)^2 with r = 2 l_z z - l, within 1."""
    from tests.test_numpy_camera import cube_top_view
    o, h, top, cube = cube_top_view()
    W = H = 256
    view, proj = nc.look_at([0.05, 0.0, 0.55], [0.05, 0.0, 0.30], [0, 1, 0]), nc.perspective(40, 1.0)
    env = BatchedREALRobotEnv(1, objects=1, width=W, height=H)
    env.state = np.asarray(o.state, np.float32)[None]
    env.set_camera(view, proj)
    col = env.default_env_appearance()['colours']
    col[0, cube] = c
    env.set_env_appearance(colours=col, light_dirs=l)
    env.render()
    rgb, _, msk = images(env)
    env.close()
    lu = np.asarray(l, np.float64) / np.linalg.norm(l)
    r = 2 * lu[2] * np.array([0.0, 0.0, 1.0]) - lu
    s = max(r[2] / np.linalg.norm(r), 0.0) ** 2
    shade = 0.6 + 0.35 * max(lu[2], 0.0) + 0.05 * s
    expect = np.minimum(np.floor(h['tex_rgb'][top] * np.asarray(c, np.float64) * shade), 255)
    assert top.sum() > 3000 and (msk[0][top] == 2).all()
    err = np.abs(rgb[0][top].astype(np.float64) - expect).max()
    print('cube top, colour %s light %s: shade %.4f, worst error %g grey levels over %d pixels' % (c, l, shade, err, top.sum()))
    assert err <= 1


def _flags(rng, N):
    return (rng.random(N) < 0.6).astype(np.uint8)


@pytest.mark.parametrize('W,H', [(128, 128), (320, 240)])
def test_default_appearance_set_explicitly_changes_no_byte(W, H):
    """A handle whose appearance is set to default_env_appearance() against a handle that never called it: 30 steps of per-env
    render flags, RGB, depth and mask byte for byte -- the float32 default light equals the shader's literals bit for bit."""
    N, T = 12, 30
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    a.set_env_appearance(**a.default_env_appearance())
    assert all(np.array_equal(a.env_appearance()[k], b.env_appearance()[k]) for k in ('colours', 'light_dirs'))
    rng = np.random.default_rng(4)
    for t in range(T):
        flags = np.ones(N, np.uint8) if t == 0 else _flags(rng, N)
        cmd = synthetic_actions(range(N), t, seed=21)
        for e in (a, b):
            e.step(cmd, render=flags)
        assert np.array_equal(a.state, b.state, equal_nan=True), t
        assert_env_equal(images(a), images(b), range(N), 'step %d' % t)
    a.close()
    b.close()


def test_default_appearance_every_step_path_at_4096_envs():
    """The same at 4096 envs on the full-range workload, where every solver class occurs (k_render_setup, the light solve's fused
    set-up, the heavy renders).  States first; if the placement made them differ, the plain handle is given the other's state and
    both render, and the images are compared then."""
    N, W, H = 4096, 128, 128
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    a.set_env_appearance(**a.default_env_appearance())
    classes = set()
    for rnd in range(3):
        for t in range(25):
            cmd = synthetic_actions(range(N), 25 * rnd + t, seed=33)
            for e in (a, b):
                e.step(cmd, render=True)
        cls = a.host(nat.F_ENV_CLASS)
        classes |= set(np.unique(cls).tolist())
        st = a.state
        same = np.array_equal(st, b.state, equal_nan=True)
        print('round %d: classes %s, states %s' % (rnd, np.bincount(cls, minlength=3).tolist(), 'equal' if same else 'DIFFER'))
        if not same:
            b.state = st
            b.render()
            a.render()
        for x, y in zip(images(a), images(b)):
            assert np.array_equal(x, y), rnd
    assert {0, 1} <= classes
    a.close()
    b.close()


def test_an_env_reads_its_own_record_only():
    """Two handles of 12 envs, the second with states, commands, render flags and appearance rows permuted: permuted images, byte
    for byte, over 30 steps of per-env render flags -- the appearance set after both had rendered (stale path) and changed once
    more for a masked subset midway."""
    N, W, H, T = 12, 128, 128, 30
    perm = np.random.default_rng(8).permutation(N)
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    col, light = draw_appearance(N, 31)
    col2, light2 = draw_appearance(N, 32, 0.0, 1.5)
    sub = (np.arange(N) % 3 == 1).astype(np.uint8)
    for t in range(3):
        cmd = synthetic_actions(range(N), t, seed=5)
        a.step(cmd, render=True)
        b.step(cmd[perm], render=True)
    a.set_env_appearance(colours=col, light_dirs=light)
    b.set_env_appearance(colours=col[perm], light_dirs=light[perm])
    rng = np.random.default_rng(6)
    for t in range(3, 3 + T):
        if t == 3 + T // 2:
            a.set_env_appearance(colours=col2, light_dirs=light2, env_mask=sub)
            b.set_env_appearance(colours=col2[perm], light_dirs=light2[perm], env_mask=sub[perm])
        flags = _flags(rng, N)
        cmd = synthetic_actions(range(N), t, seed=5)
        a.step(cmd, render=flags)
        b.step(cmd[perm], render=flags[perm])
        assert np.array_equal(a.state[perm], b.state, equal_nan=True), t
        for f, x, y in zip(IMG, images(a), images(b)):
            assert np.array_equal(x[perm], y), (t, f)
    want = np.where(sub[:, None, None].astype(bool), col2, col)
    assert np.array_equal(a.env_appearance()['colours'], want) and np.array_equal(b.env_appearance()['colours'], want[perm])
    ia = images(a)[0]
    assert not np.array_equal(ia[0], ia[1])
    a.close()
    b.close()


def test_incremental_equals_full():
    """After a change on a handle that has rendered, with no step in between, render() gives byte for byte what a fresh handle with
    the same state and appearance renders; the envs outside the mask keep their bytes."""
    N, W, H = 8, 128, 128
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    for t in range(12):
        env.step(synthetic_actions(range(N), t, seed=2), render=True)
    before = images(env)
    col, light = draw_appearance(N, 41)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    env.set_env_appearance(colours=col, light_dirs=light, env_mask=mask)
    assert_env_equal(before, images(env), range(N), 'no render yet')
    env.render()
    after = images(env)
    assert_env_equal(before, after, np.flatnonzero(mask == 0), 'outside the mask')
    for i in np.flatnonzero(mask):
        assert not np.array_equal(before[0][i], after[0][i]), i
        assert np.array_equal(before[1][i], after[1][i]) and np.array_equal(before[2][i], after[2][i]), i
    fresh = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    fresh.state = env.state
    fresh.set_env_appearance(**env.env_appearance())
    fresh.render()
    assert_env_equal(after, images(fresh), range(N), 'fresh handle')
    # ... and a second change of other envs, light only
    mask2 = np.array([0, 1, 1, 0, 0, 0, 0, 1], np.uint8)
    env.set_env_appearance(light_dirs=[0.3, 0.2, 0.4], env_mask=mask2)
    env.render()
    fresh2 = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    fresh2.state = env.state
    fresh2.set_env_appearance(**env.env_appearance())
    fresh2.render()
    assert_env_equal(images(env), images(fresh2), range(N), 'fresh handle, second change')
    assert_env_equal(after, images(env), np.flatnonzero(mask2 == 0), 'outside the second mask')
    for e in (env, fresh, fresh2):
        e.close()


def test_physics_untouched():
    """States, touch sensors and contact counts bitwise those of a plain handle over 200 steps at 512 envs, appearance in force."""
    N, W, H = 512, 128, 128
    a = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    b = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    col, light = draw_appearance(N, 51)
    a.set_env_appearance(colours=col, light_dirs=light)
    for t in range(200):
        cmd = synthetic_actions(range(N), t, seed=33)
        for e in (a, b):
            e.step(cmd, render=(t % 2 == 0))
        if t % 10 == 9 or t < 5:
            assert np.array_equal(a.state, b.state, equal_nan=True), t
            assert np.array_equal(a.host(nat.F_TOUCH), b.host(nat.F_TOUCH)), t
            assert np.array_equal(a.host(nat.F_CONTACT_COUNT), b.host(nat.F_CONTACT_COUNT)), t
    assert a.host(nat.F_CONTACT_COUNT).max() > 0
    ra, rb = images(a), images(b)
    assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]) and not np.array_equal(ra[0], rb[0])
    a.close()
    b.close()


def test_masked_semantics_validation_lifetime_and_cameras():
    N, W, H = 8, 128, 128
    cams = cameras(W, H)
    col, light = draw_appearance(N, 61)
    mask = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.uint8)
    env = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    owner = env.render_instances()
    assert owner.shape == (NI, 4) and np.array_equal(owner, nc.model()['owner'])
    d = env.default_env_appearance()
    assert np.array_equal(d['colours'][3], nc.model()['color'].astype(np.float32)) and np.allclose(d['light_dirs'], nc.LIGHT, atol=1e-7)

    def fresh_like(e, camera=None, env_cams=None):
        f = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
        f.state = e.state
        if camera is not None:
            f.set_camera(*camera)
        if env_cams is not None:
            f.set_env_cameras(*env_cams)
        f.set_env_appearance(**e.env_appearance())
        f.render()
        out = images(f)
        f.close()
        return out
    for t in range(5):
        env.step(synthetic_actions(range(N), t, seed=2), render=True)
    before = images(env)
    count0 = env.host(nat.F_FRAG_COUNT)
    env.set_env_appearance(colours=col, light_dirs=light, env_mask=mask)
    assert_env_equal(before, images(env), range(N), 'no render yet')
    assert np.array_equal(count0[mask == 0], env.host(nat.F_FRAG_COUNT)[mask == 0])
    got = env.env_appearance()
    assert np.array_equal(got['colours'][mask == 1], col[mask == 1]) and np.array_equal(got['colours'][mask == 0], d['colours'][mask == 0])
    assert np.array_equal(got['light_dirs'][mask == 0], d['light_dirs'][mask == 0])
    assert np.allclose(got['light_dirs'][mask == 1], light[mask == 1] / np.linalg.norm(light[mask == 1], axis=1)[:, None], atol=1e-6)
    # validation: the library refuses a bad row of a masked env (the Python layer is bypassed), names the env, changes nothing;
    # a bad row of an unmasked env is not read
    L, h = env.L, env.h
    for what, bad_c, bad_l in (('colour', -1.0, None), ('colour', np.nan, None), ('light', None, (0.0, 0.0, 0.0)),
                               ('light', None, (np.inf, 0.0, 1.0)), ('light', None, (0.0, 1e-8, 0.0))):
        c2, l2 = col.copy(), light.copy()
        if bad_c is not None:
            c2[2, 5, 1] = bad_c
        if bad_l is not None:
            l2[2] = bad_l
        assert L.rr_set_env_appearance(h, c2.ctypes.data, l2.ctypes.data, mask.ctypes.data) == -1
        assert b'env 2' in L.rr_last_error() and what.encode() in L.rr_last_error()
        after = env.env_appearance()
        assert np.array_equal(after['colours'], got['colours']) and np.array_equal(after['light_dirs'], got['light_dirs'])
        assert L.rr_set_env_appearance(h, c2.ctypes.data, l2.ctypes.data, np.zeros(N, np.uint8).ctypes.data) == 0
        after = env.env_appearance()
        assert np.array_equal(after['colours'], got['colours']) and np.array_equal(after['light_dirs'], got['light_dirs'])
    assert L.rr_set_env_appearance(h, None, None, mask.ctypes.data) == -1
    assert_env_equal(before, images(env), range(N), 'after the refused calls')
    # the next frames: per-env flags; unmasked envs as a plain handle, masked envs once rendered as a fresh handle
    ref = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    for t in range(5):
        ref.step(synthetic_actions(range(N), t, seed=2), render=True)
    flags = np.array([1, 0, 1, 0, 1, 0, 1, 0], np.uint8)
    for e in (env, ref):
        e.step(synthetic_actions(range(N), 5, seed=2), render=flags)
    a = images(env)
    assert_env_equal(a, images(ref), np.flatnonzero(mask == 0), 'unmasked')
    assert_env_equal(a, before, [i for i in range(N) if mask[i] and not flags[i]], 'masked, not rendered')
    full = fresh_like(env)
    assert_env_equal(a, full, [i for i in range(N) if flags[i]], 'rendered')
    # lifetime: reset, state, teleports and restore keep the appearance; checkpoints do not carry it
    ck = env.checkpoint()
    plain = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    assert plain.checkpoint().nbytes == ck.nbytes
    plain.restore(ck)
    assert np.array_equal(plain.env_appearance()['colours'], d['colours'])
    plain.close()
    env.reset(np.array([1, 1, 0, 0, 0, 0, 0, 0], np.uint8))
    env.state = env.state
    env.set_object_poses(env.host(nat.F_OBJ_POSE).reshape(N, 3, 7), env_mask=np.ones(N, np.uint8))
    env.restore(ck)
    assert np.array_equal(env.env_appearance()['colours'], got['colours'])
    env.step(synthetic_actions(range(N), 6, seed=2), render=True)
    assert_env_equal(images(env), fresh_like(env), range(N), 'after restore')
    # rr_set_camera with an appearance in force: one camera for every env, the appearance stays
    env.set_camera(*cams[3])
    env.render()
    assert_env_equal(images(env), fresh_like(env, camera=cams[3]), range(N), 'set_camera after')
    # per-env cameras on top, for some envs; then the appearance back to the model's with the cameras staying
    views = np.stack([cams[i % 4][0] for i in range(N)]).astype(np.float32)
    projs = np.stack([cams[i % 4][1] for i in range(N)]).astype(np.float32)
    cmask = np.array([1, 1, 0, 0, 1, 1, 0, 0], np.uint8)
    env.set_env_cameras(views, projs, env_mask=cmask)
    env.step(synthetic_actions(range(N), 7, seed=2), render=True)
    v2, p2 = views.copy(), projs.copy()
    v2[cmask == 0], p2[cmask == 0] = np.float32(cams[3][0]), np.float32(cams[3][1])
    assert_env_equal(images(env), fresh_like(env, env_cams=(v2, p2)), range(N), 'set_env_cameras after')
    env.set_env_appearance()
    assert np.array_equal(env.env_appearance()['colours'], d['colours']) and np.array_equal(env.env_appearance()['light_dirs'], d['light_dirs'])
    env.render()
    cam_only = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    cam_only.state = env.state
    cam_only.set_env_cameras(v2, p2)
    cam_only.render()
    assert_env_equal(images(env), images(cam_only), range(N), 'appearance off, cameras stay')
    # cameras first, appearance after (the layers exist already); set_camera ends the cameras, not the appearance
    cam_only.set_env_appearance(colours=col, light_dirs=light)
    cam_only.render()
    assert_env_equal(images(cam_only), fresh_like(cam_only, env_cams=(v2, p2)), range(N), 'set_env_cameras before')
    cam_only.set_camera(None, None)
    cam_only.render()
    assert_env_equal(images(cam_only), fresh_like(cam_only), range(N), 'set_camera(None, None) with appearance')
    # back to the shared layer: a handle that never had an appearance
    cam_only.set_env_appearance()
    cam_only.render()
    never = BatchedREALRobotEnv(N, objects=3, width=W, height=H)
    never.state = cam_only.state
    never.render()
    assert_env_equal(images(cam_only), images(never), range(N), 'back to the shared layer')
    for t in range(8, 11):
        cmd = synthetic_actions(range(N), t, seed=2)
        for e in (cam_only, never):
            e.step(cmd, render=True)
    assert_env_equal(images(cam_only), images(never), range(N), 'steps on the shared layer')
    for e in (env, ref, cam_only, never):
        e.close()


def test_vector_env_appearance_randomization(monkeypatch):
    from real_robots_amd.vector import REALRobotVectorEnv
    W, H, n = 128, 96, 16
    v = REALRobotVectorEnv(n, eye_width=W, eye_height=H, max_episode_steps=4, additional_obs=True,
                           appearance_randomization={'colour': (0.5, 1.0), 'brightness': (0.8, 1.2), 'light': 40.0})
    obs, info = v.reset(seed=11)
    app = info['appearance']
    assert app['colours'].shape == (n, NI, 3) and app['light_dirs'].shape == (n, 3)
    assert np.array_equal(v._be.env_appearance()['colours'], app['colours'])
    # two envs with different draws, same state: other RGB, same mask and depth
    assert not np.array_equal(obs['retina'][0], obs['retina'][1])
    assert np.array_equal(obs['mask'][0], obs['mask'][1]) and np.array_equal(obs['depth'][0], obs['depth'][1])

    def against(obs, app, label):
        st = v._be.state
        for i in (0, 7, 15):
            h = patched_render(monkeypatch, st[i], 3, W, H, None, None, app['colours'][i], app['light_dirs'][i])
            compare((obs['retina'][i], obs['depth'][i], obs['mask'][i]), h, '%s env %d' % (label, i))
    against(obs, app, 'reset')
    rng = np.random.default_rng(0)
    for t in range(4):
        obs, _, _, trunc, info = v.step(rng.uniform(-0.3, 0.3, (n, 9)).astype(np.float32))
    assert trunc.all() and info['_appearance'].all()
    assert not np.array_equal(info['appearance']['colours'], app['colours'])
    against(obs, info['appearance'], 'autoreset')
    v.close()


def test_facade_change_visual_shape():
    from real_robots_amd.envs.env import REALRobotEnv
    env = REALRobotEnv(objects=3, eye_width=128, eye_height=128)
    env.reset()
    (retina0, mask, _), frame0 = env.get_retina(), env.render('rgb_array').copy()
    env._p.changeVisualShape(2, -1, rgbaColor=[0.2, 0.9, 0.3, 1.0])
    retina1, frame1 = env.get_retina()[0], env.render('rgb_array').copy()
    cube = mask == 2
    assert cube.sum() > 20
    assert (retina1[cube] != retina0[cube]).any(axis=-1).mean() > 0.9 and np.array_equal(retina1[~cube], retina0[~cube])
    changed = (frame1 != frame0).any(axis=-1)
    assert changed.sum() > 20 and changed.mean() < 0.05
    # the cube's instance, and no other, has that colour: a batched handle told so directly renders the same bytes
    direct = BatchedREALRobotEnv(1, objects=3, width=128, height=128)
    owner = direct.render_instances()
    col = direct.default_env_appearance()['colours']
    col[0, (owner[:, 0] == 2) & (owner[:, 1] == 0)] = [0.2, 0.9, 0.3]
    direct.state = env._backend().state
    direct.set_env_appearance(colours=col)
    direct.render()
    assert np.array_equal(direct.host(nat.F_RGB)[0], retina1)
    direct.close()
    env._p.changeVisualShape(1, -1, rgbaColor=(0.5, 0.5, 1.0))
    retina2 = env.get_retina()[0]
    table = mask == 1
    assert (retina2[table] != retina1[table]).any(axis=-1).mean() > 0.9 and np.array_equal(retina2[cube], retina1[cube])
    for args, kw in (((0, -1), dict(rgbaColor=[1, 0, 0, 1])), ((5, -1), dict(rgbaColor=[1, 0, 0, 1])), ((2, 0), dict(rgbaColor=[1, 0, 0, 1])),
                     ((2, -1), dict(rgbaColor=[1, 0, 0, 0.5])), ((2, -1), dict(specularColor=[1, 1, 1])), ((2, -1), dict())):
        with pytest.raises(NotImplementedError):
            env._p.changeVisualShape(*args, **kw)
    assert np.array_equal(env.get_retina()[0], retina2)
    env.close()
