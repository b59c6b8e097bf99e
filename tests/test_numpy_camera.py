"""CPU tests (-m "not gpu"): the oracle's rasteriser (oracle/rr_oracle.c rro_render) against the float64 numpy ray caster of
tests/numpy_camera.py -- an independent restatement of the camera contract (world-space rays instead of screen-space edge
functions, view-depth near test instead of polygon clipping, exact barycentrics instead of the perspective-correction
formula).

Bounds, at the pixels the helper calls decided (see tests/numpy_camera.py):
  mask identical; RGB within 1 grey level; depth within numpy_camera.depth_bound(w): DEPTH_FAR where the view depth w is
  >= 0.3 m, nearer max(DEPTH_NEAR, the GL depth of a DEPTH_W_ERR error in w).
  At most MAX_UNDECIDED_MASK of a frame's pixels undecided for the mask, MAX_UNDECIDED_RGB for RGB (at least one pixel each).
  At an undecided pixel the mask is still background or the uid of a triangle whose outline passes within 0.01 px.
Measured over the scenes below (float64 oracle): worst RGB error 0 grey levels, worst depth error 8.7e-7 (w >= 0.3 m) and
3.2e-6 nearer (at most 0.04 of the near bound), worst undecided fraction 0.25 % (mask) and 0.49 % (RGB), but 1.9 % of
4 x 1024 (CAP_OVERRIDE).  The device against the helper (tests/test_gpu_numpy_camera.py; float32 forward kinematics): worst
RGB error 0, depth 3.6e-6 (w >= 0.3 m) and 3.4e-5 nearer (0.33 of the near bound).  DEPTH_FAR = 8e-6 has 9.2x headroom
over the oracle and 2.2x over the device; the near bound is set by the device (3x headroom) and is loose for the oracle,
whose forward kinematics is exact."""
import time

import numpy as np
import pytest

from oracle.oracle import Oracle
from real_robots_amd import mathutil
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_camera as nc

DEPTH_FAR = nc.DEPTH_FAR
MAX_UNDECIDED_MASK, MAX_UNDECIDED_RGB = 0.005, 0.02
# 4 x 1024 squeezes the scene 256 x across: its nearly vertical outlines pass within 1e-3 px of a sample in ~2 % of the rows
CAP_OVERRIDE = {(4, 1024): 0.025}


def q11_from_cmd(cmd):
    q = np.zeros(11)
    q[:7] = cmd[:7]
    q[7] = q[9] = cmd[7]
    q[8] = q[10] = -cmd[8]
    return q


def quat(axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.append(a * np.sin(ang / 2), np.cos(ang / 2))


TILTED = [[0.05, 0.12, 0.33, *quat([1, 2, 0.5], 0.9)], [-0.12, -0.2, 0.36, *quat([-0.3, 1, 1], 2.1)],
          [0.25, 0.62, 0.31, *quat([0.7, -0.2, 1], -1.3)]]          # the third one partly outside the frustum


def near_camera_q():
    """Postures that put the gripper 0.08 .. 0.18 m under the eye: links cross the near plane."""
    from oracle.kinematics import inverse_kinematics, quat_from_euler
    out = []
    for t in ([0.0, 0.0, 1.02], [-0.05, 0.0, 1.12]):
        q = inverse_kinematics(np.zeros(11), t, quat_from_euler(0, 0, 0))
        q[7:11] = [0.4, -0.3, 0.4, -0.3]
        out.append(q)
    return out


def scene(name):
    """-> (oracle, n_objects, W, H, view, proj, rows)"""
    W, H, nobj, view, proj, rows = 128, 128, 3, None, None, None
    q, poses = None, None
    if name.startswith('size'):
        W, H = (int(x) for x in name[4:].split('x'))
        q = q11_from_cmd(synthetic_actions([3], 40, seed=5)[0] * 0.5)
        if W == 1024:
            rows = sorted(set(range(0, H, 64)) | set(range(63, H, 64)) | set(np.random.default_rng(0).choice(H, 16, replace=False).tolist()))
    elif name.startswith('swept'):
        k = int(name[5:])
        q = q11_from_cmd(synthetic_actions([k], 10 * k, seed=11)[0] * 0.8)
    elif name.startswith('nearcam'):
        q = near_camera_q()[int(name[7:])]
    elif name.startswith('tilted'):
        nobj = int(name[6:])
        poses = TILTED[:nobj]
    elif name.startswith('objects'):
        nobj = int(name[7:])
    elif name == 'envcam':
        W, H = 320, 240
        view, proj = nc.env_camera()
        q = q11_from_cmd(np.array([0.8, 0.6, 0, -1.0, 0, 0.5, 0, 0.3, 0.2]))
    elif name == 'nearplane':      # an eye 6 cm above the table top looking across it: the near plane cuts the table
        W, H = 128, 96
        view, proj = nc.look_at([-0.05, 0.1, 0.34], [0.3, -0.05, 0.2], [0, 0, 1]), nc.perspective(80, W / H)
    elif name == 'closeup':
        W, H = 160, 120
        view, proj = nc.look_at([0.22, -0.18, 0.52], [0.0, 0.0, 0.30], [0, 0, 1]), nc.perspective(80, W / H)
        poses = [[-0.02, 0.03, 0.33, *quat([0.2, 0.3, 1], 0.6)], TILTED[1]]
        nobj = 2
    else:
        assert name == 'home', name
    o = Oracle(nobj, W, H)
    if q is not None:
        s = o.state
        s[:11] = q
        o.state = s
    for k, p in enumerate(poses or []):
        o.set_object_pose(k, p)
    if view is not None:
        o.set_camera(view, proj)
    return o, nobj, W, H, view, proj, rows


SCENES = ['home', 'swept0', 'swept1', 'swept2', 'nearcam0', 'nearcam1', 'tilted1', 'tilted2', 'tilted3', 'objects1',
          'objects2', 'envcam', 'closeup', 'nearplane', 'size320x240', 'size64x48', 'size4x1', 'size4x1024', 'size132x97', 'size128x33',
          'size1024x960']


def compare(ref, h, label='', cap=None):
    """Check one frame (rgb, depth, mask over the helper's rows) against the helper's result `h`; returns the measured
    worst errors, or a list of broken bounds when `label` is None (negative controls)."""
    r, d, m = ref
    dm, dr = h['dec_mask'], h['dec_rgb']
    npx = dm.size
    cov = dm & (h['mask'] >= 0)
    rgbe = np.abs(r.astype(int) - h['rgb'].astype(int)).max(-1)
    de = np.abs(d.astype(np.float64) - h['depth'])
    far, near = cov & (h['w'] >= 0.3), cov & (h['w'] < 0.3)
    ratio = de[near] / nc.depth_bound(h['w'][near])
    st = dict(near_ratio=float(ratio.max(initial=0)), mask_mis=int((m[dm] != h['mask'][dm]).sum()), rgb=int(rgbe[dr].max(initial=0)),
              depth_far=float(de[far].max(initial=0)), depth_near=float(de[near].max(initial=0)),
              und_mask=int((~dm).sum()), und_rgb=int((~dr).sum()), npx=npx, near_px=int(near.sum()))
    und = ~dm
    bits = h['cand'][und]
    mu = m[und]
    st['und_bad'] = int(((mu >= 0) & ((bits >> np.maximum(mu, 0)) & 1 == 0)).sum() + ((mu < -1) | (mu > 30)).sum())
    broken = [k for k, bad in (('mask', st['mask_mis'] > 0), ('rgb', st['rgb'] > 1), ('depth_far', st['depth_far'] > DEPTH_FAR),
                               ('depth_near', st['near_ratio'] > 1),
                               ('und_mask', st['und_mask'] > max(1, (cap or MAX_UNDECIDED_MASK) * npx)),
                               ('und_rgb', st['und_rgb'] > max(1, max(cap or 0, MAX_UNDECIDED_RGB) * npx)), ('und_bad', st['und_bad'] > 0)) if bad]
    if label is None:
        return broken
    print('%-14s %4dx%-4d rows %4d: mask mismatches %d, worst rgb %d, depth %.2e (w >= 0.3) %.2e (nearer, %d px; %.2f of the '
          'bound), undecided mask %d rgb %d of %d' % (label, h['size'][0], h['size'][1], len(h['rows']), st['mask_mis'],
                                                      st['rgb'], st['depth_far'], st['depth_near'], st['near_px'], st['near_ratio'],
                                                      st['und_mask'], st['und_rgb'], npx))
    assert not broken, (label, broken, st)
    return st


@pytest.mark.parametrize('name', SCENES)
def test_oracle_matches_the_numpy_ray_caster(name):
    o, nobj, W, H, view, proj, rows = scene(name)
    t0 = time.time()
    h = nc.render(o.state, nobj, W, H, view, proj, rows=rows)
    dt = time.time() - t0
    r, d, m = o.render()
    rr = h['rows']
    st = compare((r[rr], d[rr], m[rr]), h, name, CAP_OVERRIDE.get((W, H)))
    assert (h['mask'] >= 0).any() or W * H < 8
    if W * H <= 128 * 128 and rows is None:
        assert dt < 3.0, dt                         # (about 0.2 s per 128 x 128 frame on one core)
    if name.startswith('nearcam'):
        assert st['near_px'] > 100                  # geometry nearer than 0.3 m, cut by the near plane, is in the frame


def test_helper_camera_matrices_restate_mathutil():
    """The helper's matrices (camera frame inverted, glFrustum) against the closed forms of real_robots_amd.mathutil."""
    for eye, tgt, up in (([0.01, 0, 1.2], [0, 0, 0.08], [0, 0, 1]), ([0.3, -0.2, 1.0], [0.1, 0.2, 0.3], [0, 0.1, 1]),
                         ([0.22, -0.18, 0.52], [0.0, 0.0, 0.30], [0, 0, 1])):
        assert np.abs(nc.look_at(eye, tgt, up) - mathutil.look_at(eye, tgt, up)).max() < 1e-12
    for fov, aspect in ((80, 1.0), (80, 320 / 240), (60, 4 / 1024), (95, 1024 / 960)):
        assert np.abs(nc.perspective(fov, aspect, 0.1, 100) - mathutil.perspective(fov, aspect, 0.1, 100)).max() < 1e-12
    for yaw, pitch in ((30, -30), (0, 0), (-120, -70), (200, 15)):
        v = mathutil.view_from_yaw_pitch_roll([0.1, -0.2, 0.4], 1.3, yaw, pitch, 0)
        assert np.abs(nc.yaw_pitch_view([0.1, -0.2, 0.4], 1.3, yaw, pitch) - v).max() < 1e-12
    v, p = nc.eye_camera(128, 128)
    assert np.abs(v - mathutil.look_at([0.01, 0, 1.2], nc.model()['table_pos'], [0, 0, 1])).max() < 1e-12


def cube_top_view():
    """The cube parked upright on the table under a camera looking straight down at it (fov 40, 256 x 256)."""
    W = H = 256
    view, proj = nc.look_at([0.05, 0.0, 0.55], [0.05, 0.0, 0.30], [0, 1, 0]), nc.perspective(40, 1.0)
    o = Oracle(1, W, H)
    o.set_object_pose(0, [0.05, 0.0, 0.3, 0, 0, 0, 1])
    o.set_camera(view, proj)
    h = nc.render(o.state, 1, W, H, view, proj)
    M = nc.model()
    cube = [i for i, ow in enumerate(M['owner']) if ow[0] == 2 and ow[1] == 0][0]
    k = np.searchsorted(M['tid'], np.maximum(h['tri'], 0))
    top = h['dec_rgb'] & (h['tri'] >= 0) & (M['inst'][k] == cube) & (M['nrm'][k][..., 2].min(-1) > 0.9999)
    return o, h, top, cube


def test_known_answer_cube_top_face_is_uniformly_shaded():
    """A face of known orientation: the cube's top face at rest has n = +z, so every pixel of it is floor(texel x colour x
    shade) with the one shade 0.6 + 0.35 l_z + 0.05 l_z^2 (r = 2 (n.l) n - l has r_z = l_z) -- in the oracle's frame and the
    helper's."""
    o, h, top, cube = cube_top_view()
    r, _, m = o.render()
    assert top.sum() > 3000
    lz = nc.LIGHT[2]
    shade = 0.6 + 0.35 * lz + 0.05 * lz * lz
    col = nc.model()['color'][cube]
    expect = np.minimum(np.floor(h['tex_rgb'][top] * col * shade), 255)
    assert (m[top] == 2).all()
    assert np.abs(r[top] - expect).max() <= 1 and np.abs(h['rgb'][top] - expect).max() == 0


def test_known_answer_texture_appears_the_right_way_round():
    """Texture orientation: v runs UP the picture (GL), so the texel of (u, v) is the image file's pixel at column u w and row
    (1 - v) h counted from the top.  On the cube's top face the oracle's pixels must show the file that way round and not
    flipped top to bottom: at every pixel where the two readings differ, the oracle shows the upright one."""
    from real_robots_amd.model import load_model
    o, h, top, cube = cube_top_view()
    r, _, _ = o.render()
    M = nc.model()
    off, tw, th = M['tex_info'][M['owner'][cube][3]]
    img = np.asarray(load_model()['tex_data'][off:off + tw * th, :3]).reshape(th, tw, 3).astype(np.float64)   # file order
    uv = h['uv'][top]
    shade = 0.6 + 0.35 * nc.LIGHT[2] + 0.05 * nc.LIGHT[2] ** 2
    col = np.minimum((uv[:, 0] * tw).astype(int), tw - 1)
    right = img[np.minimum(((1 - uv[:, 1]) * th).astype(int), th - 1), col]
    flipped = img[np.minimum((uv[:, 1] * th).astype(int), th - 1), col]
    got = r[top].astype(np.float64)
    # judged where the two readings differ by more than 2 grey levels (the upright reading of the top face is the atlas's red
    # patch, the flipped one lands on the patches printed at the mirrored rows)
    distinct = np.abs(np.floor(right * shade) - np.floor(flipped * shade)).max(-1) > 2
    ok_right = (np.abs(got - np.floor(right * shade)).max(-1) <= 1)[distinct].mean()
    ok_flip = (np.abs(got - np.floor(flipped * shade)).max(-1) <= 1)[distinct].mean()
    print('cube top: %d pixels tell the readings apart; %.4f of them read the file v-up, %.4f flipped' % (distinct.sum(), ok_right,
                                                                                                     ok_flip))
    assert distinct.sum() > 1000 and ok_right == 1.0 and ok_flip < 0.01


NEG_SCENES = ('home', 'nearplane')


@pytest.mark.parametrize('variant', [v for v in nc.VARIANTS if v != 'ties_highest'])
def test_negative_controls_break_the_bounds(variant):
    """Each deliberately wrong restatement must break a bound against the oracle on one of two scenes: the bounds are tight
    enough to see a flipped texture row, affine interpolation, a normal left in the body frame, a sample row off by one, a
    near test on ray distance and a specular exponent of 1."""
    broken = []
    for name in NEG_SCENES:
        o, nobj, W, H, view, proj, rows = scene(name)
        r, d, m = o.render()
        h = nc.render(o.state, nobj, W, H, view, proj, variant=variant)
        broken += compare((r, d, m), h, None)
    print(variant, broken)
    assert broken, variant


def test_tie_rule_decides_no_pixel_of_this_model():
    """The tie rule (equal depth: lowest triangle id) is restated, but no two triangles of the model coincide on one frame:
    the highest-id variant changes no decided pixel.  (Should the model ever gain coincident triangles of different colour,
    this test fails and the tie rule gets a negative control of its own.)"""
    for name in NEG_SCENES:
        o, nobj, W, H, view, proj, rows = scene(name)
        a = nc.render(o.state, nobj, W, H, view, proj)
        b = nc.render(o.state, nobj, W, H, view, proj, variant='ties_highest')
        assert (a['rgb'][a['dec_rgb']] == b['rgb'][a['dec_rgb']]).all()
