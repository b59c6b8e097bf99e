"""A float64 numpy ray caster of the camera, for the tests (a helper module: pytest does not collect it).

Built from the compiled model's data (real_robots_amd.model.load_model) and the documented camera contract only -- it calls
nothing of the oracle (oracle/rr_oracle.c) or of the HIP kernels, and it takes another road than they do:

* frames: the body frames of numpy_step.forward and the object rotations of numpy_step.quat_to_mat; every render instance
  takes the owner of `inst_owner` (otype 0 static / 1 body / 2 object, oidx, uid, tex), the trailing object instances are
  skipped when n_objects < 3;
* cameras: the eye camera is a look-at from (0.01, 0, 1.2) to `table_pos`, up +z, with a GL perspective of vertical fov 80
  degrees, aspect W / H, near 0.1, far 100 (the reference's env.py:536-551); EnvCamera (render('rgb_array'), env.py:470-499)
  is Bullet's computeViewMatrixFromYawPitchRoll with upAxisIndex 2 (eye = Rz(yaw) Rx(pitch) (0, -d, 0) + target, up =
  Rz(yaw) Rx(pitch) +z).  The view matrix is the inverse of the camera-to-world frame and the projection the GL frustum
  (l, r, b, t, n, f), not the closed forms the product uses; arbitrary view / projection matrices can be passed in;
* one ray per sample point, ndc_x = 2 col / W - 1, ndc_y = 2 (H - 1 - row) / H - 1, from the eye through the unprojected
  point, intersected with every candidate triangle in WORLD space (Moller-Trumbore) -- no screen-space edge functions;
* near plane: a hit counts only where its view depth w (the clip-space w) is >= 0.1 -- no polygon clipping is needed for
  coverage; depth is the GL depth 0.5 z_ndc + 0.5 of the hit point, and the hit's barycentrics are the perspective-correct
  weights exactly;
* shading: the interpolated normal rotated into the world frame and normalised, shade = 0.6 + 0.35 max(n.l, 0) +
  0.05 max(r_z, 0)^2 with r = 2 (n.l) n - l and l = (-50, 30, 100) normalised; the nearest texel with wrap, u across the
  columns and v UP the rows: tools/compile_model.py stores tex_data in the image file's row order (top row first), so texel
  (tx, ty) = (floor(u tw), floor(v th)) is file row th - 1 - ty; times `inst_color`, floor, clamped to 255.  Background:
  white, depth 1, mask -1;
* visibility: the nearest hit wins, equal depths go to the lowest triangle id; the zero-area triangles (the padding of the
  raster clusters) are skipped.

Candidates: every triangle's projected bounding box (of its near-clipped outline, widened by EPS_PX and clamped to the image)
gives the (pixel, triangle) pairs, evaluated fully vectorised in chunks.  `rows=` restricts the work to a subset of image rows
(very large images are checked at tile boundaries and on random rows).

Ambiguity -- what tells a pixel the float32 rasterisers must agree on from one where they may legitimately differ:

* sd: the signed distance in pixels from the sample point to the projected, near-clipped outline of every candidate
  triangle (positive inside; for a point outside, the largest distance outside one edge line); sd_min is the smallest |sd|
  over the candidates whose plane is not more than DELTA behind the winner at that pixel (an outline hidden behind the
  winning surface decides nothing);
* gap: the depth gap between the winner and the nearest covering surface of ANOTHER uid, and tie_gap: the gap to the nearest
  covering surface of another triangle with a different colour (any uid).  (No two triangles of the model coincide on one
  frame, so an exact depth tie between surfaces of different colour never decides a pixel: the tie rule is restated, but
  a pixel it would decide is undecided for RGB by tie_gap.);
* texel distance: for textured hits, the distance of u tw and v th from an integer (only for texture axes wider than 1).

A pixel is DECIDED FOR THE MASK when every such candidate lies at least EPS_PX = 1e-3 px inside or outside its outline and any
covering surface within DELTA (depth) of the winner has the winner's uid.  It is DECIDED FOR RGB when it is decided for the
mask, no covering surface of another colour lies within DELTA of the winner, and its texel coordinates are at least
EPS_TEXEL = 1e-3 texel from a texel boundary.  DELTA is twice the depth bound of the comparison at the winner's view depth
(depth_bound below).

`variant=` selects a deliberately wrong restatement (negative controls of the tests): 'tex_row_unflipped',
'affine' (screen-space uv / normal interpolation), 'normal_local' (normal not rotated into the world), 'row_off_by_one'
(sample row H - row), 'near_on_distance' (near test on ray distance), 'spec_exp1', 'ties_highest'.
"""
import numpy as np

from real_robots_amd.model import load_model
from tests import numpy_step as ns

EYE = (0.01, 0.0, 1.2)
FOV, NEAR, FAR = 80.0, 0.1, 100.0
LIGHT = np.array([-50.0, 30.0, 100.0]) / np.linalg.norm([-50.0, 30.0, 100.0])
EPS_PX = 1e-3
EPS_TEXEL = 1e-3
CAND_PX = 1e-2      # a candidate whose outline passes within this distance of a sample point may cover it (cand bits)
VARIANTS = ('tex_row_unflipped', 'affine', 'normal_local', 'row_off_by_one', 'near_on_distance', 'spec_exp1', 'ties_highest')

_M = None


def model():
    """Render arrays of the model in float64 (triangles without the zero-area ones)."""
    global _M
    if _M is None:
        m = load_model()
        P = np.array(m['tri_pos'], np.float64)
        area = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
        keep = np.nonzero(area > 0)[0]
        _M = dict(tid=keep, pos=P[keep], nrm=np.array(m['tri_nrm'], np.float64)[keep],
                  uv=np.array(m['tri_uv'], np.float64)[keep], inst=np.array(m['tri_inst'], np.int64)[keep],
                  owner=np.array(m['inst_owner'], np.int64), color=np.array(m['inst_color'], np.float64),
                  tex_info=np.array(m['tex_info'], np.int64), tex_data=np.array(m['tex_data'][:, :3]),
                  table_pos=np.array(m['table_pos'], np.float64))
    return _M


# ------------------------------------------------------------------ cameras
def look_at(eye, target, up):
    """GL view matrix (row-major) as the inverse of the camera-to-world frame: camera x = right, y = up, z = backwards."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    back = eye - target
    back = back / np.linalg.norm(back)
    right = np.cross(up, back)
    right = right / np.linalg.norm(right)
    C = np.eye(4)
    C[:3, 0], C[:3, 1], C[:3, 2], C[:3, 3] = right, np.cross(back, right), back, eye
    return np.linalg.inv(C)


def perspective(fov_deg, aspect, near=NEAR, far=FAR):
    """glFrustum(l, r, b, t, n, f) of a symmetric frustum with vertical field of view fov_deg."""
    t = near * np.tan(np.radians(fov_deg) / 2)
    r, l, b = t * aspect, -t * aspect, -t
    return np.array([[2 * near / (r - l), 0, (r + l) / (r - l), 0], [0, 2 * near / (t - b), (t + b) / (t - b), 0],
                     [0, 0, -(far + near) / (far - near), -2 * far * near / (far - near)], [0, 0, -1, 0]])


def _rot(axis, ang):
    return ns._axis_angle(np.asarray(axis, np.float64), np.radians(ang))


def yaw_pitch_view(target, distance, yaw, pitch):
    """Bullet's computeViewMatrixFromYawPitchRoll(target, distance, yaw, pitch, roll=0, upAxisIndex=2): the eye offset
    (0, -distance, 0) and the up axis +z turned by Rz(yaw) Rx(pitch) (setEulerZYX(yaw, roll, pitch))."""
    R = _rot([0, 0, 1], yaw) @ _rot([1, 0, 0], pitch)
    target = np.asarray(target, np.float64)
    return look_at(R @ np.array([0.0, -distance, 0.0]) + target, target, R @ np.array([0.0, 0.0, 1.0]))


def eye_camera(W, H):
    return look_at(EYE, model()['table_pos'], [0, 0, 1]), perspective(FOV, W / H)


def env_camera():
    """EnvCamera of render('rgb_array'): distance 1.2, yaw 30, pitch -30 around [0, 0, 0.4], fov 80, 320 x 240."""
    return yaw_pitch_view([0, 0, 0.4], 1.2, 30, -30), perspective(FOV, 320 / 240)


def depth_bound(w):
    """Depth bound of a float32 rasteriser against this restatement at view depth w (see tests/test_numpy_camera.py):
    DEPTH_FAR from w = 0.3 m on; nearer, DEPTH_NEAR or what an error of DEPTH_W_ERR m in w makes of the GL depth
    (d(depth)/dw = n f / ((f - n) w^2) ~ 0.1 / w^2), whichever is larger."""
    w = np.asarray(w, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        near = np.maximum(DEPTH_NEAR, DEPTH_W_ERR * NEAR * FAR / ((FAR - NEAR) * w * w))
    return np.where(w >= 0.3, DEPTH_FAR, near)


DEPTH_FAR, DEPTH_NEAR, DEPTH_W_ERR = 8e-6, 2e-5, 1.5e-5      # tests/test_numpy_camera.py: measured worst cases


# ------------------------------------------------------------------ scene
def world_triangles(state, n_objects=3):
    """World-space triangles, instance rotations and model indices of the triangles drawn at `state` (61)."""
    M = model()
    s = np.asarray(state, np.float64)
    Rb, pb, _ = ns.forward(s[:11])
    ni = len(M['owner'])
    R, p = np.tile(np.eye(3), (ni, 1, 1)), np.zeros((ni, 3))
    used = np.ones(ni, bool)
    for i, (ot, oi, _, _) in enumerate(M['owner']):
        if ot == 1:
            R[i], p[i] = Rb[oi], pb[oi]
        elif ot == 2:
            if oi >= n_objects:
                used[i] = False
                continue
            o = s[22 + 13 * oi: 35 + 13 * oi]
            R[i], p[i] = ns.quat_to_mat(o[3:7]), o[:3]
    sel = np.nonzero(used[M['inst']])[0]
    inst = M['inst'][sel]
    Wp = np.einsum('tij,tkj->tki', R[inst], M['pos'][sel]) + p[inst][:, None, :]
    return sel, Wp, R


def _clip_outline(C):
    """Near-clipped outlines (clip space [T, 3, 4] -> screen polygons of up to 4 corners) as [T, 4, 4] (a triangle repeats
    its last corner) and a per-triangle `any` flag."""
    T = len(C)
    out = np.repeat(C[:, 2:3], 4, axis=1).copy()
    out[:, :3] = C
    inside = C[:, :, 3] >= NEAR
    n_in = inside.sum(1)
    ok = n_in > 0
    for t in np.nonzero(ok & (n_in < 3))[0]:
        poly = []
        for i in range(3):
            j = (i + 1) % 3
            a, b = C[t, i], C[t, j]
            if a[3] >= NEAR:
                poly.append(a)
            if (a[3] >= NEAR) != (b[3] >= NEAR):
                s = (NEAR - a[3]) / (b[3] - a[3])
                poly.append(a + s * (b - a))
        poly += [poly[-1]] * (4 - len(poly))
        out[t] = poly
    return out, ok


def render(state, n_objects=3, W=128, H=128, view=None, proj=None, rows=None, variant=None, chunk=1 << 18):
    """Ray-cast image of `state` (61 floats, the layout of rr_get_state).  Returns a dict of per-pixel arrays over the
    selected rows (rows: None = all, else an increasing list of image rows): rgb [R, W, 3] u8, depth [R, W], mask [R, W],
    tri (model triangle id, -1), w (view depth of the winner), sd_min (smallest |signed outline distance| over the
    candidates, px), gap (to the nearest covering surface of another uid), tie_gap (of another colour), texel (distance from
    a texel boundary), tex_rgb (the texel fetched), uv (wrapped to [0, 1)), cand (bit u set: a triangle of uid u lies within CAND_PX outside of the sample point or covers it),
    dec_mask, dec_rgb, `rows` and the image `size` (W, H)."""
    assert variant is None or variant in VARIANTS, variant
    M = model()
    if view is None:
        view, proj = eye_camera(W, H)
    view, proj = np.asarray(view, np.float64), np.asarray(proj, np.float64)
    VP = proj @ view
    iVP = np.linalg.inv(VP)
    eye = np.linalg.inv(view)[:3, 3]
    rows = np.arange(H) if rows is None else np.asarray(rows, np.int64)
    R_ = len(rows)
    # one ray per sample point
    sy = (H - rows if variant == 'row_off_by_one' else H - 1 - rows).astype(np.float64)
    nx = 2.0 * np.arange(W) / W - 1.0
    ny = 2.0 * sy / H - 1.0
    far = np.einsum('ij,rcj->rci', iVP, np.stack([np.broadcast_to(nx[None, :], (R_, W)), np.broadcast_to(ny[:, None], (R_, W)),
                                                   np.ones((R_, W)), np.ones((R_, W))], -1))
    D = (far[..., :3] / far[..., 3:4] - eye).reshape(-1, 3)
    # triangles
    sel, Pw, Rinst = world_triangles(state, n_objects)
    inst = M['inst'][sel]
    C = np.einsum('ij,tkj->tki', VP, np.concatenate([Pw, np.ones(Pw.shape[:2] + (1,))], -1))
    outline, ok = _clip_outline(C)
    outline[~ok] = [0.0, 0.0, 0.0, 1.0]
    S = np.empty(outline.shape[:2] + (2,))
    S[..., 0] = (outline[..., 0] / outline[..., 3] + 1) * W / 2
    S[..., 1] = (outline[..., 1] / outline[..., 3] + 1) * H / 2
    x0 = np.clip(np.ceil(S[..., 0].min(1) - EPS_PX), 0, W)
    x1 = np.clip(np.floor(S[..., 0].max(1) + EPS_PX), -1, W - 1)
    y0 = np.clip(np.ceil(S[..., 1].min(1) - EPS_PX), 0, H)
    y1 = np.clip(np.floor(S[..., 1].max(1) + EPS_PX), -1, H - 1)
    # the sample y of the selected rows, increasing: rank range of every triangle's [y0, y1]
    ys = np.sort(sy)
    order = np.argsort(sy, kind='stable')
    k0 = np.searchsorted(ys, y0, 'left')
    k1 = np.searchsorted(ys, y1, 'right')
    nxs = np.maximum(x1 - x0 + 1, 0).astype(np.int64)
    nys = np.maximum(k1 - k0, 0).astype(np.int64)
    npair = np.where(ok, nxs * nys, 0)
    # outline orientation and edges
    area = np.sum(S[:, [0, 1, 2, 3], 0] * S[:, [1, 2, 3, 0], 1] - S[:, [1, 2, 3, 0], 0] * S[:, [0, 1, 2, 3], 1], 1)
    E = np.roll(S, -1, axis=1) - S                                    # edge vectors [T, 4, 2]
    El = np.linalg.norm(E, axis=-1)
    # per-triangle data of the hit
    e1, e2 = Pw[:, 1] - Pw[:, 0], Pw[:, 2] - Pw[:, 0]
    tex = M['owner'][inst, 3]
    col = M['color'][inst]
    uid = M['owner'][inst, 2]
    tid = M['tid'][sel]
    NP = R_ * W
    best = np.full(NP, np.inf)
    best_t = np.full(NP, -1, np.int64)                               # index into sel
    best_c = np.zeros((NP, 3))
    sdmin = np.full(NP, np.inf)
    cand = np.zeros(NP, np.int64)
    edge = []
    hits = []                                                        # (pixel, depth, local tri) of every hit
    tris = np.nonzero(npair)[0]
    cs = np.cumsum(npair[tris])
    for tt in np.split(tris, np.searchsorted(cs, np.arange(chunk, cs[-1] if len(cs) else 0, chunk))):
        if not len(tt):
            continue
        cnt = npair[tt]
        t = np.repeat(tt, cnt)
        k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        col_ = (x0[t] + k % nxs[t]).astype(np.int64)
        r_ = order[(k0[t] + k // nxs[t]).astype(np.int64)]           # index into rows
        pix = r_ * W + col_
        px = np.stack([col_.astype(np.float64), sy[r_]], -1)
        # signed outline distance (pixels)
        rel = px[:, None, :] - S[t]
        cr = E[t, :, 0] * rel[..., 1] - E[t, :, 1] * rel[..., 0]
        with np.errstate(invalid='ignore', divide='ignore'):
            dist = np.where(El[t] > 0, np.sign(area[t])[:, None] * cr / np.where(El[t] > 0, El[t], 1), np.inf)
        sd = dist.min(1)
        close = sd >= -CAND_PX
        np.bitwise_or.at(cand, pix[close], 1 << uid[t[close]])
        # Moller-Trumbore
        d = D[pix]
        pv = np.cross(d, e2[t])
        det = np.einsum('ij,ij->i', e1[t], pv)
        with np.errstate(invalid='ignore', divide='ignore'):
            idet = 1.0 / det
            tv = eye - Pw[t, 0]
            u = np.einsum('ij,ij->i', tv, pv) * idet
            qv = np.cross(tv, e1[t])
            v = np.einsum('ij,ij->i', d, qv) * idet
            s = np.einsum('ij,ij->i', e2[t], qv) * idet
        X = eye + s[:, None] * d
        cw = X @ VP[3, :3] + VP[3, 3]
        cz = X @ VP[2, :3] + VP[2, 3]
        dep = 0.5 * cz / cw + 0.5
        if variant == 'near_on_distance':
            front = s * np.linalg.norm(d, axis=1) >= NEAR
        else:
            front = cw >= NEAR
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (s > 0) & front & (dep <= 1)     # (far plane)
        h = np.nonzero(hit)[0]
        hits.append((pix[h], dep[h], t[h], np.stack([1 - u[h] - v[h], u[h], v[h]], -1)))
        e = np.nonzero(np.abs(sd) < EPS_PX)[0]                       # outlines through a sample point: depth of their plane there
        edge.append((pix[e], np.abs(sd[e]), np.where((det[e] != 0) & (s[e] > 0) & np.isfinite(dep[e]), dep[e], -np.inf)))
    pix_h = np.concatenate([a[0] for a in hits]) if hits else np.zeros(0, np.int64)
    dep_h = np.concatenate([a[1] for a in hits]) if hits else np.zeros(0)
    tri_h = np.concatenate([a[2] for a in hits]) if hits else np.zeros(0, np.int64)
    bc_h = np.concatenate([a[3] for a in hits]) if hits else np.zeros((0, 3))
    # visibility: nearest, then lowest (or highest) triangle id
    key2 = -tid[tri_h] if variant == 'ties_highest' else tid[tri_h]
    o = np.lexsort((key2, dep_h, pix_h))
    first = np.ones(len(o), bool)
    first[1:] = pix_h[o][1:] != pix_h[o][:-1]
    win = o[first]
    wp = pix_h[win]
    best[wp] = dep_h[win]
    best_t[wp] = tri_h[win]
    best_c[wp] = bc_h[win]
    # gaps to other covering surfaces (another uid / another colour)
    gap = np.full(NP, np.inf)
    tie_gap = np.full(NP, np.inf)
    wt = best_t[pix_h]
    other_uid = uid[tri_h] != uid[wt]
    g = dep_h - best[pix_h]
    np.minimum.at(gap, pix_h[other_uid], np.abs(g[other_uid]))
    # shading of every hit (to tell surfaces of another colour) -- only hits within reach of the winner need it
    near_h = np.nonzero((tri_h != wt) & (np.abs(g) < 1e-3))[0]
    ex = {}
    rgbf_win, texd_win, w_win = _shade(M, sel, Pw, Rinst, inst, tex, col, best_t[wp], best_c[wp], VP, variant, ex)
    tex_rgb = np.full((NP, 3), 255.0)
    tex_rgb[wp] = ex['tex_rgb']
    uvw = np.full((NP, 2), np.nan)
    uvw[wp] = ex['uv']
    if len(near_h):
        rgbf_o, _, _ = _shade(M, sel, Pw, Rinst, inst, tex, col, tri_h[near_h], bc_h[near_h], VP, variant)
        full = np.zeros((NP, 3))
        full[wp] = rgbf_win
        diff = np.abs(np.floor(rgbf_o) - np.floor(full[pix_h[near_h]])).max(1) > 0
        np.minimum.at(tie_gap, pix_h[near_h][diff], np.abs(g[near_h][diff]))
    rgb = np.full((NP, 3), 255, np.uint8)
    rgb[wp] = np.minimum(np.floor(rgbf_win), 255).astype(np.uint8)
    depth = np.ones(NP)
    depth[wp] = best[wp]
    mask = np.full(NP, -1, np.int64)
    mask[wp] = uid[best_t[wp]]
    tri = np.full(NP, -1, np.int64)
    tri[wp] = tid[best_t[wp]]
    w = np.full(NP, np.inf)
    w[wp] = w_win
    texel = np.full(NP, np.inf)
    texel[wp] = texd_win
    delta = 2 * depth_bound(w)
    # an outline through the sample point matters where its plane is not clearly behind the winner
    for ep, es, ed in edge:
        front = ed <= depth[ep] + delta[ep]
        np.minimum.at(sdmin, ep[front], es[front])
    dec_mask = (sdmin >= EPS_PX) & (gap >= delta)
    dec_rgb = dec_mask & (tie_gap >= delta) & (texel >= EPS_TEXEL)
    sh = (R_, W)
    return dict(rgb=rgb.reshape(sh + (3,)), depth=depth.reshape(sh), mask=mask.reshape(sh), tri=tri.reshape(sh),
                w=w.reshape(sh), sd_min=sdmin.reshape(sh), gap=gap.reshape(sh), tie_gap=tie_gap.reshape(sh),
                texel=texel.reshape(sh), tex_rgb=tex_rgb.reshape(sh + (3,)), uv=uvw.reshape(sh + (2,)), cand=cand.reshape(sh), dec_mask=dec_mask.reshape(sh), dec_rgb=dec_rgb.reshape(sh), rows=rows, size=(W, H))


def _shade(M, sel, Pw, Rinst, inst, tex, col, t, c, VP, variant, extra=None):
    """Colour (float, before floor), texel-boundary distance and view depth of hits (local triangle t, weights c)."""
    w3 = np.einsum('j,tkj->tk', VP[3, :3], Pw[t]) + VP[3, 3]            # view depth of the corners
    w = np.einsum('tk,tk->t', c, w3)                                    # (an affine function of the hit point)
    if variant == 'affine':                                             # screen-space weights: c_i w_i normalised
        c = c * w3
        c = c / c.sum(1, keepdims=True)
    j = sel[t]
    nl = np.einsum('tk,tki->ti', c, M['nrm'][j])
    nw = nl if variant == 'normal_local' else np.einsum('tij,tj->ti', Rinst[inst[t]], nl)
    nw = nw / np.linalg.norm(nw, axis=1, keepdims=True)
    ndl = nw @ LIGHT
    r = 2 * ndl[:, None] * nw - LIGHT
    rz = np.maximum(r[:, 2] / np.linalg.norm(r, axis=1), 0)
    spec = rz if variant == 'spec_exp1' else rz * rz
    shade = 0.6 + 0.35 * np.maximum(ndl, 0) + 0.05 * spec
    texel = np.full(len(t), np.inf)
    tx_rgb = np.full((len(t), 3), 255.0)
    tt = tex[t]
    m = np.nonzero(tt >= 0)[0]
    if len(m):
        uv = np.einsum('tk,tki->ti', c[m], M['uv'][j[m]])
        uv = uv - np.floor(uv)
        off, tw, th = (M['tex_info'][tt[m], i] for i in range(3))
        fu, fv = uv[:, 0] * tw, uv[:, 1] * th
        du = np.where(tw > 1, np.abs(fu - np.round(fu)), np.inf)
        dv = np.where(th > 1, np.abs(fv - np.round(fv)), np.inf)
        texel[m] = np.minimum(du, dv)
        tx = np.minimum(np.floor(fu).astype(np.int64), tw - 1)
        ty = np.minimum(np.floor(fv).astype(np.int64), th - 1)
        file_row = ty if variant == 'tex_row_unflipped' else th - 1 - ty
        tx_rgb[m] = M['tex_data'][off + file_row * tw + tx]
    out = tx_rgb * col[t] * shade[:, None]
    if extra is not None:
        extra['tex_rgb'], extra['uv'] = tx_rgb, np.full((len(t), 2), np.nan)
        if len(m):
            extra['uv'][m] = uv
    return out, texel, w
