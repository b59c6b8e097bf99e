// rr_render.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// rasteriser: k_raster, k_shade, the list-walking render kernels
// ---------------------------------------------------------------------------------------------- rasteriser
// One workgroup per (env, tile). Tile = full-width strip of tile_h rows (<= TILE_PIX pixels, 8 bytes of LDS key each).
#ifndef RASTER_THREADS
#define RASTER_THREADS 512       // with TILE_PIX 4096: 39.5 KB of LDS -> four workgroups = eight waves per SIMD (A/B below)
#endif
#define VIS_WAS_DYNAMIC (~0ull - 1)   // visibility key of a pixel that was dynamic in the previous frame and is not (yet) now
#define FRAG_VACATED 0x3ffffu         // triangle field of a fragment-list entry for such a pixel: back to the static layer
// A/B at 4096 envs, 128x128 (k_raster ms): 16384 px x 1024 threads (one workgroup per CU) 0.564; 8192 x 512 (two) 0.521;
// 4096 x 512 (three) 0.449; 4096 x 256 0.629; 2048 x 256 0.546.  At 320x240: 0.460 / 0.432 / 0.442.
#ifndef TILE_PIX
#define TILE_PIX 4096
#endif
// LDS of a raster workgroup: 32 KB of keys + 1 KB window list + 1 KB running ends + 1.5 KB matrices + 4 KB clip queue = 39.5 KB:
// four workgroups per CU = eight waves per SIMD, which also needs <= 64 VGPRs (A/B: three workgroups 0.434 ms, four 0.390 ms)
#ifndef MAXWIN
#define MAXWIN 512       // 64-triangle windows per model (rr_create checks nt)
#endif
#define RASTER_INST 24   // instances whose matrices a raster workgroup stages (rr_create checks the model)
#define RASTER_ATTR __attribute__((amdgpu_waves_per_eu(8, 8)))

static_assert(RASTER_INST <= MAXINST && MAXWIN <= 512, "clip queue entries: window position (9 bits) << 6 | lane");
#ifndef CLIPQ
#define CLIPQ 2048       // triangles crossing the near plane per (env, tile) that are clipped (a link cut by the plane has a few hundred;
#endif                   // an overflow raises error flag 4 of the env instead of dropping triangles silently)
#ifndef INLINE_PIX
#define INLINE_PIX 2     // sample points of a small triangle walked by its own lane; the rest is redistributed over the wave
#endif
#define SMALL_AREA 64    // bbox area (sample points) up to which a triangle takes the per-lane + redistribution path (A/B: 16 0.60, 32 0.54, 64 0.53, 128 0.54 ms)
static_assert(SMALL_AREA <= 64, "a raster record's box width has 6 bits");

struct STri { float sx[3], sy[3], sz[3], w[3]; };

// Coverage decisions are discontinuous: projection, barycentrics and depth must round exactly like the oracle's --
// geometry a few cm from the near plane projects to huge screen coordinates where one rounding flips whole pixel bands.
// So nothing here is left to the compiler's contraction: the fused operations are written out (a C fmaf in the oracle and
// v_fma_f32 round identically), everything else is compiled contraction-free.
#define FMA3(a0, x0, a1, x1, a2, x2, c) __builtin_fmaf((a0), (x0), __builtin_fmaf((a1), (x1), __builtin_fmaf((a2), (x2), (c))))   // a0 x0 + (a1 x1 + (a2 x2 + c))
#define PDIFF(a, b, c, d) __builtin_fmaf((a), (b), -((c) * (d)))                                                                  // a b - c d: one product, one fused step
// Correctly rounded 1 / x for a normal x whose reciprocal is normal too (|x| within 2^-96 .. 2^96: clip w >= 0.1, signed areas
// 1e-12 .. 1e12): the compiler's IEEE division expands to v_div_scale x 2, v_rcp, a Newton step, two residual corrections,
// v_div_fmas, v_div_fixup -- eleven instructions; inside that range the scaling and the fix-up are the identity and what remains is
// this sequence, operation for operation (so the bits are those of `1.0f / x` and of the oracle's division): eight instructions.
__device__ __forceinline__ float recip_exact(float x) {
    const float r0 = __builtin_amdgcn_rcpf(x);
    const float e0 = __builtin_fmaf(-x, r0, 1.0f);
    const float r1 = __builtin_fmaf(e0, r0, r0);
    const float q0 = r1;                                   // numerator 1
    const float e1 = __builtin_fmaf(-x, q0, 1.0f);
    const float q1 = __builtin_fmaf(e1, r1, q0);
    const float e2 = __builtin_fmaf(-x, q1, 1.0f);
    return __builtin_fmaf(e2, r1, q1);
}
__device__ __forceinline__ bool project_tri(const float *mvp, const float *tp /*9 floats*/, int W, int H, STri &s) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float vx = tp[3 * k], vy = tp[3 * k + 1], vz = tp[3 * k + 2];
        float cx = FMA3(mvp[0], vx, mvp[1], vy, mvp[2], vz, mvp[3]);
        float cy = FMA3(mvp[4], vx, mvp[5], vy, mvp[6], vz, mvp[7]);
        float cz = FMA3(mvp[8], vx, mvp[9], vy, mvp[10], vz, mvp[11]);
        float cw = FMA3(mvp[12], vx, mvp[13], vy, mvp[14], vz, mvp[15]);
        if (cw < 0.1f) return false;
        float iw = recip_exact(cw);
        s.sx[k] = __builtin_fmaf(cx * iw, 0.5f * (float)W, 0.5f * (float)W);
        s.sy[k] = __builtin_fmaf(cy * iw, 0.5f * (float)H, 0.5f * (float)H);
        s.sz[k] = cz * iw;
        s.w[k] = iw;             // reciprocal clip w (deferred shading)
    }
    return true;
}

// One vertex of project_tri (identical arithmetic); a vertex nearer than the near plane yields sx = NaN.
__device__ __forceinline__ void project_vertex(const float *mvp, float vx, float vy, float vz, int W, int H, float &sx, float &sy, float &sz) {
#pragma clang fp contract(off)
    const float cx = FMA3(mvp[0], vx, mvp[1], vy, mvp[2], vz, mvp[3]);
    const float cy = FMA3(mvp[4], vx, mvp[5], vy, mvp[6], vz, mvp[7]);
    const float cz = FMA3(mvp[8], vx, mvp[9], vy, mvp[10], vz, mvp[11]);
    const float cw = FMA3(mvp[12], vx, mvp[13], vy, mvp[14], vz, mvp[15]);
    const float iw = recip_exact(cw);                         // (a vertex behind the near plane is flagged below; its values are never used)
    sx = (cw < 0.1f) ? __int_as_float(0x7fc00000) : __builtin_fmaf(cx * iw, 0.5f * (float)W, 0.5f * (float)W);
    sy = __builtin_fmaf(cy * iw, 0.5f * (float)H, 0.5f * (float)H);
    sz = cz * iw;
}
// Near-plane clipping (oracle clip_near / to_screen, identical arithmetic): clip coordinates of one vertex, the screen
// position of a clip-space point, and the intersection of an edge with w = NEAR_W computed from the inside end a towards
// the outside end b.
#define NEAR_W 0.1f
__device__ __forceinline__ void clip_vertex(const float *mvp, float vx, float vy, float vz, float *c) {
#pragma clang fp contract(off)
    c[0] = FMA3(mvp[0], vx, mvp[1], vy, mvp[2], vz, mvp[3]);
    c[1] = FMA3(mvp[4], vx, mvp[5], vy, mvp[6], vz, mvp[7]);
    c[2] = FMA3(mvp[8], vx, mvp[9], vy, mvp[10], vz, mvp[11]);
    c[3] = FMA3(mvp[12], vx, mvp[13], vy, mvp[14], vz, mvp[15]);
}
__device__ __forceinline__ void clip_to_screen(const float *c, int W, int H, float &sx, float &sy, float &sz) {
#pragma clang fp contract(off)
    const float iw = 1.0f / c[3];
    sx = __builtin_fmaf(c[0] * iw, 0.5f * (float)W, 0.5f * (float)W);
    sy = __builtin_fmaf(c[1] * iw, 0.5f * (float)H, 0.5f * (float)H);
    sz = c[2] * iw;
}
__device__ __forceinline__ void clip_edge(const float *a, const float *b, float *o) {
#pragma clang fp contract(off)
    const float t = (NEAR_W - a[3]) / (b[3] - a[3]);
    o[0] = __builtin_fmaf(t, b[0] - a[0], a[0]);
    o[1] = __builtin_fmaf(t, b[1] - a[1], a[1]);
    o[2] = __builtin_fmaf(t, b[2] - a[2], a[2]);
    o[3] = NEAR_W;
}

__device__ __forceinline__ bool bary(const STri &s, float px, float py, float *b) {
#pragma clang fp contract(off)
    float x0 = s.sx[0], y0 = s.sy[0], x1 = s.sx[1], y1 = s.sy[1], x2 = s.sx[2], y2 = s.sy[2];
    float area = PDIFF(x1 - x0, y2 - y0, x2 - x0, y1 - y0);
    if (fabsf(area) < 1e-12f) return false;
    float ia = recip_exact(area);
    b[0] = PDIFF(x1 - px, y2 - py, x2 - px, y1 - py) * ia;
    b[1] = PDIFF(x2 - px, y0 - py, x0 - px, y2 - py) * ia;
    b[2] = 1.0f - b[0] - b[1];
    return b[0] >= 0 && b[1] >= 0 && b[2] >= 0;
}

__device__ __forceinline__ void raster_pixel(const STri &s, int t, int px, int py, int H, int W, int row0, int rows,
                                             unsigned long long *vis) {
#pragma clang fp contract(off)
    int row = H - 1 - py;
    if (row < row0 || row >= row0 + rows) return;
    float b[3];
    if (!bary(s, (float)px, (float)py, b)) return;
    float z = __builtin_fmaf(b[0], s.sz[0], __builtin_fmaf(b[1], s.sz[1], b[2] * s.sz[2]));
    float d = __builtin_fmaf(0.5f, z, 0.5f);
    if (!(d >= 0.0f && d <= 1.0f)) return;
    unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)t;
    atomicMin(&vis[(row - row0) * W + px], key);
}

// Same arithmetic as bary()/raster_pixel() with the per-triangle part (signed area, its reciprocal) hoisted out of the
// pixel loop; (px, py) must already lie inside the tile.
struct TriEdge { float ia; bool ok; };
__device__ __forceinline__ TriEdge tri_edge(const STri &s) {
#pragma clang fp contract(off)
    float area = PDIFF(s.sx[1] - s.sx[0], s.sy[2] - s.sy[0], s.sx[2] - s.sx[0], s.sy[1] - s.sy[0]);
    TriEdge e;
    e.ok = !(fabsf(area) < 1e-12f);
    e.ia = recip_exact(area);                               // (|area| >= 1e-12 when ok; a degenerate triangle is not drawn and its value never used)
    return e;
}
__device__ __forceinline__ void raster_pixel_hoisted(const STri &s, float ia, int t, int px, int py, int H, int W /* row stride of the tile's buffer */, int row0,
                                                     unsigned long long *vis, int xoff = 0 /* first column of the tile */) {
#pragma clang fp contract(off)
    const float fx = (float)px, fy = (float)py;
    const float b0 = PDIFF(s.sx[1] - fx, s.sy[2] - fy, s.sx[2] - fx, s.sy[1] - fy) * ia;
    const float b1 = PDIFF(s.sx[2] - fx, s.sy[0] - fy, s.sx[0] - fx, s.sy[2] - fy) * ia;
    const float b2 = 1.0f - b0 - b1;
    if (!(b0 >= 0 && b1 >= 0 && b2 >= 0)) return;
    const float z = __builtin_fmaf(b0, s.sz[0], __builtin_fmaf(b1, s.sz[1], b2 * s.sz[2]));
    const float d = __builtin_fmaf(0.5f, z, 0.5f);
    if (!(d >= 0.0f && d <= 1.0f)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)t;
    atomicMin(&vis[(H - 1 - py - row0) * W + px - xoff], key);
}

// The same for a sample point given as floats (integer valued: exact) with its index in the tile's visibility buffer already known.
__device__ __forceinline__ void raster_pixel_at(const STri &s, float ia, int t, float fx, float fy, int vidx, unsigned long long *vis) {
#pragma clang fp contract(off)
    const float b0 = PDIFF(s.sx[1] - fx, s.sy[2] - fy, s.sx[2] - fx, s.sy[1] - fy) * ia;
    const float b1 = PDIFF(s.sx[2] - fx, s.sy[0] - fy, s.sx[0] - fx, s.sy[2] - fy) * ia;
    const float b2 = 1.0f - b0 - b1;
    if (!(b0 >= 0 && b1 >= 0 && b2 >= 0)) return;
    const float z = __builtin_fmaf(b0, s.sz[0], __builtin_fmaf(b1, s.sz[1], b2 * s.sz[2]));
    const float d = __builtin_fmaf(0.5f, z, 0.5f);
    if (!(d >= 0.0f && d <= 1.0f)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)t;
    atomicMin(&vis[vidx], key);
}

// Conservative test "can any sample point of the pixel rectangle [px0,px1]x[py0,py1] pass raster_pixel_hoisted's
// inside test?".  Exact barycentrics are affine in (px, py), so their maximum over the rectangle is at a corner; the
// float evaluation of raster_pixel_hoisted differs from the exact value by at most delta (see the caller), hence a
// rectangle whose four corner values of some barycentric are all < -2*delta cannot contain a covered sample point.
__device__ __forceinline__ bool block_may_overlap(const STri &s, float ia, int px0, int px1, int py0, int py1, float delta2) {
#pragma clang fp contract(off)
    float m0 = -3.0e38f, m1 = -3.0e38f, m2 = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float fx = (float)((c & 1) ? px1 : px0), fy = (float)((c & 2) ? py1 : py0);
        const float b0 = PDIFF(s.sx[1] - fx, s.sy[2] - fy, s.sx[2] - fx, s.sy[1] - fy) * ia;
        const float b1 = PDIFF(s.sx[2] - fx, s.sy[0] - fy, s.sx[0] - fx, s.sy[2] - fy) * ia;
        const float b2 = 1.0f - b0 - b1;
        m0 = fmaxf(m0, b0); m1 = fmaxf(m1, b1); m2 = fmaxf(m2, b2);
    }
    return !(m0 < -delta2 || m1 < -delta2 || m2 < -delta2);
}

// Deferred shading of one pixel from its visibility key (depth bits | triangle id): re-projects the winning triangle,
// perspective-correct barycentrics, interpolated normal -> Phong-like TinyRenderer shading, nearest texel.
// mvp / sinst: per-instance constants of this env staged in LDS by stage_instances(); sinst holds 16 floats per instance
// {R[9], colour[3], tex_off, tex_w (0: untextured; -1: one texel, in place of the offset), tex_h, uid}, which keeps the chain of dependent global loads of a
// shaded pixel at two (triangle record, texel).
// L0..L2: the unit light direction of the (env, tile) item being shaded (shade_light): uniform in the wave.
struct ShadeCtx { const DevPtrs *D; const float *mvp; const float *sinst; int W, H; float L0, L1, L2; };
// The light of an env: the handle-wide default l = (-50, 30, 100) normalised, or -- per-env appearance -- the env's own unit
// vector, one 12-byte read through the scalar cache (env is uniform in the workgroup, as for the camera record in raster_tile).
// The host's default_light() does the default's arithmetic in the same float32 operations: same bits.
__device__ __forceinline__ void shade_light(const DevPtrs &D, int env, ShadeCtx &c) {
    const float Lx = -50.0f, Ly = 30.0f, Lz = 100.0f;
    const float linv = 1.0f / sqrtf(Lx * Lx + Ly * Ly + Lz * Lz);
    c.L0 = Lx * linv; c.L1 = Ly * linv; c.L2 = Lz * linv;
    if (D.env_light) {
        const float *l = D.env_light + (size_t)__builtin_amdgcn_readfirstlane(env) * 4;
        c.L0 = l[0]; c.L1 = l[1]; c.L2 = l[2];
    }
}
// one 128-byte record per triangle {pos[9], nrm[9], inst, -, uv[6]}: 16-byte loads from a single cache line instead of 26
// scattered dwords.  Every lane shades a different triangle, and what such a load costs is vector-memory issue, not cache misses
// (round 5 probes: the same loads from ONE record through the scalar cache take 25 of the kernel's 89 us off, from 64 L1-resident
// records nothing; at half the occupancy the kernel takes a third longer): positions, normals and the instance are five loads; the texture coordinates are
// two more, fetched only by the lanes whose instance has a real texture (a 1 x 1 "texture" -- the arm's colours -- is one texel,
// which travels with the instance constants: no texel fetch either).
struct TriRec { float4 v[5]; const float4 *uv; };
__device__ __forceinline__ TriRec load_tri_rec(const DevPtrs &D, int t) {
    TriRec r;
    const float4 *rp = D.tri_rec + (size_t)8 * t;
#pragma unroll
    for (int k = 0; k < 5; k++) r.v[k] = rp[k];
    r.uv = rp + 5;
    return r;
}
__device__ __forceinline__ void shade_pixel(const ShadeCtx &c, const TriRec &tr, int px, int row, unsigned char *rgb3, int &mask) {
    const DevPtrs &D = *c.D;
    const int W = c.W, H = c.H;
    const float L0 = c.L0, L1 = c.L1, L2 = c.L2;
    float rec[20];
#pragma unroll
    for (int k = 0; k < 5; k++) { rec[4 * k] = tr.v[k].x; rec[4 * k + 1] = tr.v[k].y; rec[4 * k + 2] = tr.v[k].z; rec[4 * k + 3] = tr.v[k].w; }
    const float *tp = rec, *nn = rec + 9;
    const int inst = __float_as_int(rec[18]);
    STri s;
    float c0, c1, c2;
    if (project_tri(c.mvp + inst * 16, tp, W, H, s)) {
        float b[3] = {0, 0, 0};
        bary(s, (float)px, (float)(H - 1 - row), b);
        // perspective-correct weights b_k / w_k: s.w holds 1 / w_k (the reciprocal the projection computed anyway)
        c0 = b[0] * s.w[0]; c1 = b[1] * s.w[1]; c2 = b[2] * s.w[2];
    } else {
        // a corner is nearer than the near plane (the triangle was clipped by k_raster): perspective-correct weights straight
        // from the clip coordinates, c ~ u x v with u_i = x_i - xn w_i, v_i = y_i - yn w_i (oracle rro_render, same arithmetic)
#pragma clang fp contract(off)
        float k0[4], k1[4], k2[4];
        clip_vertex(c.mvp + inst * 16, tp[0], tp[1], tp[2], k0);
        clip_vertex(c.mvp + inst * 16, tp[3], tp[4], tp[5], k1);
        clip_vertex(c.mvp + inst * 16, tp[6], tp[7], tp[8], k2);
        const float xn = (float)px * (2.0f / (float)W) - 1.0f, yn = (float)(H - 1 - row) * (2.0f / (float)H) - 1.0f;
        const float u0 = k0[0] - xn * k0[3], u1 = k1[0] - xn * k1[3], u2 = k2[0] - xn * k2[3];
        const float v0 = k0[1] - yn * k0[3], v1 = k1[1] - yn * k1[3], v2 = k2[1] - yn * k2[3];
        c0 = u1 * v2 - u2 * v1; c1 = u2 * v0 - u0 * v2; c2 = u0 * v1 - u1 * v0;
    }
    float cs = recip_exact(c0 + c1 + c2);              // (sum of the perspective weights: of the order of 1 / w, far inside the range)
    c0 *= cs; c1 *= cs; c2 *= cs;
    float n0 = c0 * nn[0] + c1 * nn[3] + c2 * nn[6], n1 = c0 * nn[1] + c1 * nn[4] + c2 * nn[7], n2 = c0 * nn[2] + c1 * nn[5] + c2 * nn[8];
    const float *xf = c.sinst + inst * 16;
    float w0 = xf[0] * n0 + xf[1] * n1 + xf[2] * n2, w1 = xf[3] * n0 + xf[4] * n1 + xf[5] * n2, w2 = xf[6] * n0 + xf[7] * n1 + xf[8] * n2;
    float nlen = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
    if (nlen > 0) { const float inl = recip_exact(nlen); w0 *= inl; w1 *= inl; w2 *= inl; }      // (a rotated unit normal: length ~1)
    float ndl = w0 * L0 + w1 * L1 + w2 * L2;
    float diff = fmaxf(ndl, 0.0f);
    float r0 = w0 * (2 * ndl) - L0, r1 = w1 * (2 * ndl) - L1, r2 = w2 * (2 * ndl) - L2;
    float rl = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
    float rz = rl > 0 ? fmaxf(r2 / rl, 0.0f) : 0.0f;
    float spec = rz * rz;
    float tex0 = 255.0f, tex1 = 255.0f, tex2 = 255.0f;
    const int tw = __float_as_int(xf[13]);
    if (tw != 0) {
        unsigned px4 = (unsigned)__float_as_int(xf[12]);             // (tw < 0: a one-texel texture, the texel itself -- rr_create)
        if (tw > 0) {
            const int th = __float_as_int(xf[14]);
            const float4 ua = tr.uv[0], ub = tr.uv[1];
            float u = c0 * ua.x + c1 * ua.z + c2 * ub.x, v = c0 * ua.y + c1 * ua.w + c2 * ub.y;
            u = u - floorf(u); v = v - floorf(v);
            int tx = min((int)(u * (float)tw), tw - 1), ty = min((int)(v * (float)th), th - 1);
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 2)
            px4 = D.tex[(size_t)__float_as_int(xf[12]) + (size_t)((tx + ty) & 63)];      // (probe: texels of one cache-line set)
#else
            px4 = D.tex[(size_t)__float_as_int(xf[12]) + (size_t)(th - 1 - ty) * tw + tx];
#endif
        }
        tex0 = (float)(px4 & 255); tex1 = (float)((px4 >> 8) & 255); tex2 = (float)((px4 >> 16) & 255);
    }
    float shade = 0.6f + 0.35f * diff + 0.05f * spec;
    rgb3[0] = (unsigned char)min((int)(tex0 * xf[9] * shade), 255);
    rgb3[1] = (unsigned char)min((int)(tex1 * xf[10] * shade), 255);
    rgb3[2] = (unsigned char)min((int)(tex2 * xf[11] * shade), 255);
    mask = __float_as_int(xf[15]);
}

// Stages the per-instance constants of one env (computed by k_render_setup) in LDS: mvp and, when sinst != nullptr, the
// shading constants. A plain copy, 16 bytes per thread. Caller synchronises.
__device__ __forceinline__ void stage_instances(const RenderModel &RM, const DevPtrs &D, int env, int tid, int nthreads,
                                                float (*mvp)[16], float (*sinst)[16]) {
    const float4 *src = (const float4 *)(D.inst_xf + (size_t)env * MAXINST * 32);
    for (int i = tid; i < RM.ni * 8; i += nthreads) {
        const int inst = i >> 3, q = i & 7;
        if (q < 4) *(float4 *)&mvp[inst][4 * q] = src[i];
        else if (sinst) *(float4 *)&sinst[inst][4 * (q - 4)] = src[i];
    }
}

#ifdef RR_RASTER_STATS
// Development-only work counters (librealrobot_hip_stats.so, `make stats`; never part of the shipped library).
__device__ unsigned long long g_rstats[16];
#define RSTAT(i, v) do { if (P.ablate & 0x8000) atomicAdd(&g_rstats[i], (unsigned long long)(v)); } while (0)   /* RR_ABLATE=32768 */
extern "C" int rr_debug_raster_stats(unsigned long long *out16, int reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_rstats), sizeof(g_rstats)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_rstats), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
// phase clock of the window loop (RR_ABLATE=4096; scratch/rphase.py): wave cycles between phase marks; every workgroup sums its
// waves in LDS and writes its ten totals to a slot of its own (global atomics from every wave would be what the clock measures)
__device__ unsigned g_rphase_wg[65536][10];
#define PH_DECL unsigned long long ph_t_ = __builtin_readcyclecounter(); unsigned pa0_ = 0, pa1_ = 0, pa2_ = 0, pa3_ = 0, pa4_ = 0, pa5_ = 0, pa6_ = 0, pa7_ = 0, pa8_ = 0, pa9_ = 0; \
    __shared__ unsigned ph_lds_[10]; if (tid < 10) ph_lds_[tid] = 0;
#define PH(i) do { if (P.ablate & 0x1000) { const unsigned long long n_ = __builtin_readcyclecounter(); pa##i##_ += (unsigned)(n_ - ph_t_); ph_t_ = n_; } } while (0)
#define PH_FLUSH do { if (P.ablate & 0x1000) { if (lane == 0) { atomicAdd(&ph_lds_[0], pa0_); atomicAdd(&ph_lds_[1], pa1_); atomicAdd(&ph_lds_[2], pa2_); atomicAdd(&ph_lds_[3], pa3_); atomicAdd(&ph_lds_[4], pa4_); \
    atomicAdd(&ph_lds_[5], pa5_); atomicAdd(&ph_lds_[6], pa6_); atomicAdd(&ph_lds_[7], pa7_); atomicAdd(&ph_lds_[8], pa8_); atomicAdd(&ph_lds_[9], pa9_); } __syncthreads(); \
    if (tid < 10) g_rphase_wg[(env * RM.ntiles + tile) & 65535][tid] = ph_lds_[tid]; } } while (0)
extern "C" int rr_debug_raster_phase(unsigned long long *out16, int reset) {
    static unsigned h[65536][10];
    if (out16) {
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_rphase_wg), sizeof(h)) != hipSuccess) return -1;
        for (int i = 0; i < 16; i++) out16[i] = 0;
        for (int w = 0; w < 65536; w++) for (int i = 0; i < 10; i++) out16[i] += h[w][i];
    }
    if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_rphase_wg), h, sizeof(h)) != hipSuccess) return -1; }
    return 0;
}
// workgroup timeline of k_raster (RR_ABLATE=16384; scratch/rwgtime.py): start / end on the 100 MHz clock and the hardware slot
// (HW_ID, XCC_ID) of every workgroup of the last launch -- how full the four workgroup slots of a CU are kept
__device__ unsigned long long g_rwg_time[65536][3];
__device__ int g_shade_ablate;      // (k_shade has no SimParams: rr_debug_shade_ablate sets what it records)
extern "C" int rr_debug_shade_ablate(int v) { return hipMemcpyToSymbol(HIP_SYMBOL(g_shade_ablate), &v, sizeof(v)) == hipSuccess ? 0 : -1; }
extern "C" int rr_debug_raster_wgtime(unsigned long long *out /*[65536][3]*/, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rwg_time), sizeof(g_rwg_time)) != hipSuccess) return -1;
    if (reset) { static unsigned long long z[65536][3]; if (hipMemcpyToSymbol(HIP_SYMBOL(g_rwg_time), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
// ... and marks inside a workgroup (thread 0, 100 MHz clock): 0 kernel entry, 1 selection flags there, 2 LDS filled + instances staged,
// 3 clusters culled, 4 window loop done, 5 near-plane pass done, 6 list written
__device__ unsigned long long g_rwg_marks[65536][8];
#define WGM(i) do { if ((P.ablate & 0x4000) && threadIdx.x == 0) g_rwg_marks[(env * RM.ntiles + tile) & 65535][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int rr_debug_raster_wgmarks(unsigned long long *out /*[65536][8]*/) {
    return (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rwg_marks), sizeof(g_rwg_marks)) == hipSuccess) ? 0 : -1;
}
// phase ablations of k_raster for the time breakdown in DESIGN.md (RR_ABLATE bits: 1 no rasterisation after projection,
// 2 no wave-cooperative path, 8 no triangles at all); compiled out of the shipped library
#define ABL(bit) (P.ablate & (bit))
#else
#define RSTAT(i, v)
#define WGM(i)
#define ABL(bit) false
#define PH_DECL
#define PH(i)
#define PH_FLUSH
#endif

// The cluster cull of raster_tile: clip-space centre of the cluster's bounding sphere against the five
// frustum planes, then against the planes of a tile's first / last sample row and column (RM.tile_plane), radius enlarged -- conservative.
// pn / tp: the camera's plane_norm and the tile's row of tile_plane (RenderModel's, or the env's record with per-env cameras).
struct ClusterClip { float cx, cy, cw, r; };
__device__ __forceinline__ bool cluster_outside_frustum(const float *pn /*RM.plane_norm*/, const float *m, const float4 cs, ClusterClip &c) {
    c.cx = m[0] * cs.x + m[1] * cs.y + m[2] * cs.z + m[3]; c.cy = m[4] * cs.x + m[5] * cs.y + m[6] * cs.z + m[7];
    c.cw = m[12] * cs.x + m[13] * cs.y + m[14] * cs.z + m[15];
    c.r = cs.w * 1.001f + 1e-4f;
    return (c.cw + c.cx) < -c.r * pn[0] || (c.cw - c.cx) < -c.r * pn[1] || (c.cw + c.cy) < -c.r * pn[2] ||
           (c.cw - c.cy) < -c.r * pn[3] || (c.cw - 0.1f) < -c.r * pn[4];
}
__device__ __forceinline__ bool cluster_outside_tile(const ClusterClip &c, const float *tp /*RM.tile_plane[tile]*/, bool tiled, bool xtiled) {
    return (tiled && ((tp[0] * c.cw - c.cy) > c.r * tp[1] * 1.001f + 1e-4f * c.cw || (c.cy - tp[2] * c.cw) > c.r * tp[3] * 1.001f + 1e-4f * c.cw)) ||
           (xtiled && ((tp[4] * c.cw - c.cx) > c.r * tp[5] * 1.001f + 1e-4f * c.cw || (c.cx - tp[6] * c.cw) > c.r * tp[7] * 1.001f + 1e-4f * c.cw));
}

// Visibility pass of one (env, tile).  pass 0 = per-env frame: starts from the static layer's keys when D.static_vis !=
// nullptr and rasterises only the triangles of moving instances; pass 1 = static layer (instances that never move: table,
// shelf, robot base link_0; one launch at creation, result shared by all envs).  Output: the list of pixels won by a
// rasterised triangle {depth bits, pixel-in-tile << 18 | triangle}, shaded by k_shade; everything else in the image is the
// static layer, copied by k_static_copy.
struct ImageOut { unsigned char *rgb; float *depth; int *mask; size_t env_stride; /* pixels between envs */ };
// the tile's visibility buffer (file scope: the list-walking render kernels stage their shading constants in it once the
// fragment list is out -- their workgroups then need no more LDS than a raster workgroup)
__shared__ __attribute__((aligned(16))) unsigned long long g_vis[TILE_PIX];
// PRE: the caller has fetched this thread's two words of the previous frame's list (count, first entry) beside its own loads.
template <int NT_, bool CARRY = true, bool LOOPED = false, bool PRE = false>
__device__ __forceinline__ void raster_tile(const SimParams &P, const RenderModel &RM, const DevPtrs &D, int n_inst_used, int pass, int env, int tile, int restore,
                                            unsigned n_old_pre = 0u, unsigned en_first_pre = 0u) {
    unsigned long long *vis = g_vis;
    __shared__ __attribute__((aligned(16))) float mvp[RASTER_INST][16];
    __shared__ unsigned nlist, wcount, wnext;
    __shared__ unsigned short wlist[MAXWIN];
    __shared__ unsigned short wends[NT_ / 64][64];      // per wave: running ends of the lanes' left-over points (<= 64 x SMALL_AREA)
    __shared__ unsigned short clipq[CLIPQ];             // triangles that cross the near plane (rare), clipped after the window loop: position in wlist << 6 | lane
    __shared__ unsigned nclipq;
    const int W = RM.W, H = RM.H;
    // the tile: rows [row0, row0 + rows) x columns [tx0i, tx0i + cols); its visibility buffer has TW pixels per row
    const int TW = RM.tile_w, tyi = tile / RM.ntx, tx0i = (tile - tyi * RM.ntx) * TW;
    const int row0 = tyi * RM.tile_h;
    const int rows = min(RM.tile_h, H - row0), cols = min(TW, W - tx0i);
    const int npix = rows * TW;
    // (k_raster's instance -- PRE -- leaves the duration of the workgroup for the next frame's dispatch order, dispatch_order_class; the
    // start time waits in LDS: scalar registers held across the whole pass were spilled)
    __shared__ unsigned s_tc0;
    if (PRE && threadIdx.x == 0) s_tc0 = (unsigned)__builtin_amdgcn_s_memrealtime();
    int tid_ = threadIdx.x;
    if (LOOPED) asm volatile("" : "+v"(tid_));      // (inside an item loop: nothing derived from the thread index is kept live across items)
    const int tid = tid_;
    const bool layered = (pass == 0) && (D.static_vis != nullptr);
    // (incremental image update, see below: this thread's entry of the previous frame's list is fetched first -- its
    // round trip hides behind the LDS fill and the instance staging)
    // (a workgroup of an empty tile is nothing but a chain of round trips to memory -- 5 us, and two thirds of the tiles of the
    // benchmark camera are nearly empty, scratch/rwgtime.py: every load whose address is known is issued before the first wait)
    const unsigned n_old = restore ? (PRE ? n_old_pre : D.frag_count[(size_t)env * RM.ntiles + tile]) : 0u;
    const uint2 *old_lst = D.frag_list + ((size_t)env * RM.ntiles + tile) * TILE_PIX;
    const unsigned en_first = (unsigned)tid < n_old ? (PRE ? en_first_pre : old_lst[tid].y) : 0xffffffffu;
    // the cull's inputs of this thread's cluster (one cluster per thread: MAXWIN <= NT_), fetched ahead of the LDS fill and the barrier
    const int t_begin_ = ((pass == 0) && (D.static_vis != nullptr)) ? RM.first_dynamic_tri : 0;
    const int nwin_ = ((ABL(8) ? 0 : ((pass == 1) ? RM.first_dynamic_tri : RM.nt)) - t_begin_ + 63) >> 6;
    const bool cull_mine = tid < nwin_;
    const int cull_tb = min(t_begin_ + (min(tid, max(nwin_ - 1, 0)) << 6), RM.nt - 64);      // (clamped: the loads are unconditional, straight-line code)
    const int cull_inst = D.tri_inst[cull_tb];
    const float4 cull_cs = D.cluster_sphere[cull_tb >> 6];
    // The tile starts empty (an LDS-only fill); the static layer's keys are compared at compaction time and only for the
    // few pixels a moving triangle reached (min is associative) -- no 128 KB read of the static keys per env.
    // (a tile that held nothing last time most likely holds nothing now -- more than a third of all workgroups with the benchmark camera --:
    // its 32 KB are only filled once the cull has found a cluster for it)
    const bool early_fill = n_old != 0u || pass != 0;
    if (early_fill) for (int i = tid; i < npix; i += NT_) vis[i] = ~0ull;
    if (tid == 0) { nlist = 0; wcount = 0; wnext = 0; nclipq = 0; }
    stage_instances(RM, D, env, tid, NT_, mvp, nullptr);
    __syncthreads();
    WGM(2);
    // tile bounds in screen y (py = H-1-row)
    const float ty0 = (float)(H - 1 - (row0 + rows - 1)), ty1 = (float)(H - 1 - row0);
    const float txlo = (float)tx0i, txhi = (float)(tx0i + cols - 1);      // ... and in screen x
    const int NT = RM.nt;
    const int t_begin = layered ? RM.first_dynamic_tri : 0;
    const int t_end = (pass == 1) ? RM.first_dynamic_tri : NT;
    // Window queue: one thread per 64-triangle cluster ("window"; never spans two instances) runs the frustum test of the
    // cluster's bounding sphere and appends survivors to an LDS list; the waves then pull windows from that list with an
    // LDS counter, so culled windows cost nothing in the wave loops and waves that drew cheap windows take more of them.
    const int t_stop = ABL(8) ? 0 : t_end;
    const int lane = tid & 63, lx = lane & 7, ly = lane >> 3;
    const int nwin = (t_stop - t_begin + 63) >> 6;
    // tile bounds as two more planes of the cull (multi-tile images): NDC y of the tile's first and last sample rows
    const bool xtiled = RM.ntx > 1;
    const bool tiled = RM.ntiles > 1;
    // Incremental image update (do_render): the env's image in HBM still holds its previous frame.  The pixels of that
    // frame's fragment list are marked in the (still empty) visibility buffer with a key above every real one; those that
    // no triangle reaches this time leave the compaction as "vacated" entries, which k_shade puts back to the static layer.
    if (restore) {
        if (en_first != 0xffffffffu && (en_first & 0x3ffffu) != FRAG_VACATED) vis[en_first >> 18] = VIS_WAS_DYNAMIC;
        for (unsigned i = tid + NT_; i < n_old; i += NT_) {          // more than 1024 entries: rare
            const unsigned en = old_lst[i].y;
            if ((en & 0x3ffffu) != FRAG_VACATED) vis[en >> 18] = VIS_WAS_DYNAMIC;     // (a vacated entry was put back last time)
        }
    }
    static_assert(MAXWIN <= NT_, "one cluster per thread in the cull");
    if (cull_mine) {
        // the cull's camera planes: the handle's, or this env's record (env and tile are uniform in the workgroup: scalar loads)
        const float *cam_pn = RM.plane_norm, *cam_tp = RM.tile_plane[tile];
        if (D.env_cam) {
            const float *cam = D.env_cam + (size_t)__builtin_amdgcn_readfirstlane(env) * cam_floats(RM.ntiles);
            cam_pn = cam + CAM_PN; cam_tp = cam + CAM_TP + 8 * __builtin_amdgcn_readfirstlane(tile);
        }
        const int wi = tid;
        int inst = cull_inst;
        float4 cs = cull_cs;
        asm("" : "+v"(inst), "+v"(cs.x), "+v"(cs.y), "+v"(cs.z), "+v"(cs.w));      // (nothing computed from them ahead of the barrier: the wait for the two loads stays down here)
        ClusterClip cc;
        const bool out = cluster_outside_frustum(cam_pn, mvp[inst], cs, cc) || cluster_outside_tile(cc, cam_tp, tiled, xtiled);
        RSTAT(0, 1);                                // windows
        if (!out && inst < n_inst_used) wlist[atomicAdd(&wcount, 1u)] = (unsigned short)wi;
    }
    __syncthreads();
    WGM(3);
    // Every wave takes 64 consecutive triangles per window.  A triangle whose clipped bounding box holds <= SMALL_AREA
    // sample points is rasterised by its own lane; bigger ones are handed to the whole wave (ballot, v_readlane broadcast
    // of the projected triangle, 64 sample points per step in 8x8 blocks) so that one large triangle does not make 63
    // lanes wait.
    const unsigned nw = wcount;
    // Nothing reaches this tile and nothing was drawn in it last time (more than half of the lower tiles of the benchmark camera):
    // its list stays empty -- no window loop, no near-plane pass, no compaction of an untouched buffer (3 of the 6.6 us such a
    // workgroup lasts, scratch/rwgtime.py)
    if (pass == 0 && nw == 0 && n_old == 0) {
        if (tid == 0) { D.frag_count[(size_t)env * RM.ntiles + tile] = 0; RSTAT(13, 1); if (PRE && D.item_cost) D.item_cost[(size_t)env * RM.ntiles + tile] = (unsigned)__builtin_amdgcn_s_memrealtime() - s_tc0 + 1u; }
        return;
    }
    if (!early_fill) {
        for (int i = tid; i < npix; i += NT_) vis[i] = ~0ull;
        __syncthreads();
    }
#ifdef RR_RASTER_STATS
    const unsigned long long t_loop0_ = __builtin_readcyclecounter();
#endif
    PH_DECL
    for (;;) {
        unsigned k = 0;
        if (lane == 0) k = atomicAdd(&wnext, 1u);
        k = (unsigned)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= nw) break;
        PH(0);                                      // window fetch
        const int tb = t_begin + ((int)wlist[k] << 6);
        if (lane == 0) RSTAT(1, 1);                 // windows that pass the cluster test
        const int t = tb + lane;
        bool live = t < t_stop;
        const int inst = D.tri_inst[tb];
        STri s;
        int x0 = 0, y0 = 0, x1 = -1, y1 = -1, area = 0;
        bool needs_clip = false;
        float ia = 0.0f;
        {
            // The window is one cluster: lane l projects the cluster's vertex l (<= 64 distinct positions for its 64
            // triangles, so a vertex is transformed once instead of once per incident corner); every triangle lane then
            // gathers its three corners from the owning lanes (ds_bpermute).  Same arithmetic as project_tri.
            const float *cv = D.cluster_verts + (size_t)(tb >> 6) * 192;
            float psx, psy, psz;
            project_vertex(mvp[inst], cv[lane], cv[64 + lane], cv[128 + lane], W, H, psx, psy, psz);
            const int vi = D.tri_vidx[t];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int adr = (vi >> (8 * k)) & 255;               // (byte address of the owning lane: v_bfe_u32)
                s.sx[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(adr, __float_as_int(psx)));
                s.sy[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(adr, __float_as_int(psy)));
                s.sz[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(adr, __float_as_int(psz)));
                s.w[k] = 1.0f;
            }
#if defined(RR_PROBE_BPERM) || defined(RR_PROBE_VALU) || defined(RR_PROBE_DSMIN)
            // (sensitivity probes, development variants only: extra LDS permutes / VALU work / LDS atomics per window -- which pipe
            // does the kernel's duration follow?  scratch/variants)
            {
                float pv0 = psx, pv1 = psy, pv2 = psz, pv3 = psx + psy;
#ifdef RR_PROBE_BPERM
                for (int i_ = 0; i_ < RR_PROBE_BPERM / 4; i_++) { pv0 = lane_gather(pv0, (lane + 1) & 63); pv1 = lane_gather(pv1, (lane + 3) & 63); pv2 = lane_gather(pv2, (lane + 5) & 63); pv3 = lane_gather(pv3, (lane + 7) & 63); }
#endif
#ifdef RR_PROBE_VALU
#pragma unroll
                for (int i_ = 0; i_ < RR_PROBE_VALU / 4; i_++) { pv0 = __builtin_fmaf(pv0, 1.0001f, 0.5f); pv1 = __builtin_fmaf(pv1, 1.0001f, 0.5f); pv2 = __builtin_fmaf(pv2, 1.0001f, 0.5f); pv3 = __builtin_fmaf(pv3, 1.0001f, 0.5f); }
#endif
#ifdef RR_PROBE_DSMIN
                for (int i_ = 0; i_ < RR_PROBE_DSMIN; i_++) atomicMin(&vis[(lane * 61 + i_ * 7) & (TILE_PIX - 1)], ~0ull);      // (never changes a key)
#endif
                if (pv0 + pv1 + pv2 + pv3 == 12345.678f) s.sz[0] = pv0;
            }
#endif
            // corners nearer than the near plane (sx = NaN): none -> the ordinary paths below; all -> nothing to draw;
            // one or two -> the triangle is clipped against the plane by the whole wave (rare, see the end of the loop body)
            // (a NaN among the three sx: their sum is NaN; all three: their minimum is NaN too -- v_min3 returns a number when it has one)
            const float sxsum = s.sx[0] + s.sx[1] + s.sx[2], sxmin = fminf(s.sx[0], fminf(s.sx[1], s.sx[2]));
            const bool any_near = sxsum != sxsum, all_near = sxmin != sxmin;
            needs_clip = live && any_near && !all_near;
            live = live && !any_near;
        }
        PH(1);                                      // loads, projection, corner gather
        {
            // Straight-line set-up for all 64 lanes (nested `if (live)` blocks save nothing in lock-step and cost exec-mask bookkeeping
            // and re-initialisation on every path): box, clamps as one v_med3 each -- the visibility test in front of them
            // guarantees xmax >= the tile's first column, xmin <= its last, ... so med3(x, lo, hi) is max(x, lo) resp. min(x, hi): the
            // oracle's box clipped to the tile --,
            // signed area and its reciprocal; a lane that is not live ends with area 0.
            const float xmin = fminf(s.sx[0], fminf(s.sx[1], s.sx[2])), xmax = fmaxf(s.sx[0], fmaxf(s.sx[1], s.sx[2]));
            const float ymin = fminf(s.sy[0], fminf(s.sy[1], s.sy[2])), ymax = fmaxf(s.sy[0], fmaxf(s.sy[1], s.sy[2]));
            bool on = live && !(xmax < txlo || ymax < ty0 || xmin > txhi || ymin > ty1);
            const TriEdge te = tri_edge(s);
            x0 = (int)ceilf(__builtin_amdgcn_fmed3f(xmin, txlo, txhi)); x1 = (int)floorf(__builtin_amdgcn_fmed3f(xmax, txlo, txhi));
            y0 = (int)ceilf(__builtin_amdgcn_fmed3f(ymin, ty0, ty1)); y1 = (int)floorf(__builtin_amdgcn_fmed3f(ymax, ty0, ty1));
            on = on && !(x1 < x0 || y1 < y0) && te.ok;
            ia = te.ia;
            area = on ? (x1 - x0 + 1) * (y1 - y0 + 1) : 0;
            live = on;
        }
        PH(2);                                      // bounding box, set-up
        if (ABL(1)) continue;
        const bool big = live && area > SMALL_AREA;
#ifdef RR_RASTER_STATS
        {
            const unsigned long long lm = __ballot(live), bm = __ballot(big);
            int sa_ = (live && !big) ? area : 0, mx = sa_, sm = sa_;
            for (int o = 32; o; o >>= 1) { mx = max(mx, __shfl_xor(mx, o)); sm += __shfl_xor(sm, o); }
            if (lane == 0) {
                RSTAT(2, __popcll(lm)); RSTAT(3, __popcll(bm)); RSTAT(4, sm); RSTAT(5, mx);
                if (lm) RSTAT(6, 1);
                if (lm & ~bm) RSTAT(7, 1);
            }
            if (big) RSTAT(8, area);
        }
#endif
        // Small triangles.  Most cover one or two sample points, a few up to small_area: a per-lane walk of the whole
        // bounding box makes the wave wait for its largest triangle (~20 % lane utilisation).  So every lane walks only
        // the first INLINE_PIX points of its box; the remaining points of all lanes are dealt out evenly: a wave prefix
        // sum numbers them, each lane takes points lane, lane+64, ..., finds the owner with a 6-step binary search over
        // the running ends (64 ints of LDS per wave), fetches the owner's triangle with ds_bpermute and tests its point.
        // Same per-point arithmetic, and ds_min is order independent.
        {
            const bool small = live && !big;
            const int bw = x1 - x0 + 1;
            const int ninl = small ? min(area, INLINE_PIX) : 0;
#if INLINE_PIX == 2
            // (written out: the first point of the box, then its right neighbour -- or the point below it when the box is one
            // column wide; a loop with a per-lane trip count pays for its bookkeeping in every iteration)
            if (!CARRY) {        // (the list-walking kernels: three registers fewer around their item loop)
                if (ninl > 0) raster_pixel_hoisted(s, ia, t, x0, y0, H, TW, row0, vis, tx0i);
                if (ninl > 1) raster_pixel_hoisted(s, ia, t, bw > 1 ? x0 + 1 : x0, bw > 1 ? y0 : y0 + 1, H, TW, row0, vis, tx0i);
            } else {
                // (coordinates as floats and the buffer index carried from the first point to the second: one conversion pair and
                // one integer multiply per triangle instead of per point)
                const float fx0 = (float)x0, fy0 = (float)y0;
                const int vi0 = (H - 1 - y0 - row0) * TW + x0 - tx0i;
                const bool wide = bw > 1;
                if (ninl > 0) raster_pixel_at(s, ia, t, fx0, fy0, vi0, vis);
                if (ninl > 1) raster_pixel_at(s, ia, t, wide ? fx0 + 1.0f : fx0, wide ? fy0 : fy0 + 1.0f, wide ? vi0 + 1 : vi0 - TW, vis);
            }
#else
            int px = x0, py = y0;
            for (int i = 0; i < ninl; i++) {
                raster_pixel_hoisted(s, ia, t, px, py, H, TW, row0, vis, tx0i);
                if (++px > x1) { px = x0; py++; }
            }
#endif
            PH(3);                                  // in-lane sample points
            const int rem = small ? area - ninl : 0;
            int total;
            const int pre = wave_excl_scan(rem, lane, total);
            PH(4);                                  // scan
            if (total > 0) {
                unsigned short *we = wends[tid >> 6];
                we[lane] = (unsigned short)(pre + rem);                                // inclusive ends, non-decreasing over the lanes
                // (box origin relative to the tile, box width and the lane's first point number in one word: one ds_bpermute per round
                // instead of four -- an LDS permute costs the CU six cycles, three times a 4-byte LDS read (tools/ubench/valu_issue.hip).
                // 14 bits of origin: column in tile_xbits, row above it -- a tile has <= 4096 pixels --; 6 of width - 1: a small box is at
                // most 64 wide; 12 of point number: at most 64 x 62 left-over points)
                const int ty0i = H - row0 - rows, xb = RM.tile_xbits;                  // (screen y of the tile's lowest row)
                const int packed = (x0 - tx0i) | ((y0 - ty0i) << xb) | ((bw - 1) << 14) | (pre << 20);
                for (int w0 = 0; w0 < total; w0 += 64) {             // wave-uniform trip count: ds_bpermute needs the owner lanes active
                    const int w = w0 + lane;
                    const bool valid = w < total;
                    int src = 0;                                     // owner = number of lanes whose points end at or before w
#pragma unroll
                    for (int step = 32; step; step >>= 1) if ((int)we[src + step - 1] <= w) src += step;
                    src = valid ? src : 0;
                    STri bs;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        bs.sx[k] = lane_gather(s.sx[k], src); bs.sy[k] = lane_gather(s.sy[k], src); bs.sz[k] = lane_gather(s.sz[k], src);
                        bs.w[k] = 1.0f;
                    }
                    const float bia = lane_gather(ia, src);
                    const int pk = lane_gather_i(packed, src);
                    const int sx0 = (pk & ((1 << xb) - 1)) + tx0i, sy0 = ((pk & 0x3fff) >> xb) + ty0i, sbw = ((pk >> 14) & 63) + 1;
                    const int idx = INLINE_PIX + w - (int)((unsigned)pk >> 20);
                    // row of point idx in a box sbw wide: (idx + 0.5) / sbw lies at least 0.5 / 64 from an integer, far more than the
                    // error of the approximate reciprocal on these small integers (idx < 64 + INLINE_PIX, sbw <= 64)
                    const int ry = (int)(((float)idx + 0.5f) * __builtin_amdgcn_rcpf((float)sbw));
                    if (valid) raster_pixel_hoisted(bs, bia, tb + src, sx0 + idx - ry * sbw, sy0 + ry, H, TW, row0, vis, tx0i);
                }
            }
            PH(5);                                  // redistribution rounds
        }
        unsigned long long todo = ABL(2) ? 0ull : __ballot(big);
        while (todo) {        // wave-cooperative: all 64 lanes rasterise the triangle of lane `src`
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            STri bs;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                bs.sx[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.sx[k]), src));
                bs.sy[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.sy[k]), src));
                bs.sz[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.sz[k]), src));
                bs.w[k] = 1.0f;
            }
            const float bia = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ia), src));
            const int bt = tb + src;
            const int bx0 = __builtin_amdgcn_readlane(x0, src), by0 = __builtin_amdgcn_readlane(y0, src);
            const int bw = __builtin_amdgcn_readlane(x1, src) - bx0 + 1, bh = __builtin_amdgcn_readlane(y1, src) - by0 + 1;
            const int nbx = (bw + 7) >> 3, nby = (bh + 7) >> 3, nblk = nbx * nby;
            if (nblk <= 4) {
                for (int by = 0; by < bh; by += 8)
                    for (int bx = 0; bx < bw; bx += 8) {
                        const int ox = bx + lx, oy = by + ly;
                        if (ox < bw && oy < bh) raster_pixel_hoisted(bs, bia, bt, bx0 + ox, by0 + oy, H, TW, row0, vis, tx0i);
                    }
                continue;
            }
            // Hierarchical: each lane first classifies one 8x8 block (64 blocks per step) with the conservative corner
            // test; only blocks that may hold covered sample points are rasterised.  Triangles close to the near plane
            // project to slivers whose clipped bounding box is the whole image -- without this they dominate the kernel.
            // delta bounds |float - exact| of a barycentric anywhere in the tile: each edge function is a difference of
            // two products of magnitude <= X*Y (X = max|sx|+W, Y = max|sy|+H), evaluated with <= 4 roundings.
            const float X = fmaxf(fabsf(bs.sx[0]), fmaxf(fabsf(bs.sx[1]), fabsf(bs.sx[2]))) + (float)W;
            const float Y = fmaxf(fabsf(bs.sy[0]), fmaxf(fabsf(bs.sy[1]), fabsf(bs.sy[2]))) + (float)H;
            const float delta2 = 2.0f * (8.0e-6f * X * Y * fabsf(bia) + 1.0e-6f);
            const float inbx = 1.0f / (float)nbx;
            if (lane == 0) { RSTAT(10, 1); }
            for (int c0 = 0; c0 < nblk; c0 += 64) {
                const int bi = c0 + lane;
                bool keep = false;
                if (bi < nblk) {
                    const int byi = (int)(((float)bi + 0.5f) * inbx), bxi = bi - byi * nbx;
                    const int px0 = bx0 + 8 * bxi, py0 = by0 + 8 * byi;
                    keep = block_may_overlap(bs, bia, px0, min(px0 + 7, bx0 + bw - 1), py0, min(py0 + 7, by0 + bh - 1), delta2);
                }
                unsigned long long km = __ballot(keep);
                while (km) {
                    const int j = c0 + __ffsll((long long)km) - 1;
                    km &= km - 1;
                    const int byi = (int)(((float)j + 0.5f) * inbx), bxi = j - byi * nbx;
                    const int ox = 8 * bxi + lx, oy = 8 * byi + ly;
                    if (lane == 0) RSTAT(9, 1);     // 8x8 blocks rasterised by the hierarchical path
                    if (ox < bw && oy < bh) raster_pixel_hoisted(bs, bia, bt, bx0 + ox, by0 + oy, H, TW, row0, vis, tx0i);
                }
            }
        }
        PH(6);                                      // wave-cooperative large triangles
        // triangles that cross the near plane are rare: they are queued and clipped after the window loop
        if (needs_clip && !ABL(16)) { const unsigned qi = atomicAdd(&nclipq, 1u); if (qi < CLIPQ) clipq[qi] = (unsigned short)((k << 6) | lane); }
    }
    PH(7);                                          // last fetch + (below) waiting for the other waves
    // ---- triangles that cross the near plane (queued above): clipped against w = NEAR_W (Sutherland-Hodgman, the oracle's
    // clip_near()) into a triangle or a fan of two, which a whole wave rasterises under the original triangle id
    __syncthreads();
    PH(8);
    WGM(4);
    for (unsigned qi = tid >> 6; qi < min(nclipq, (unsigned)CLIPQ); qi += NT_ / 64) {
        const int bt = t_begin + ((int)wlist[clipq[qi] >> 6] << 6) + (clipq[qi] & 63);
        const int tb = bt & ~63;
        const int inst = D.tri_inst[tb];
        STri ta, tb2;
        int nsub = 0;
        {
            const int cvi = D.tri_vidx[bt];
                const float *cv = D.cluster_verts + (size_t)(tb >> 6) * 192;
            float c0[4], c1[4], c2[4];
            { const int i0 = (cvi & 255) >> 2, i1 = ((cvi >> 8) & 255) >> 2, i2 = ((cvi >> 16) & 255) >> 2;
              clip_vertex(mvp[inst], cv[i0], cv[64 + i0], cv[128 + i0], c0);
              clip_vertex(mvp[inst], cv[i1], cv[64 + i1], cv[128 + i1], c1);
              clip_vertex(mvp[inst], cv[i2], cv[64 + i2], cv[128 + i2], c2); }
            const bool in0 = c0[3] >= NEAR_W, in1 = c1[3] >= NEAR_W, in2 = c2[3] >= NEAR_W;
            float e01[4] = {0, 0, 0, 1}, e12[4] = {0, 0, 0, 1}, e20[4] = {0, 0, 0, 1};
            if (in0 != in1) { if (in0) clip_edge(c0, c1, e01); else clip_edge(c1, c0, e01); }
            if (in1 != in2) { if (in1) clip_edge(c1, c2, e12); else clip_edge(c2, c1, e12); }
            if (in2 != in0) { if (in2) clip_edge(c2, c0, e20); else clip_edge(c0, c2, e20); }
            // polygon in Sutherland-Hodgman order: [v0] [x01] [v1] [x12] [v2] [x20] with the absent ones left out (values
            // are copied, not pointed to: private arrays behind pointers would live in scratch memory)
            float p0[4], p1[4], p2[4], p3[4];
#define CP4(D_, S_) { D_[0] = S_[0]; D_[1] = S_[1]; D_[2] = S_[2]; D_[3] = S_[3]; }
            CP4(p0, c0) CP4(p1, c0) CP4(p2, c0) CP4(p3, c0)
            const int msk = (in0 ? 1 : 0) | (in1 ? 2 : 0) | (in2 ? 4 : 0);       // wave-uniform
            if (msk == 1) { CP4(p0, c0) CP4(p1, e01) CP4(p2, e20) nsub = 1; }
            else if (msk == 2) { CP4(p0, e01) CP4(p1, c1) CP4(p2, e12) nsub = 1; }
            else if (msk == 4) { CP4(p0, e12) CP4(p1, c2) CP4(p2, e20) nsub = 1; }
            else if (msk == 3) { CP4(p0, c0) CP4(p1, c1) CP4(p2, e12) CP4(p3, e20) nsub = 2; }
            else if (msk == 6) { CP4(p0, e01) CP4(p1, c1) CP4(p2, c2) CP4(p3, e20) nsub = 2; }
            else if (msk == 5) { CP4(p0, c0) CP4(p1, e01) CP4(p2, e12) CP4(p3, c2) nsub = 2; }
#undef CP4
            clip_to_screen(p0, W, H, ta.sx[0], ta.sy[0], ta.sz[0]);          // fan (0, 1, 2), (0, 2, 3)
            clip_to_screen(p1, W, H, ta.sx[1], ta.sy[1], ta.sz[1]);
            clip_to_screen(p2, W, H, ta.sx[2], ta.sy[2], ta.sz[2]);
            tb2.sx[0] = ta.sx[0]; tb2.sy[0] = ta.sy[0]; tb2.sz[0] = ta.sz[0];
            tb2.sx[1] = ta.sx[2]; tb2.sy[1] = ta.sy[2]; tb2.sz[1] = ta.sz[2];
            clip_to_screen(p3, W, H, tb2.sx[2], tb2.sy[2], tb2.sz[2]);
            ta.w[0] = ta.w[1] = ta.w[2] = tb2.w[0] = tb2.w[1] = tb2.w[2] = 1.0f;
        }
        for (int sub = 0; sub < nsub; sub++) {
            STri bs;
#pragma unroll
            for (int k = 0; k < 3; k++) { bs.sx[k] = sub ? tb2.sx[k] : ta.sx[k]; bs.sy[k] = sub ? tb2.sy[k] : ta.sy[k]; bs.sz[k] = sub ? tb2.sz[k] : ta.sz[k]; bs.w[k] = 1.0f; }
            // clipped bounding box and reciprocal area: the same arithmetic as the per-lane set-up above
            const float xmin = fminf(bs.sx[0], fminf(bs.sx[1], bs.sx[2])), xmax = fmaxf(bs.sx[0], fmaxf(bs.sx[1], bs.sx[2]));
            const float ymin = fminf(bs.sy[0], fminf(bs.sy[1], bs.sy[2])), ymax = fmaxf(bs.sy[0], fmaxf(bs.sy[1], bs.sy[2]));
            if (xmax < txlo || ymax < ty0 || xmin > txhi || ymin > ty1) continue;
            const int bx0 = (int)ceilf(fmaxf(xmin, txlo)), bx1 = (int)floorf(fminf(xmax, txhi));
            const int by0 = (int)ceilf(fmaxf(ymin, ty0)), by1 = (int)floorf(fminf(ymax, ty1));
            if (bx1 < bx0 || by1 < by0) continue;
            const TriEdge te = tri_edge(bs);
            if (!te.ok) continue;
            const float bia = te.ia;
            const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
            const int nbx = (bw + 7) >> 3, nby = (bh + 7) >> 3, nblk = nbx * nby;
            if (nblk <= 4) {
                for (int by = 0; by < bh; by += 8)
                    for (int bx = 0; bx < bw; bx += 8) {
                        const int ox = bx + lx, oy = by + ly;
                        if (ox < bw && oy < bh) raster_pixel_hoisted(bs, bia, bt, bx0 + ox, by0 + oy, H, TW, row0, vis, tx0i);
                    }
                continue;
            }
            // Hierarchical: each lane first classifies one 8x8 block (64 blocks per step) with the conservative corner
            // test; only blocks that may hold covered sample points are rasterised.  Triangles close to the near plane
            // project to slivers whose clipped bounding box is the whole image -- without this they dominate the kernel.
            // delta bounds |float - exact| of a barycentric anywhere in the tile: each edge function is a difference of
            // two products of magnitude <= X*Y (X = max|sx|+W, Y = max|sy|+H), evaluated with <= 4 roundings.
            const float X = fmaxf(fabsf(bs.sx[0]), fmaxf(fabsf(bs.sx[1]), fabsf(bs.sx[2]))) + (float)W;
            const float Y = fmaxf(fabsf(bs.sy[0]), fmaxf(fabsf(bs.sy[1]), fabsf(bs.sy[2]))) + (float)H;
            const float delta2 = 2.0f * (8.0e-6f * X * Y * fabsf(bia) + 1.0e-6f);
            const float inbx = 1.0f / (float)nbx;
            if (lane == 0) { RSTAT(10, 1); }
            for (int c0 = 0; c0 < nblk; c0 += 64) {
                const int bi = c0 + lane;
                bool keep = false;
                if (bi < nblk) {
                    const int byi = (int)(((float)bi + 0.5f) * inbx), bxi = bi - byi * nbx;
                    const int px0 = bx0 + 8 * bxi, py0 = by0 + 8 * byi;
                    keep = block_may_overlap(bs, bia, px0, min(px0 + 7, bx0 + bw - 1), py0, min(py0 + 7, by0 + bh - 1), delta2);
                }
                unsigned long long km = __ballot(keep);
                while (km) {
                    const int j = c0 + __ffsll((long long)km) - 1;
                    km &= km - 1;
                    const int byi = (int)(((float)j + 0.5f) * inbx), bxi = j - byi * nbx;
                    const int ox = 8 * bxi + lx, oy = 8 * byi + ly;
                    if (lane == 0) RSTAT(9, 1);     // 8x8 blocks rasterised by the hierarchical path
                    if (ox < bw && oy < bh) raster_pixel_hoisted(bs, bia, bt, bx0 + ox, by0 + oy, H, TW, row0, vis, tx0i);
                }
            }
        }
    }
    PH(9);                                          // near-plane pass
    PH_FLUSH;
    WGM(5);
#ifdef RR_RASTER_STATS
    const unsigned long long t_exit_ = __builtin_readcyclecounter();
#endif
    __syncthreads();
#ifdef RR_RASTER_STATS
    if (lane == 0 && (P.ablate & 0x2000)) {   // RR_ABLATE=8192: only these two (idle at the barrier / busy in the loop)
        atomicAdd(&g_rstats[14], (unsigned long long)(__builtin_readcyclecounter() - t_exit_)); atomicAdd(&g_rstats[15], (unsigned long long)(t_exit_ - t_loop0_));
    }
#endif
    if (pass == 1) {   // publish the static layer's keys: the shared layer is built as env 0, an env's own layer (per-env cameras) as that env
        unsigned long long *sv = D.static_vis_out + (size_t)env * W * H + (size_t)row0 * W + tx0i;
        for (int i = tid; i < npix; i += NT_) { const int lr = i / TW, lx = i - lr * TW; if (lx < cols) sv[(size_t)lr * W + lx] = vis[i]; }
    }
    // ---- compaction: pixels owned by a triangle rasterised in this pass go to the fragment list of this (env, tile)
    // (the comparison with the static layer's key is left to k_shade: a dependent global read at the tail of this
    // LDS-limited workgroup is exposed latency, in the high-occupancy shading kernel it is not)
    uint2 *lst = D.frag_list + ((size_t)env * RM.ntiles + tile) * TILE_PIX;
#ifdef RR_RASTER_STATS
    __shared__ unsigned win_bits[MAXWIN / 32];      // clusters that own a pixel of the tile at the end
    for (int i = tid; i < MAXWIN / 32; i += NT_) win_bits[i] = 0;
    __syncthreads();
    for (int i = tid; i < npix; i += NT_) {
        const unsigned long long key = vis[i];
        if (key != ~0ull && key != VIS_WAS_DYNAMIC) { const unsigned w_ = ((unsigned)(key & 0xffffffffu) - (unsigned)t_begin) >> 6; atomicOr(&win_bits[w_ >> 5], 1u << (w_ & 31)); }
    }
    __syncthreads();
    if (tid < MAXWIN / 32) RSTAT(11, __popc(win_bits[tid]));      // (slot 11 reused: clusters with at least one winning pixel)
#endif
    // (one LDS atomic per wave and trip -- ballot, popcount, v_mbcnt -- instead of one per listed pixel: ~300 same-address atomics
    // per tile serialise in the LDS; the order of the list is immaterial)
    for (int i0 = 0; i0 < npix; i0 += NT_) {
        const int i = i0 + tid;
        const unsigned long long key = i < npix ? vis[i] : ~0ull;
        const unsigned tri = key == VIS_WAS_DYNAMIC ? FRAG_VACATED : (unsigned)(key & 0xffffffffu);
        const bool has = key != ~0ull;
        const unsigned long long hm = __ballot(has);
        if (hm == 0ull) continue;                       // (wave-uniform)
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&nlist, (unsigned)__popcll(hm));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (has) {
            const unsigned slot = base + __builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u));
            lst[slot] = make_uint2((unsigned)(key >> 32), ((unsigned)i << 18) | tri);
        }
    }
    __syncthreads();
    if (tid == 0 && nclipq > CLIPQ) atomicOr(&D.errflags[env], 8u);      // (clip queue overflow: triangles were dropped; a RENDER status -- the solve's dead mask ignores bit 8)
    WGM(6);
    if (PRE && pass == 0 && tid == 0 && D.item_cost) D.item_cost[(size_t)env * RM.ntiles + tile] = (unsigned)__builtin_amdgcn_s_memrealtime() - s_tc0 + 1u;      // (100 MHz ticks)
    if (tid == 0) { D.frag_count[(size_t)env * RM.ntiles + tile] = nlist; RSTAT(12, nlist); RSTAT(13, 1); RSTAT(14, nclipq); RSTAT(15, nclipq > 0 ? 1 : 0); }
}

// One workgroup per (env, tile); sel (env_selected): all envs, or only those of light solver groups.
// Grid (envs, tiles) -- or, with D.item_perm (pass 0), one dimension of envs * tiles workgroups that take the items in the order of
// dispatch_order_class: the hardware deals workgroups out by their linear index -- XCD = index mod 8, shader engine = (index / 8) mod 4,
// strictly in turn: a shader engine whose four slots per CU are taken holds up its XCD's queue -- so the index order decides how evenly
// the 32 engines are loaded (scratch/rwgtime.py, scratch/rorder.py: env order 0.708 of the slots busy, cost order 0.842).
__global__ void __launch_bounds__(RASTER_THREADS) RASTER_ATTR k_raster(SimParams P, const RenderModel *RMp, DevPtrs D, int n_inst_used, int pass, int env0, int restore, int sel) {
    int env, tile;
    if (pass == 0 && D.item_perm) { const unsigned it = D.item_perm[blockIdx.x]; if (it == 0xffffffffu) return; env = (int)(it >> 8); tile = (int)(it & 255u); }
    else { env = blockIdx.x + env0; tile = blockIdx.y; }
#ifdef RR_RASTER_STATS
    { const RenderModel &RM = *RMp; WGM(0); }
#endif
    // (the two selection flags and this thread's words of the previous frame's list in ONE round trip, then the branches)
    const size_t item = (size_t)env * RMp->ntiles + tile;
    const bool flagged = pass == 0 && D.render_flags != nullptr;
    const unsigned char rflag = (flagged ? D.render_flags : (const unsigned char *)D.hgflag)[env];
    const int cls = D.hgflag[env];
    const unsigned n_old_pre = D.frag_count[item];
    const unsigned en_first_pre = D.frag_list[item * TILE_PIX + threadIdx.x].y;
    // (one branch on all four: none of the loads can be moved behind it.  The last term is never true -- N > 0 --, whatever the
    // two words hold)
    const int selected = (int)(sel == 0) | ((int)(sel == 1) & (int)(cls == 0)) | ((int)(sel == 2) & (int)(cls == 1)) | ((int)(sel == 3) & (int)(cls == 2));
    if (((int)flagged & (int)(rflag == 0)) | (selected ^ 1) | ((int)(P.N < 0) & ((int)(n_old_pre > 0x7fffffffu) | (int)((en_first_pre >> 30) == 2u)))) return;
#ifdef RR_RASTER_STATS
    unsigned long long wt0_ = 0;
    if (P.ablate & 0x4000) wt0_ = __builtin_amdgcn_s_memrealtime();
    { const RenderModel &RM = *RMp; WGM(1); }
#endif
    raster_tile<RASTER_THREADS, true, false, true>(P, *RMp, D, n_inst_used, pass, env, tile, restore, n_old_pre, en_first_pre);
#ifdef RR_RASTER_STATS
    if ((P.ablate & 0x4000) && threadIdx.x == 0) {
        unsigned long long *g = g_rwg_time[(env * RMp->ntiles + tile) & 65535];
        g[0] = wt0_; g[1] = __builtin_amdgcn_s_memrealtime();
        g[2] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11)) << 32);
    }
#endif
}

// (dispatch_order_class -- the counting sort behind the cost-ordered dispatch of k_raster and k_collide -- is in realrobot.hip)

#ifndef LIST_CARRY
#define LIST_CARRY false
#endif
#ifndef LIST_WAVES
#define LIST_WAVES 6         // (79 VGPRs: three workgroups per CU -- since nothing derived from the thread index stays live across the items of the loop)
#endif
#define RASTER_LIST_WGS 768      // three per CU: the item loop around the tile needs more than the 64 VGPRs of four (a long list of heavy
                                 // envs must not be rendered at a fraction of the occupancy)
// The heavy envs (D.hlist, D.hcount -- known on the device only): a fixed number of workgroups walk the
// list, so that no LDS-filling workgroup is launched just to find that its env is not on it.
__global__ void __launch_bounds__(RASTER_THREADS) __attribute__((amdgpu_waves_per_eu(LIST_WAVES, 8))) k_raster_list(SimParams P, const RenderModel *RMp, DevPtrs D, int n_inst_used, int restore, int which) {
    const RenderModel &RM = *RMp;
    int *hcount = which ? D.hcount2 : D.hcount;
    const int *hlist = which ? D.hlist2 : D.hlist;
    const int nitems = hcount[0] * RM.ntiles;
    __shared__ int s_item;
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&hcount[1], 1);      // dynamic assignment: tiles differ a lot in cost
        __syncthreads();
        const int it = s_item;
        if (it >= nitems) break;
        const int tile = it % RM.ntiles, ge = it / RM.ntiles;
        const int env = hlist[ge];
        if (env < P.N && !(D.render_flags && !D.render_flags[env])) raster_tile<RASTER_THREADS, LIST_CARRY, true>(P, RM, D, n_inst_used, 0, env, tile, restore);
        __syncthreads();        // the LDS of the tile is reused
    }
}

// Image targets of k_static_copy / k_shade: the per-env observation buffers (pass 0) or the shared static layer (pass 1).

// Copies the static layer (or the background when there is none) into the images of every rendered env: 4 pixels per
// thread (W % 4 == 0 enforced at create).  Pure streaming: reads hit L2, writes are the obs bytes of SURVEY 8(d).
// stale != nullptr: only the rendered envs whose byte is set (images that predate the current static layer, rr_set_camera).
#define COPY_THREADS 256
__global__ void __launch_bounds__(COPY_THREADS) k_static_copy(const RenderModel *RMp, DevPtrs D, ImageOut out, int use_flags, int N,
                                                              const unsigned char *stale) {
    const int ngroups = (RMp->W * RMp->H) >> 2;
    for (int env = blockIdx.y; env < N; env += gridDim.y) {
    if (use_flags && D.render_flags && !D.render_flags[env]) continue;
    if (stale && !stale[env]) continue;
    const size_t base = (size_t)env * out.env_stride, sbase = D.static_stride * env;      // (sbase: the env's own layer, per-env cameras)
    for (int g = blockIdx.x * COPY_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * COPY_THREADS) {
        const unsigned *srgb = (const unsigned *)(D.static_rgb + 3 * sbase) + (size_t)3 * g;      // (3 H W is a multiple of 4: W % 4 == 0)
        const unsigned r0 = srgb[0], r1 = srgb[1], r2 = srgb[2];
        const float4 dv = *(const float4 *)(D.static_depth + sbase + (size_t)4 * g);
        unsigned *rgbp = (unsigned *)(out.rgb + (base + (size_t)4 * g) * 3);
        rgbp[0] = r0; rgbp[1] = r1; rgbp[2] = r2;
        *(float4 *)(out.depth + base + (size_t)4 * g) = dv;
        if (out.mask) *(int4 *)(out.mask + base + (size_t)4 * g) = *(const int4 *)(D.static_mask + sbase + (size_t)4 * g);
    }
    }
}

// Behind k_static_copy(stale): the rendered stale envs hold the full static layer now -- empty fragment lists (nothing to
// restore), no longer stale.  One thread per env.
__global__ void k_stale_clear(const RenderModel *RMp, DevPtrs D, int N, unsigned char *stale) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N || !stale[env] || (D.render_flags && !D.render_flags[env])) return;
    const int nt = RMp->ntiles;
    for (int t = 0; t < nt; t++) D.frag_count[(size_t)env * nt + t] = 0u;
    stale[env] = 0;
}

// Background fill of the static images (before the static layer is shaded): the shared layer (N = 1), or the layers of the
// envs whose mask byte is set (per-env cameras; mask == nullptr: all N).
__global__ void k_background(const RenderModel *RMp, DevPtrs D, int N, const unsigned char *mask) {
    const int npx = RMp->W * RMp->H;
    for (int env = blockIdx.y; env < N; env += gridDim.y) {
    if (mask && !mask[env]) continue;
    unsigned char *rgb = D.static_rgb + 3 * D.static_stride * env;
    float *depth = D.static_depth + D.static_stride * env;
    int *msk = D.static_mask + D.static_stride * env;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
        rgb[3 * i] = 255; rgb[3 * i + 1] = 255; rgb[3 * i + 2] = 255;
        depth[i] = 1.0f; msk[i] = -1;
    }
    }
}

// Per-env cameras: the visibility keys of the shared static layer into every env's layer (the images go by k_static_copy).
__global__ void k_static_vis_spread(const unsigned long long *src, unsigned long long *dst, size_t npx, int N) {
    for (int env = blockIdx.y; env < N; env += gridDim.y)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) dst[(size_t)env * npx + i] = src[i];
}

// Per-env cameras, behind the rebuild of the static layers of the envs whose mask byte is set: their fragment lists (scratch
// of the rebuild) are empty, and -- stale != nullptr -- their images predate their new layer (a full copy at their next render).
__global__ void k_camera_changed(const RenderModel *RMp, DevPtrs D, int N, const unsigned char *mask, unsigned char *stale) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N || !mask[env]) return;
    const int nt = RMp->ntiles;
    for (int t = 0; t < nt; t++) D.frag_count[(size_t)env * nt + t] = 0u;
    if (stale) stale[env] = 1;
}

// Deferred shading of the fragment lists, one lane per listed pixel.  Every (env, tile) list is dealt out in
// SHADE_THREADS-entry chunks to SHADE_SPLIT workgroups (blocks whose first chunk lies beyond the list exit at once).
// A/B (k_shade, ms): 64x16 0.175, 128x8 0.145, 256x8 0.131, 256x2 0.122, 512x2 0.119, 1024x1 0.120 -- the per-block
// staging of the instance constants outweighs the tail of long lists.
#ifndef SHADE_THREADS
#define SHADE_THREADS 256
#endif
#ifndef SHADE_SPLIT
#define SHADE_SPLIT 2       // with four tiles per env a list holds ~300 entries: 256 x 8 0.113 ms, x 4 0.101, x 2 0.098, 512 x 1 0.106, 128 x 3 0.100
#endif
// chunk z of nz of the fragment list of (env, tile); mvp / sinst: the workgroup's staging arrays
// Deferred shading of chunk z of nz of the fragment list of (env, tile) by the calling workgroup.
#ifdef RR_RASTER_STATS
// marks inside a shading workgroup (thread 0, first trip of its loop; 100 MHz clock; scratch/rwgtime.py shade): 1 count known,
// 2 instance constants staged, 3 list entry arrived, 4 static key + triangle record arrived, 5 pixel shaded (texel arrived), 6 stores issued
#define SHM(i) do { if ((g_shade_ablate & 0x10000) && threadIdx.x == 0 && first_) g_rwg_marks[((env * RM.ntiles + tile) * nz + z) & 65535][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SHM(i)
#endif
template <int NTHREADS>
__device__ __forceinline__ void shade_block(const RenderModel &RM, const DevPtrs &D, const ImageOut &out, int env, int tile, int z, int nz,
                                            float (*mvp)[16], float (*sinst)[16]) {
    const unsigned n = D.frag_count[(size_t)env * RM.ntiles + tile];
    if ((unsigned)z * NTHREADS >= n) return;                    // (workgroup-uniform)
    bool first_ = true;
    SHM(1);
    stage_instances(RM, D, env, threadIdx.x, NTHREADS, mvp, sinst);
    __syncthreads();
    SHM(2);
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 8)
    if (mvp[0][0] != 12345.678f) return;           // (probe: the prologue only -- count, instance constants, barrier)
#endif
    ShadeCtx ctx;
    ctx.D = &D; ctx.mvp = &mvp[0][0]; ctx.sinst = &sinst[0][0]; ctx.W = RM.W; ctx.H = RM.H;
    shade_light(D, env, ctx);
    const uint2 *lst = D.frag_list + ((size_t)env * RM.ntiles + tile) * TILE_PIX;
    const int tyi = tile / RM.ntx, row0 = tyi * RM.tile_h, tx0i = (tile - tyi * RM.ntx) * RM.tile_w;
    const size_t ebase = (size_t)env * out.env_stride;
    const size_t sbase = D.static_stride * env;                  // the env's own static layer (per-env cameras), else 0
    const unsigned long long *sv = D.static_vis ? D.static_vis + sbase : nullptr;     // null while the static layer itself is built
    for (unsigned i = z * NTHREADS + threadIdx.x; i < n; i += nz * NTHREADS) {
        const uint2 f = lst[i];
#ifdef RR_RASTER_STATS
        if (g_shade_ablate & 0x10000) { asm volatile("" :: "v"(f.x), "v"(f.y)); SHM(3); }
#endif
        const int pi = (int)(f.y >> 18), t = (int)(f.y & 0x3ffffu);
        // pixel-in-tile index -> row and column of the image (tile_w pixels per buffer row; multiply-high instead of a division)
        const int lrow = (int)__umulhi((unsigned)pi, RM.w_magic), px = tx0i + pi - lrow * RM.tile_w;
        const size_t gp = (size_t)(row0 + lrow) * RM.W + (size_t)px;        // pixel of the image / of the static layer
        // a moving triangle only shows where it beats the static layer (depth, then triangle id; static ids are lower);
        // where it does not, and where the previous frame's fragment has gone, the pixel goes back to the static layer
        // (the image persists in HBM from frame to frame, do_render)
        if (t == (int)FRAG_VACATED || (sv && !((((unsigned long long)f.x << 32) | (unsigned)t) < sv[gp]))) {
            // (vacated entries only exist in env frames)
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 128)
            continue;       // (probe: what does the put-back path cost?)
#endif
            const size_t so = sbase + gp, o = ebase + gp;
            out.rgb[o * 3] = D.static_rgb[so * 3]; out.rgb[o * 3 + 1] = D.static_rgb[so * 3 + 1]; out.rgb[o * 3 + 2] = D.static_rgb[so * 3 + 2];
            out.depth[o] = D.static_depth[so];
            if (out.mask) out.mask[o] = D.static_mask[so];
            continue;
        }
        unsigned char c3[3]; int m;
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 64)
        shade_pixel(ctx, load_tri_rec(D, RM.first_dynamic_tri), px, row0 + lrow, c3, m);      // (probe: ONE record for everybody, a uniform address: scalar loads, no vector-memory work for the records)
#elif defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 4)
        shade_pixel(ctx, load_tri_rec(D, t & 63), px, row0 + lrow, c3, m);      // (probe: 64 records for everybody -- one cache line set)
#else
#ifdef RR_RASTER_STATS
        const TriRec trr_ = load_tri_rec(D, t);
        if (g_shade_ablate & 0x10000) { asm volatile("" :: "v"(trr_.v[0].x), "v"(trr_.v[3].x), "v"(trr_.v[4].x)); SHM(4); }
        shade_pixel(ctx, trr_, px, row0 + lrow, c3, m);
        if (g_shade_ablate & 0x10000) { asm volatile("" :: "v"((int)c3[0]), "v"(m)); SHM(5); }
#else
        shade_pixel(ctx, load_tri_rec(D, t), px, row0 + lrow, c3, m);
#endif
#endif
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 16)
        {   // (probe: +128 VALU instructions per shaded fragment batch, four independent chains -- does the kernel follow its VALU count?)
            float pv0 = (float)c3[0], pv1 = (float)c3[1], pv2 = (float)c3[2], pv3 = (float)m;
#pragma unroll
            for (int i_ = 0; i_ < 32; i_++) { pv0 = __builtin_fmaf(pv0, 1.0001f, 0.5f); pv1 = __builtin_fmaf(pv1, 1.0001f, 0.5f); pv2 = __builtin_fmaf(pv2, 1.0001f, 0.5f); pv3 = __builtin_fmaf(pv3, 1.0001f, 0.5f); }
            if (pv0 + pv1 + pv2 + pv3 == 12345.678f) m = 0;
        }
#endif
        const size_t o = ebase + gp;
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 1)
        if (c3[0] == 1 && c3[1] == 2 && c3[2] == 3 && m == 12345) out.depth[o] = 0.0f;      // (probe: no image stores)
#else
        out.rgb[o * 3] = c3[0]; out.rgb[o * 3 + 1] = c3[1]; out.rgb[o * 3 + 2] = c3[2];
        out.depth[o] = __uint_as_float(f.x);
        if (out.mask) out.mask[o] = m;
#endif
        SHM(6);
        first_ = false;
    }
}
// Measured in round 4 and dropped (k_shade alone, 4096 envs, 0.103 ms as it stands): the first list entry requested together with the
// count and the triangle record together with the instance constants (three dependent round trips instead of five): 0.104 ms;
// cooperative record loads -- eight lanes per 128-byte record, one load instruction covering eight records in eight cache
// lines instead of 64, transposed through 14 KB of LDS: 0.101 ms; one 512-thread workgroup per env walking the concatenation
// of its tile lists (4 096 workgroups instead of 32 768, instance constants staged once per env): 0.120 ms.
// order_n > 0: the launch has one more column of workgroups (blockIdx.x == order_n = the number of envs), which make the dispatch
// order of the next frame's k_raster from the costs the last one has left (dispatch_order_class, eight classes).
__global__ void __launch_bounds__(SHADE_THREADS) k_shade(const RenderModel *RMp, DevPtrs D, ImageOut out, int use_flags, int env0, int sel, int order_n, unsigned *order_perm) {
    __shared__ __attribute__((aligned(16))) float mvp[MAXINST][16];
    __shared__ __attribute__((aligned(16))) float sinst[MAXINST][16];
#if defined(RR_SHADE_PROBE) && (RR_SHADE_PROBE & 32)
    volatile __shared__ float occ_pad[RR_SHADE_PAD / 4];      // (probe: fewer workgroups per CU -- is the kernel bound by latency or by a per-CU rate?)
    occ_pad[threadIdx.x + (RR_SHADE_PAD / 4 - SHADE_THREADS)] = 1.0f;
#endif
    if (order_n > 0 && (int)blockIdx.x == order_n) {
        const int nt = RMp->ntiles, per_class = ((order_n + 7) >> 3) * nt;
        for (int x = blockIdx.z * gridDim.y + blockIdx.y; x < 8; x += gridDim.y * gridDim.z) dispatch_order_class<SHADE_THREADS>(x, order_n, nt, per_class, D.item_cost, D.item_bin, order_perm);
        return;
    }
    const int env = blockIdx.x + env0, tile = blockIdx.y;
    if (use_flags && D.render_flags && !D.render_flags[env]) return;
    if (!env_selected(D.hgflag, env, sel)) return;
#ifdef RR_RASTER_STATS
    unsigned long long wt0_ = 0;      // (workgroup timeline of the shading: rr_debug_shade_ablate(0x10000), scratch/rwgtime.py shade)
    if (g_shade_ablate & 0x10000) wt0_ = __builtin_amdgcn_s_memrealtime();
#endif
    shade_block<SHADE_THREADS>(*RMp, D, out, env, tile, blockIdx.z, gridDim.z, mvp, sinst);
#ifdef RR_RASTER_STATS
    if ((g_shade_ablate & 0x10000) && threadIdx.x == 0) {
        unsigned long long *g = g_rwg_time[((env * RMp->ntiles + tile) * gridDim.z + blockIdx.z) & 65535];
        g[0] = wt0_; g[1] = __builtin_amdgcn_s_memrealtime();
        g[2] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11)) << 32);
    }
#endif
}
// (Visibility pass and shading of a tile in one workgroup -- k_render_list's body for every env, 64 VGPRs, same LDS -- was
// measured: 0.470 ms instead of 0.383 + 0.097 alone, but 0.739 instead of 0.725 ms for the step: the heavy lists' render
// only gets onto the machine when this launch drains, 100 us later than behind the plain visibility pass.)
// The render of the heavy envs (D.hlist, D.hcount -- known on the device only), which follows their solve on the side stream
// and is the tail of the step's longest chain: ONE launch instead of three.  A fixed number of workgroups walk the list of
// (env, tile) items (dynamic assignment: tiles differ a lot in cost; no LDS-filling workgroup is launched just to find that
// its env is not on the list); for each item: the env's instance matrices (22 threads; the four tiles of an env write the
// same values), the visibility pass of the tile, the shading of its fragment list.
// (launched with at most RENDER_LIST_WGS workgroups, rr_plan.inc: two resident per CU)
template <int NT_>
__device__ __forceinline__ void render_list_body(const BodyParams &B, const SimParams &P, const RenderModel *RMp, const DevPtrs &D, const ImageOut &out, int n_inst_used, int restore, int which, int setup_done) {
    const RenderModel &RM = *RMp;
    int *hcount = which ? D.hcount2 : D.hcount;
    const int *hlist = which ? D.hlist2 : D.hlist;
    static_assert(TILE_PIX * 8 >= 2 * MAXINST * 16 * 4, "the shading constants are staged in the visibility buffer");
    float (*smvp)[16] = (float (*)[16])g_vis;                      // (the buffer is dead once raster_tile has written the list)
    float (*sinst)[16] = (float (*)[16])((float *)g_vis + MAXINST * 16);
    const int nitems = hcount[0] * RM.ntiles;
    __shared__ int s_item;
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(&hcount[1], 1);
        __syncthreads();
        const int it = s_item;
        if (it >= nitems) break;
        const int tile = it % RM.ntiles, env = hlist[it / RM.ntiles];
        if (env < P.N && !(D.render_flags && !D.render_flags[env])) {
            if (!setup_done) {          // (setup_done: the env's solve kernel has left its instance constants, solve_body)
                if ((int)threadIdx.x < RM.ni) instance_setup(B, P, RM, D, env, threadIdx.x);
                __threadfence_block();
                __syncthreads();
            }
            raster_tile<NT_, true, true>(P, RM, D, n_inst_used, 0, env, tile, restore);
            __threadfence_block();      // the fragment list and its count, written by this workgroup, are read back below
            __syncthreads();
            shade_block<NT_>(RM, D, out, env, tile, 0, 1, smvp, sinst);
        }
        __syncthreads();        // the LDS of the tile and the staging arrays are reused
    }
}
#ifndef RENDER_LIST_WAVES
#define RENDER_LIST_WAVES 4
#endif
__global__ void __launch_bounds__(RASTER_THREADS) __attribute__((amdgpu_waves_per_eu(RENDER_LIST_WAVES, 8)))
k_render_list(BodyParams B, SimParams P, const RenderModel *RMp, DevPtrs D, ImageOut out, int n_inst_used, int restore, int which, int setup_done) {
    render_list_body<RASTER_THREADS>(B, P, RMp, D, out, n_inst_used, restore, which, setup_done);
}
// (The same with 256 threads -- the footprint of one raster workgroup, so that it moves into the hole a retiring raster
// workgroup leaves -- was measured: 0.762 ms with the heavy list, 0.788 with both, instead of 0.727: an item takes twice as
// long and the visibility pass of the light envs loses as much as the lists gain.)
