// rr_dist.inc -- part of realrobot.hip (included there, behind rr_ray.inc; not a stand-alone translation unit).
// k_closest_points: Q pairs of collision shapes per env of the whole batch, the distance and the closest points of the two convex
// hulls at the present state (rr_closest_points, realrobot.h) -- pybullet's getClosestPoints for two links.  Read-only on the
// simulation (it reads D.state, the model constants and the pair table, never the preparation record); launched by
// rr_closest_points alone, never by a step.  The shape data is the device copy k_collide reads (D.shapes); a shape is the convex
// hull of its VERTEX set verts[s][0 .. nv), not of its planes.
//
// DIST_ENVS envs (one) per 256-thread workgroup, ONE WAVE64 PER (env, pair): item i of the workgroup is pair i / DIST_ENVS of env
// i % DIST_ENVS, wave w takes the items w, w + 4, ...  Phases 1 and 2 are k_ray_cast's (dist_stage_frames: the step's frames in LDS).
// Per item, all 64 lanes (dist_pair):
//   a  the two shapes' frames from LDS; the bounding-sphere gap, and with a cull the status-2 record;
//   b  lane l takes the vertices l, l + 64, l + 128 of A and of B, once, into registers: turned into the world ABOUT THE SHAPE'S
//      SPHERE CENTRE, R (x - c_local), so that they keep the rounding of a shape-sized number; the centres' difference cc is carried
//      apart (a vertex index behind the shape's last repeats the last vertex: it can never win a tie, so no lane is masked);
//   c  GJK on the Minkowski difference A - B.  v is the point of the simplex nearest the origin.  A trip: the support vertices of
//      A along -v and of B along v -- each lane the first maximum of its three, then a butterfly of __shfl_xor over (value, index)
//      that prefers the larger value and, among equals, the LOWER index; the winner's coordinates come out of its lane by
//      v_readlane --; r = a_i - b_j, w = r + cc; the support plane gives the bound  v . w / |v| <= distance;  then the point of
//      conv(simplex + w) nearest the origin among the features that hold w (w; the segments to the <= 3 kept points, clamped; the
//      triangles with two of them where the origin projects strictly inside; the tetrahedron, which ends the search when it holds
//      the origin), candidates in this fixed order, a later one only when strictly nearer.  Points with weight 0 leave the simplex.
//      Every lane computes the same simplex step (the indices are made wave-uniform by v_readfirstlane).
// Plain float32, but for the squared norms |p|^2 of the candidates, |v|^2 and v . w, which are float64 sums of exact products of
// the float32 components: a sideways step of 1e-5 m at 0.25 m shortens |v|^2 by less than a float32 rounding, and with float32
// norms the search stopped that far beside the closest point (measured; DESIGN.md).
// It ends, status 0, when  |v|^2 - v . w <= DIST_EPS |v|^2  (the relative gap between distance and bound), when the support
// vertex pair is already in the simplex, or when the new point is not strictly nearer than v (rounding has been reached: the
// earlier v stays); status 1 when the tetrahedron holds the origin or |v| <= DIST_TOUCH; status 3 after DIST_ITER_CAP trips.
// Degenerate simplices are the rule here (coplanar vertices of table and shelf, cube faces parallel to the table): a segment of
// zero length and a triangle with sin^2 of its corner angle below 1e-10 offer no candidate of their own (their sub-features do),
// a tetrahedron flatter than 1e-6 of its edges' product is never "inside" (its faces decide).  Whatever candidate wins is a point
// of the simplex, so |v| is an upper bound of the distance at every trip and never grows.  Edges of the simplex are differences
// of the r, in which cc cancels: a small face seen from a metre away keeps its normal to the rounding of its own size (with world
// vertices the closest vector of far pairs was off sideways by up to 1e-5 m; measured, DESIGN.md).
// Loop bounds are constants (3 vertex trips, 6 butterfly steps, DIST_ITER_CAP); no atomics; the result is a function of (state,
// table) alone and does not depend on N, the env's place in the batch or its neighbours.  No state value forms an address: vertex
// indices come out of compares over lane numbers.
#ifndef DIST_ENVS
#define DIST_ENVS 1          // envs per workgroup: its four waves share the env's frames and take every fourth pair (2, 4 and 8 were measured: DESIGN.md)
#endif
#define DIST_THREADS 256
#define DIST_WAVES (DIST_THREADS / 64)
#define DIST_TRIPS 3         // vertex registers per lane and shape: 64 * 3 = VMAXC
#define DIST_ITER_CAP 32     // GJK trips per pair at most (status 3 behind them)
#define DIST_EPS 1e-12f      // relative gap (|v|^2 - v . w) / |v|^2 that ends the search: distance - lower bound <= DIST_EPS distance (the float32 columns show it only down to rounding)
#define DIST_TOUCH 1e-6f     // m: a distance at or below this is "touching" (status 1): below the rounding of world coordinates

// the device copy of the handle's pair table (rr_set_distance_pairs)
struct DistTable { int a[RR_DIST_MAX], b[RR_DIST_MAX]; float max_distance; };

// Phases 1 and 2 of k_ray_cast restated (its operations in its order; sharing one function with that kernel changed its instructions,
// so it keeps its own text): the 32 state floats of the ENVS envs from env0 on into s_st, then the step's body frames into s_fr and
// the objects' frames into s_ob (the layouts of rr_ray.inc: RAY_ST, RAY_FR, RAY_FR_P); a barrier behind each phase (every thread of
// the workgroup calls this; an env behind the batch's end reads the last env's state)
template <int ENVS, int THREADS>
__device__ __forceinline__ void dist_stage_frames(const BodyParams &B, const DevPtrs &D, const int N, const int env0, const int tid,
                                                 float (*s_st)[ENVS], float (*s_fr)[RAY_FR], float (*s_ob)[12 * NOBJ + 1]) {
    static_assert(ST_OPOS == 2 * NB && ST_OQUAT == ST_OPOS + 3 * NOBJ, "staged slot s is state slot s (s < 11) or s + 11: positions and quaternions are one run");
    static_assert(THREADS >= 4 * ENVS, "phase 2: a thread per env and per (env, object)");
    // 1
    for (int i = tid; i < RAY_ST * ENVS; i += THREADS) {
        const int s = i / ENVS, e = i % ENVS;
        s_st[s][e] = D.state[(size_t)(s < NB ? s : s + NB) * N + min(env0 + e, N - 1)];
    }
    __syncthreads();
    // 2
    if (tid < ENVS) {
        // k_kinematics' phase 2 restated (the nc:: twins, det_sincosf: the floats of the step's forward kinematics), without the axes
        float *fr = s_fr[tid];
        for (int b = 0; b < NB; b++) {
            const int p = PARENT[b];
            m3 Rp = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
            v3 pp = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]);
            if (p >= 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) Rp.m[k] = fr[9 * p + k];
                pp = mk(fr[RAY_FR_P + 3 * p], fr[RAY_FR_P + 3 * p + 1], fr[RAY_FR_P + 3 * p + 2]);
            }
            m3 jr;
#pragma unroll
            for (int k = 0; k < 9; k++) jr.m[k] = B.jrot[b][k];
            const m3 Rj = nc::mul(Rp, jr);
            const v3 ax = mk(B.axis[b][0], B.axis[b][1], B.axis[b][2]);
            const v3 pb = nc::add(pp, nc::mulv(Rp, mk(B.jpos[b][0], B.jpos[b][1], B.jpos[b][2])));
            const m3 Rb = nc::mul(Rj, nc::axis_angle(ax, s_st[ST_Q + b][tid]));
#pragma unroll
            for (int k = 0; k < 9; k++) fr[9 * b + k] = Rb.m[k];
            fr[RAY_FR_P + 3 * b] = pb.x; fr[RAY_FR_P + 3 * b + 1] = pb.y; fr[RAY_FR_P + 3 * b + 2] = pb.z;
        }
    } else if (tid < 4 * ENVS) {
        const int e = (tid - ENVS) / NOBJ, o = (tid - ENVS) % NOBJ;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][e], s_st[21 + 4 * o][e], s_st[22 + 4 * o][e], s_st[23 + 4 * o][e]);
        float *ob = s_ob[e] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][e]; ob[10] = s_st[12 + 3 * o][e]; ob[11] = s_st[13 + 3 * o][e];
    }
    __syncthreads();
}

// first maximum of dot(x[t], d) over the vertices of the wave: the lowest vertex index among equal values, uniform in the wave
__device__ __forceinline__ int dist_support(const v3 *x, const v3 d, const int lane) {
    float best = dot(x[0], d);
    int bi = lane;
#pragma unroll
    for (int t = 1; t < DIST_TRIPS; t++) {
        const float s = dot(x[t], d);
        const bool g = s > best;
        best = g ? s : best;
        bi = g ? 64 * t + lane : bi;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float ov = __shfl_xor(best, m);
        const int oi = __shfl_xor(bi, m);
        const bool take = ov > best || (ov == best && oi < bi);
        best = take ? ov : best;
        bi = take ? oi : bi;
    }
    return min(max(__builtin_amdgcn_readfirstlane(bi), 0), 64 * DIST_TRIPS - 1);
}

// vertex idx (uniform) out of the lane that holds it
__device__ __forceinline__ v3 dist_fetch(const v3 x0, const v3 x1, const v3 x2, const int idx) {       // (by value: a select between loads would index the array)
    const int t = idx >> 6, l = idx & 63;
    const v3 s = mk(t == 0 ? x0.x : (t == 1 ? x1.x : x2.x), t == 0 ? x0.y : (t == 1 ? x1.y : x2.y), t == 0 ? x0.z : (t == 1 ? x1.z : x2.z));
    return mk(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.x), l)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.y), l)),
              __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.z), l)));
}

// a . b with exact products and sums in float64: squared norms and the gap are compared below the rounding of a float32 square
__device__ __forceinline__ double dist_ddot(const v3 a, const v3 b) { return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z; }
__device__ __forceinline__ float dist_det(const v3 a, const v3 b, const v3 c) { return dot(a, cross(b, c)); }

// One pair of the table for the 64 lanes of one wave: steps a to c of the header, the text that k_closest_points and
// k_posture_clearance (rr_posture.inc) both run; it returns the record's three float4, status, trips and the owners of the two
// shapes, the same values in every lane.  (k_signed_distance keeps a copy of its own, sd_pair: rr_signed.inc says why.)
struct DistItem { float4 o0, o1, o2; int status, iters, ota, oia, otb, oib; };
__device__ __forceinline__ DistItem dist_pair(const ShapeData *__restrict__ S, const DistTable *__restrict__ tab, const int j, const float *fr, const float *ob,
                                                const bool cull, const float maxd, const int lane) {
    // a.  (The table is validated by rr_set_distance_pairs; the clamps only keep the model's tables in range.)
    const int sa = min(max(__builtin_amdgcn_readfirstlane(tab->a[j]), 0), MAXSHAPES - 1), sb = min(max(__builtin_amdgcn_readfirstlane(tab->b[j]), 0), MAXSHAPES - 1);
    const int ota = S->otype[sa], otb = S->otype[sb];
    const int oia = min(max(S->oidx[sa], 0), ota == 2 ? NOBJ - 1 : NB - 1), oib = min(max(S->oidx[sb], 0), otb == 2 ? NOBJ - 1 : NB - 1);
    m3 Ra, Rb; v3 pa, pb;
    ray_shape_frame(ota, oia, fr, ob, &Ra, &pa);
    ray_shape_frame(otb, oib, fr, ob, &Rb, &pb);
    const v3 sca = mk(S->sphere[sa][0], S->sphere[sa][1], S->sphere[sa][2]), scb = mk(S->sphere[sb][0], S->sphere[sb][1], S->sphere[sb][2]);
    const v3 ca = mulv(Ra, sca) + pa, cb = mulv(Rb, scb) + pb;
    const float ra = S->sphere[sa][3], rb = S->sphere[sb][3];
    const v3 cc = ca - cb;
    const float cn = sqrtf(dot(cc, cc));
    const float gap = cn - ra - rb;
    float4 o0, o1, o2;
    int status, iters = 0;
    if (cull && gap > maxd) {
        const v3 u = cc * (1.0f / cn);
        const v3 xa = ca - u * ra, xb = cb + u * rb;
        status = 2;
        o0 = make_float4(gap, gap, xa.x, xa.y); o1 = make_float4(xa.z, xb.x, xb.y, xb.z); o2 = make_float4(u.x, u.y, u.z, 0.0f);
    } else {
        // b
        v3 xa[DIST_TRIPS], xb[DIST_TRIPS];
        const int nva = min(max(S->nv[sa], 1), VMAXC), nvb = min(max(S->nv[sb], 1), VMAXC);
#pragma unroll
        for (int t = 0; t < DIST_TRIPS; t++) {
            const int ka = min(64 * t + lane, nva - 1), kb = min(64 * t + lane, nvb - 1);
            xa[t] = mulv(Ra, mk(S->verts[sa][ka][0], S->verts[sa][ka][1], S->verts[sa][ka][2]) - sca);
            xb[t] = mulv(Rb, mk(S->verts[sb][kb][0], S->verts[sb][kb][1], S->verts[sb][kb][2]) - scb);
        }
        // c.  The simplex: three slots {r = a - b about the centres (the point is r + cc), a, b, the two vertex indices, weight}; weight 0: the slot is free.
        v3 sr[3], sA[3], sB[3];
        int ia[3], ib[3];
        float lam[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 3; k++) { sr[k] = sA[k] = sB[k] = mk(0.0f, 0.0f, 0.0f); ia[k] = ib[k] = -1; }
        v3 v = cn > 0.0f ? cc : mk(1.0f, 0.0f, 0.0f);             // the first direction: between the sphere centres (no point of the simplex yet)
        double vv = INFINITY;
        float lower = 0.0f;
        status = 3;
        for (int it = 0; it < DIST_ITER_CAP; it++) {
            iters = it + 1;
            const int ja = dist_support(xa, v * -1.0f, lane), jb = dist_support(xb, v, lane);
            const v3 wa = dist_fetch(xa[0], xa[1], xa[2], ja), wb = dist_fetch(xb[0], xb[1], xb[2], jb);
            const v3 r = wa - wb, w = r + cc;
            const double vw = dist_ddot(v, w);
            const float vn = sqrtf(dot(v, v));
            if (vn > 0.0f) lower = fmaxf(lower, (float)vw / vn);
            bool stop = false;
            if (it > 0) {
                bool dup = false;
#pragma unroll
                for (int k = 0; k < 3; k++) dup = dup || (lam[k] > 0.0f && ia[k] == ja && ib[k] == jb);
                stop = dup || vv - vw <= (double)DIST_EPS * vv;
            }
            if (__builtin_amdgcn_readfirstlane(stop)) { status = 0; break; }
            // the nearest point of the features that hold w: weights l[0..2] of the slots and lw of w
            float l[3] = {0.0f, 0.0f, 0.0f}, lw = 1.0f;
            v3 nv = w;
            double nvv = dist_ddot(w, w);
#pragma unroll
            for (int k = 0; k < 3; k++) {                           // segments w -- slot k
                const v3 d = sr[k] - r;
                const float dd = dot(d, d);
                const float t = fminf(fmaxf(-dot(w, d) / dd, 0.0f), 1.0f);
                const v3 p = w + d * t;
                const double pp = dist_ddot(p, p);
                if (lam[k] > 0.0f && dd > 0.0f && pp < nvv) {
                    nvv = pp; nv = p; lw = 1.0f - t;
                    l[0] = l[1] = l[2] = 0.0f; l[k] = t;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {                           // triangles w, slot f, slot g: (0, 1), (1, 2), (2, 0)
                const int f = k, g = (k + 1) % 3;
                const v3 ab = sr[f] - r, ac = sr[g] - r, wf = sr[f] + cc, wg = sr[g] + cc;
                const float d1 = -dot(ab, w), d2 = -dot(ac, w), d3 = -dot(ab, wf), d4 = -dot(ac, wf), d5 = -dot(ab, wg), d6 = -dot(ac, wg);
                const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
                const v3 n = cross(ab, ac);
                const float nn = dot(n, n);
                const v3 p = n * (dot(n, w) / nn);
                const double pp = dist_ddot(p, p);
                const bool in = lam[f] > 0.0f && lam[g] > 0.0f && va > 0.0f && vb > 0.0f && vc > 0.0f && nn > 1e-10f * dot(ab, ab) * dot(ac, ac);
                if (in && pp < nvv) {
                    const float q = 1.0f / (va + vb + vc);
                    nvv = pp; nv = p; lw = va * q;
                    l[0] = l[1] = l[2] = 0.0f; l[f] = vb * q; l[g] = vc * q;
                }
            }
            bool inside = false;
            if (lam[0] > 0.0f && lam[1] > 0.0f && lam[2] > 0.0f) {  // the tetrahedron slot 0, 1, 2, w
                const v3 a = sr[0] + cc, ab = sr[1] - sr[0], ac = sr[2] - sr[0], ad = r - sr[0];
                const float V = dist_det(ab, ac, ad);
                const float La = dist_det(sr[1] + cc, sr[2] + cc, w), Lb = dist_det(a * -1.0f, ac, ad), Lc = dist_det(ab, a * -1.0f, ad), Ld = dist_det(ab, ac, a * -1.0f);
                const float sg = V > 0.0f ? 1.0f : -1.0f;
                inside = fabsf(V) > 1e-6f * sqrtf(dot(ab, ab) * dot(ac, ac) * dot(ad, ad)) && La * sg >= 0.0f && Lb * sg >= 0.0f && Lc * sg >= 0.0f && Ld * sg >= 0.0f;
            }
            if (__builtin_amdgcn_readfirstlane(inside)) { status = 1; break; }
            if (__builtin_amdgcn_readfirstlane(it > 0 && !(nvv < vv))) { status = 0; break; }     // not strictly nearer: v stays
            // w into the first free slot
            bool placed = false;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const bool here = !placed && !(l[k] > 0.0f);
                if (here) { sr[k] = r; sA[k] = wa; sB[k] = wb; ia[k] = ja; ib[k] = jb; }
                lam[k] = here ? lw : l[k];
                placed = placed || here;
            }
            v = nv; vv = nvv;
            if (__builtin_amdgcn_readfirstlane(vv <= (double)DIST_TOUCH * DIST_TOUCH)) { status = 1; break; }
        }
        v3 xA = mk(0.0f, 0.0f, 0.0f), xB = xA;                  // the weighted vertices about the centres, then the centres
#pragma unroll
        for (int k = 0; k < 3; k++) { xA = xA + sA[k] * lam[k]; xB = xB + sB[k] * lam[k]; }
        xA = xA + ca; xB = xB + cb;
        if (status == 1) {
            o0 = make_float4(0.0f, 0.0f, xA.x, xA.y); o1 = make_float4(xA.z, xA.x, xA.y, xA.z); o2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            const float dist = sqrtf((float)vv);
            const v3 n = v * (1.0f / dist);
            o0 = make_float4(dist, fminf(lower, dist), xA.x, xA.y); o1 = make_float4(xA.z, xB.x, xB.y, xB.z); o2 = make_float4(n.x, n.y, n.z, 0.0f);
        }
    }
    DistItem R;
    R.o0 = o0; R.o1 = o1; R.o2 = o2; R.status = status; R.iters = iters; R.ota = ota; R.oia = oia; R.otb = otb; R.oib = oib;
    return R;
}

__global__ void __launch_bounds__(DIST_THREADS) k_closest_points(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                 float4 *__restrict__ out_pts /*[N][Q][3]*/, int4 *__restrict__ out_id /*[N][Q]*/) {
    static_assert(64 * DIST_TRIPS == VMAXC && DIST_ENVS <= DIST_WAVES * 64 / 4, "a lane holds three vertices of a shape; dist_stage_frames' threads");
    __shared__ float s_st[RAY_ST][DIST_ENVS];
    __shared__ float s_fr[DIST_ENVS][RAY_FR];
    __shared__ float s_ob[DIST_ENVS][12 * NOBJ + 1];
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int env0 = blockIdx.x * DIST_ENVS;
    dist_stage_frames<DIST_ENVS, DIST_THREADS>(B, D, N, env0, tid, s_st, s_fr, s_ob);
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    const int items = DIST_ENVS * Q;
    for (int i = wave; i < items; i += DIST_WAVES) {
        const int e = i % DIST_ENVS, j = i / DIST_ENVS, env = env0 + e;
        if (env >= N) continue;                                                                 // (uniform in the wave)
        const DistItem R = dist_pair(S, tab, j, s_fr[e], s_ob[e], cull, maxd, lane);
        if (lane == 0) {
            const size_t r = (size_t)env * Q + j;
            out_pts[3 * r] = R.o0; out_pts[3 * r + 1] = R.o1; out_pts[3 * r + 2] = R.o2;
            out_id[r] = make_int4(R.status, R.iters, R.ota == 0 ? -1 : (R.ota == 1 ? R.oia : 16 + R.oia), R.otb == 0 ? -1 : (R.otb == 1 ? R.oib : 16 + R.oib));
        }
    }
}
