// rr_posture.inc -- part of realrobot.hip (included there, behind rr_dist.inc; not a stand-alone translation unit).
// k_posture_clearance: the clearance of K candidate joint postures per env of the whole batch (rr_posture_clearance, realrobot.h):
// posture (e, k) is env e's present state with its eleven joint columns taken from the caller's tensor, the objects where they are;
// per posture the distance and status of every pair of the table (rr_set_distance_pairs) and the full record of the NEAREST pair,
// reduced on the device.  Read-only on the simulation (D.state's object columns, the model constants, the pair table and the
// tensor; never the preparation record); launched by rr_posture_clearance alone, never by a step.
//
// One 256-thread workgroup per (env, posture), grid N * K exactly; its four waves take every fourth pair, ONE WAVE64 PER PAIR, and a
// pair is steps a to c of rr_dist.inc's header (cull, vertices about the sphere centre, GJK with float64 norms), RESTATED here as
// pc_pair.  Moving those steps into one inline function used by both kernels was tried first: k_closest_points then compiled to other
// instructions (another scalar register allocation and three more lines), so by the project's standing rule rr_dist.inc keeps its text
// untouched and this file carries a copy.  The two kernels may therefore contract differently; the tests measure it.
//   1  the 32 staged floats into LDS: slots 0..10 from the posture's 44-byte row of the tensor, 11..31 (object positions and
//      quaternions) from D.state;
//   2  the rolled forward kinematics on one lane and the object rotations on three -- dist_stage_frames' phase 2 restated (the nc::
//      twins in the step's order), that function reads its joints from D.state;
//   3  per pair, lane 0 stores the distance and the status word {status, iterations << 8}; the wave carries its best pair so far in
//      wave-uniform registers (v_readfirstlane: scalar registers) -- the key, j, the record's three float4, status and bodies --,
//      taken when the distance is strictly below the key, over ascending j.  The key starts at +inf and the record at the wave's
//      first pair, so a NaN distance never displaces a number and a wave always has a record;
//   4  lane 0 of each wave parks its best in LDS; behind one barrier thread 0 picks over the waves that had a pair by (key, j) --
//      the first minimum of the row -- and writes RR_PC_NEAREST / RR_PC_ID.  Every wave reaches the barrier: the grid is exact and
//      the pair loop has no early exit.
// No atomics, fixed order: row (e, k) is a function of (env e's objects, posture (e, k), the table) alone.  Loop bounds are
// constants or Q; no value of the tensor or the state forms an address.
#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / 64)
#define PC_PARK 20           // floats a wave parks: the record 0..11, key 12, j 13, status 14, body A 15, body B 16

__device__ __forceinline__ float pc_uniform(const float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ float4 pc_uniform(const float4 x) { return make_float4(pc_uniform(x.x), pc_uniform(x.y), pc_uniform(x.z), pc_uniform(x.w)); }

// One pair of the table for the 64 lanes of one wave: steps a to c of k_closest_points RESTATED, its operations in its order (the
// helpers dist_support, dist_fetch, dist_ddot, dist_det and ray_shape_frame are that file's own); it returns the record's three
// float4, status, trips and the owners of the two shapes, the same values in every lane.
struct PcItem { float4 o0, o1, o2; int status, iters, ota, oia, otb, oib; };
__device__ __forceinline__ PcItem pc_pair(const ShapeData *__restrict__ S, const DistTable *__restrict__ tab, const int j, const float *fr, const float *ob,
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
    PcItem R;
    R.o0 = o0; R.o1 = o1; R.o2 = o2; R.status = status; R.iters = iters; R.ota = ota; R.oia = oia; R.otb = otb; R.oib = oib;
    return R;
}

__global__ void __launch_bounds__(PC_THREADS) k_posture_clearance(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                  const float *__restrict__ postures /*[N][K][11]*/, int K,
                                                                  float4 *__restrict__ out_near /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                  float *__restrict__ out_dist /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/) {
    static_assert(RAY_ST == 32 && NB == 11 && ST_OPOS == 2 * NB, "staged slot s is the posture's column s (s < 11) or state slot s + 11");
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][RAY_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    __shared__ float s_best[PC_WAVES][PC_PARK];
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row = blockIdx.x;                                    // e * K + k
    const int env = min((int)(row / (size_t)K), N - 1);
    // 1
    if (tid < RAY_ST) s_st[tid][0] = tid < NB ? postures[row * NB + tid] : D.state[(size_t)(tid + NB) * N + env];
    __syncthreads();
    // 2
    if (tid == 0) {
        float *fr = s_fr[0];
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
            const m3 Rb = nc::mul(Rj, nc::axis_angle(ax, s_st[ST_Q + b][0]));
#pragma unroll
            for (int k = 0; k < 9; k++) fr[9 * b + k] = Rb.m[k];
            fr[RAY_FR_P + 3 * b] = pb.x; fr[RAY_FR_P + 3 * b + 1] = pb.y; fr[RAY_FR_P + 3 * b + 2] = pb.z;
        }
    } else if (tid < 1 + NOBJ) {
        const int o = tid - 1;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][0], s_st[21 + 4 * o][0], s_st[22 + 4 * o][0], s_st[23 + 4 * o][0]);
        float *ob = s_ob[0] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][0]; ob[10] = s_st[12 + 3 * o][0]; ob[11] = s_st[13 + 3 * o][0];
    }
    __syncthreads();
    // 3
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    float key = INFINITY;
    int bj = wave, bst = 0, ba = -1, bb = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0, b2 = b0;
    for (int j = wave; j < Q; j += PC_WAVES) {
        const PcItem R = pc_pair(S, tab, j, s_fr[0], s_ob[0], cull, maxd, lane);
        if (lane == 0) {
            out_dist[row * Q + j] = R.o0.x;
            out_status[row * Q + j] = (R.status & 255) | ((R.iters & 255) << 8);
        }
        const float d = pc_uniform(R.o0.x);
        const bool nearer = d < key;
        if (nearer || j == wave) {                                      // (uniform in the wave)
            bj = j; bst = __builtin_amdgcn_readfirstlane(R.status);
            ba = __builtin_amdgcn_readfirstlane(R.ota == 0 ? -1 : (R.ota == 1 ? R.oia : 16 + R.oia));
            bb = __builtin_amdgcn_readfirstlane(R.otb == 0 ? -1 : (R.otb == 1 ? R.oib : 16 + R.oib));
            b0 = pc_uniform(R.o0); b1 = pc_uniform(R.o1); b2 = pc_uniform(R.o2);
        }
        key = nearer ? d : key;
    }
    // 4
    if (lane == 0) {
        float *w = s_best[wave];
        w[0] = b0.x; w[1] = b0.y; w[2] = b0.z; w[3] = b0.w; w[4] = b1.x; w[5] = b1.y; w[6] = b1.z; w[7] = b1.w;
        w[8] = b2.x; w[9] = b2.y; w[10] = b2.z; w[11] = b2.w;
        w[12] = key; w[13] = __int_as_float(bj); w[14] = __int_as_float(bst); w[15] = __int_as_float(ba); w[16] = __int_as_float(bb);
    }
    __syncthreads();
    if (tid == 0) {
        int win = 0;
        for (int w = 1; w < PC_WAVES; w++) {
            const bool lower = s_best[w][12] < s_best[win][12] ||
                               (s_best[w][12] == s_best[win][12] && __float_as_int(s_best[w][13]) < __float_as_int(s_best[win][13]));
            win = (w < Q && lower) ? w : win;                               // a wave behind the table's end had no pair
        }
        const float *w = s_best[win];
        out_near[3 * row] = make_float4(w[0], w[1], w[2], w[3]);
        out_near[3 * row + 1] = make_float4(w[4], w[5], w[6], w[7]);
        out_near[3 * row + 2] = make_float4(w[8], w[9], w[10], w[11]);
        out_id[row] = make_int4(__float_as_int(w[14]), __float_as_int(w[13]), __float_as_int(w[15]), __float_as_int(w[16]));
    }
}
