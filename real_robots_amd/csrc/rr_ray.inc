// rr_ray.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_ray_cast: R segments per env of the whole batch against the model's convex collision hulls at the present state (rr_ray_cast,
// realrobot.h) -- pybullet's rayTestBatch with parentLinkIndex: what does this segment hit first, where, with which normal.
// Read-only on the simulation (it reads D.state, the model constants, the ray table and the caller's segments, never the preparation
// record); launched by rr_ray_cast alone, never by a step.  The shape data is the device copy k_collide reads (D.shapes).
//
// RAY_ENVS envs per 256-thread workgroup, ONE LANE PER RAY (a wave per ray with lanes over planes was built and measured:
// DESIGN.md).  Four phases, a barrier behind each of the first two, every thread at every barrier (an env behind the batch's end
// reads the last env's state and stores nothing):
//   1  all threads: the 32 state floats the frames need -- q, object positions and quaternions -- of the workgroup's envs into LDS;
//   2  threads 0 .. RAY_ENVS-1: the forward kinematics of one env each, k_kinematics' loop (fk_all's operations in its order: the
//      step's body frames); the next 3 RAY_ENVS threads: an object's rotation from its quaternion as the step forms it;
//   3  lane i of pass p is ray (p * 256 + i) % R of env (p * 256 + i) / R: its link's COM frame (the expression of k_link_poses)
//      takes the segment into the world;
//   4  the lane walks the hulls.  The shape index s and the plane index k of the loops are uniform in the wave, so a shape's
//      constants and its planes come in by scalar loads and no lane's DATA steers the control flow: per shape the lane takes its
//      segment into the shape's frame (the frame of its own env, from LDS) and tests the segment against the bounding sphere; the
//      wave votes and skips the plane loop when no lane's segment comes near.  Inside the loop every lane clips against every
//      plane; a lane whose sphere test failed cannot accept (so a ray's result does not depend on its neighbours in the wave).
// A hull is {x : n_k . x - d_k <= 0}.  With o, d the segment's origin and direction in the hull's frame: t_in is the largest
// (n_k . o - d_k) / -(n_k . d) over the planes with n_k . d < 0 (first maximum: the lowest plane index among equals), t_out the
// smallest over those with n_k . d > 0; the hull is hit iff some plane has the origin strictly outside, no plane parallel to the
// segment has, 0 <= t_in <= min(t_out, 1).  The reciprocal is v_rcp_f32 (1 ulp).  Over the hulls the smallest float32 t_in wins, the
// lowest shape index among equals (strict compares in ascending order).  No atomics, no order between threads: the buffers are a
// function of (state, rays) alone.  Neither a ray value nor a state value ever forms an address.
#define RAY_ENVS 4           // envs per workgroup: with R = 64 one pass of four full waves, with R = 16 one wave (DESIGN.md has the alternatives measured)
#define RAY_UNROLL 8         // planes per trip of the plane loop
#define RAY_THREADS 256
#define RAY_ST 32            // staged state floats per env: q 0..10, object positions 11..19 and quaternions 20..31
#define RAY_FR 133           // floats of an env's body frames: R 0..98, p 99..131 (an odd stride: phase 2's lanes hit distinct banks)
#define RAY_FR_P 99
#define RAY_CULL_SLACK 1e-3f // m added to a bounding sphere's radius: the spheres bound the hulls' vertices, the planes were fitted within 0.3 mm of them

// the device copy of the handle's ray table (rr_set_rays), and the uid of every collision shape (the blob's shape_owner, column 3)
struct RayTable { int link[RR_RAY_MAX]; float seg[RR_RAY_MAX][6]; int uid[MAXSHAPES]; };

// world frame of collision shape s (owner kind ot, owner index oi) of the env whose body frames are fr and object frames ob
__device__ __forceinline__ void ray_shape_frame(int ot, int oi, const float *fr, const float *ob, m3 *R, v3 *p) {
    m3 I = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    *R = I; *p = mk(0.0f, 0.0f, 0.0f);
    if (ot == 1) {
#pragma unroll
        for (int k = 0; k < 9; k++) R->m[k] = fr[9 * oi + k];
        *p = mk(fr[RAY_FR_P + 3 * oi], fr[RAY_FR_P + 3 * oi + 1], fr[RAY_FR_P + 3 * oi + 2]);
    } else if (ot == 2) {
#pragma unroll
        for (int k = 0; k < 9; k++) R->m[k] = ob[12 * oi + k];
        *p = mk(ob[12 * oi + 9], ob[12 * oi + 10], ob[12 * oi + 11]);
    }
}

__global__ void __launch_bounds__(RAY_THREADS) k_ray_cast(BodyParams B, SimParams P, const RenderModel *RMp, DevPtrs D, int ns,
                                                         const RayTable *__restrict__ tab, const float *__restrict__ rays /*[N][R][6] or nullptr: the table's*/,
                                                         int R, float4 *__restrict__ out_hit /*[N][R][2]*/, int4 *__restrict__ out_id /*[N][R]*/) {
    static_assert(ST_OPOS == 2 * NB && ST_OQUAT == ST_OPOS + 3 * NOBJ, "staged slot s is state slot s (s < 11) or s + 11: positions and quaternions are one run");
    static_assert(RAY_THREADS >= 4 * RAY_ENVS, "phase 2: a thread per env and per (env, object)");
    __shared__ float s_st[RAY_ST][RAY_ENVS];
    __shared__ float s_fr[RAY_ENVS][RAY_FR];
    __shared__ float s_ob[RAY_ENVS][12 * NOBJ + 1];        // per object R (9), p (3)
    const RenderModel &RM = *RMp;
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x;
    const int env0 = blockIdx.x * RAY_ENVS;
    // 1
    for (int i = tid; i < RAY_ST * RAY_ENVS; i += RAY_THREADS) {
        const int s = i / RAY_ENVS, e = i % RAY_ENVS;
        s_st[s][e] = D.state[(size_t)(s < NB ? s : s + NB) * N + min(env0 + e, N - 1)];
    }
    __syncthreads();
    // 2
    if (tid < RAY_ENVS) {
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
    } else if (tid < 4 * RAY_ENVS) {
        const int e = (tid - RAY_ENVS) / NOBJ, o = (tid - RAY_ENVS) % NOBJ;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][e], s_st[21 + 4 * o][e], s_st[22 + 4 * o][e], s_st[23 + 4 * o][e]);
        float *ob = s_ob[e] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][e]; ob[10] = s_st[12 + 3 * o][e]; ob[11] = s_st[13 + 3 * o][e];
    }
    __syncthreads();
    // 3, 4
    const int items = RAY_ENVS * R;
    for (int i0 = 0; i0 < items; i0 += RAY_THREADS) {       // (uniform bounds: every lane of a wave takes every vote)
        const int i = min(i0 + tid, items - 1);
        const int e = i / R, j = i - e * R;
        const int env = env0 + e;
        const bool live = i0 + tid < items && env < N;
        const float *fr = s_fr[e], *ob = s_ob[e];
        // 3: the ray's frame.  (The link is validated by rr_set_rays; the clamps only keep the model's tables in range.)
        const int l = min(max(tab->link[j], -1), KIN_LINKS - 1);
        m3 Rl = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
        v3 pl = mk(0.0f, 0.0f, 0.0f);
        if (l >= 0) {
            const int b = min(RM.link_body[l], NB - 1);
            m3 lr;
#pragma unroll
            for (int k = 0; k < 9; k++) lr.m[k] = RM.link_rot[l][k];
            const v3 lp = mk(RM.link_pos[l][0], RM.link_pos[l][1], RM.link_pos[l][2]);
            Rl = lr;
            pl = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]) + lp;
            if (b >= 0) {
                m3 Rb;
#pragma unroll
                for (int k = 0; k < 9; k++) Rb.m[k] = fr[9 * b + k];
                Rl = mul(Rb, lr);
                pl = mulv(Rb, lp) + mk(fr[RAY_FR_P + 3 * b], fr[RAY_FR_P + 3 * b + 1], fr[RAY_FR_P + 3 * b + 2]);
            }
        }
        const float *seg = rays ? rays + ((size_t)min(env, N - 1) * R + j) * 6 : tab->seg[j];
        const v3 fw = mulv(Rl, mk(seg[0], seg[1], seg[2])) + pl;
        const v3 tw = mulv(Rl, mk(seg[3], seg[4], seg[5])) + pl;
        const v3 dw = tw - fw;
        const float len = sqrtf(dot(dw, dw));
        // a segment that can hit: finite (a NaN or an overflow anywhere fails the compare) and not of zero length
        const bool castable = live && (fabsf(fw.x) + fabsf(fw.y) + fabsf(fw.z) + len < INFINITY) && len > 0.0f;
        // 4
        float best_t = INFINITY;
        int best_s = -1, best_k = 0;
        for (int s = 0; s < ns; s++) {
            const int ot = S->otype[s], oi = S->oidx[s];
            // an object the handle does not have; an owner outside the frames (no model has one: the LDS index stays in range) -- uniform
            if ((ot == 2 && (unsigned)oi >= (unsigned)min(P.nobj, NOBJ)) || (ot == 1 && (unsigned)oi >= NB)) continue;
            m3 Rs; v3 ps;
            ray_shape_frame(ot, oi, fr, ob, &Rs, &ps);
            const v3 o = tmulv(Rs, fw - ps), d = tmulv(Rs, dw);
            const v3 m = mk(S->sphere[s][0], S->sphere[s][1], S->sphere[s][2]) - o;
            const float rad = S->sphere[s][3] + RAY_CULL_SLACK;
            const float tc = fminf(fmaxf(dot(m, d) * __builtin_amdgcn_rcpf(dot(d, d)), 0.0f), 1.0f);
            const v3 q = m - d * tc;
            const bool near = castable && dot(q, q) <= rad * rad;
            if (!__any(near)) continue;                                                            // the wave's vote
            const int nf = min(S->nf[s], FMAXC);
            float t_in = -INFINITY, t_out = INFINITY;
            int k_in = 0;
            bool outside = false, barred = false;
            // RAY_UNROLL planes per trip: their scalar loads are issued together, one wait for all (one plane per trip waits out the
            // scalar cache's latency 192 times a hull); the last nf % RAY_UNROLL planes one by one
            auto clip = [&](const float4 pk, const int k) {
                const float den = pk.x * d.x + pk.y * d.y + pk.z * d.z;
                const float dist = pk.x * o.x + pk.y * o.y + pk.z * o.z - pk.w;
                const float t = dist * __builtin_amdgcn_rcpf(-den);
                outside = outside || dist > 0.0f;
                barred = barred || (den == 0.0f && dist > 0.0f);
                const bool enter = den < 0.0f && t > t_in;
                t_in = enter ? t : t_in;
                k_in = enter ? k : k_in;
                t_out = den > 0.0f ? fminf(t_out, t) : t_out;
            };
            const float4 *__restrict__ pls = (const float4 *)S->planes[s];
            int k = 0;
            for (; k + RAY_UNROLL <= nf; k += RAY_UNROLL) {
                float4 pk[RAY_UNROLL];
#pragma unroll
                for (int u = 0; u < RAY_UNROLL; u++) pk[u] = pls[k + u];
#pragma unroll
                for (int u = 0; u < RAY_UNROLL; u++) clip(pk[u], k + u);
            }
            for (; k < nf; k++) clip(pls[k], k);
            const bool hit = near && outside && !barred && t_in >= 0.0f && t_in <= fminf(t_out, 1.0f) && t_in < best_t;
            best_t = hit ? t_in : best_t;
            best_s = hit ? s : best_s;
            best_k = hit ? k_in : best_k;
        }
        // the record.  (best_s, best_k: this lane's own indices, within [0, ns) x [0, nf) by construction.)
        float4 h0 = make_float4(1.0f, len, tw.x, tw.y), h1 = make_float4(tw.z, 0.0f, 0.0f, 0.0f);
        int4 id = make_int4(-1, -1, -1, -1);
        if (best_s >= 0) {
            const int ot = S->otype[best_s], oi = S->oidx[best_s];
            m3 Rs; v3 ps;
            ray_shape_frame(ot, oi, fr, ob, &Rs, &ps);
            const float4 pk = ((const float4 *)S->planes[best_s])[best_k];
            const v3 n = mulv(Rs, mk(pk.x, pk.y, pk.z));
            const v3 x = fw + dw * best_t;
            h0 = make_float4(best_t, best_t * len, x.x, x.y);
            h1 = make_float4(x.z, n.x, n.y, n.z);
            id = make_int4(tab->uid[best_s], ot == 0 ? -1 : (ot == 1 ? oi : 16 + oi), S->link[best_s], best_s);
        }
        if (live) {
            const size_t r = (size_t)env * R + j;
            out_hit[2 * r] = h0; out_hit[2 * r + 1] = h1;
            out_id[r] = id;
        }
    }
}
