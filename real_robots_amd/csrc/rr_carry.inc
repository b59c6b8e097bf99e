// rr_carry.inc -- part of realrobot.hip (included there, behind rr_grad.inc; not a stand-alone translation unit).
// Carried objects in the posture queries (rr_set_attachments, realrobot.h): an object declared rigid with a robot link is, at a candidate
// posture, where that link's forward kinematics puts it, and its shapes take the joint columns of that link in the gradient.  A
// query-side setting: nothing of the step reads the table.
//
// The table, [N][NOBJ][ATT_ROW] floats, holds per (env, object) the pose of the object's state frame in the frame of the MOVING BODY b
// its link hangs on -- R_rel row-major in floats 0..8, t_rel in 9..11 -- and in float 12 the integer b + 1, 0 for a free object: a
// zero-filled table is all free.  The host converts from and to the link's COM frame (rr_host.inc); no kernel here reads a link table.
//
// k_attach_set       the rows of the masked envs from a staged copy, one thread per float.
// k_attach_capture   rel = T_b(q_present)^-1 o T_object(present) for the attached objects of the masked envs: one 64-thread workgroup
//                    per env, dist_stage_frames (the step's frames of the present state, the nc:: twins in the step's order), then
//                    thread o < NOBJ: R_rel = R_b^T R_o, t_rel = R_b^T (p_o - p_b), contraction off.
// k_posture_clearance_carry, k_signed_distance_carry, k_signed_gradient_carry
//                    the three posture kernels with carried objects, launched in place of the originals while the handle's attachments
//                    are on (e->att_on).  Launch shape, staging, pair function (dist_pair / sd_pair: called), reduction, summation order
//                    and stores are the originals', whose text is restated here -- rr_posture.inc's header records that sharing a
//                    phase with another kernel once changed that kernel's scalar code, and the originals' instructions must not change
//                    (tools/compare_kernel_asm.py).  Two things differ:
//   phase 2  one more barrier: thread 0 rolls the forward kinematics, and BEHIND the barrier threads 1..NOBJ stage the objects
//            (carry_stage_object).  A free object by exactly the original's operations -- its bits are the original's --, an attached
//            one as R_o = R_b R_rel, p_o = p_b + R_b t_rel from the frames just rolled (contraction off), not from D.state.  Thread 0 and
//            threads 1..3 are lanes of one wave, so the original's two branches ran one after the other as well: the order costs the
//            barrier and nothing else (DESIGN.md).
//   phase 3  (gradient only) a shape of an attached object takes the joint mask KIN_ANC.m[b] of its body: the objects' b + 1 are made
//            wave-uniform behind phase 2, picked by a compare chain over the masked object index sd_pair returns, and fed to the
//            original's compare chain over the body index.  A free object has no mask, as before.
// The table's body index is clamped to [0, NB) before it indexes the frames in LDS; no other value of the table forms an address.
// Reported ids are unchanged: an object is 16 + o, attached or not.
#define ATT_ROW 16           // floats of a table row: R_rel 0..8, t_rel 9..11, b + 1 as an integer 12, 13..15 zero
#define ATT_BODY 12

__global__ void __launch_bounds__(256) k_attach_set(int N, const float *__restrict__ src /*[N][NOBJ][ATT_ROW]*/, const unsigned char *__restrict__ mask /*[N] or nullptr: all*/,
                                                    float *__restrict__ table) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N * (NOBJ * ATT_ROW)) return;
    if (mask && !mask[i / (NOBJ * ATT_ROW)]) return;
    table[i] = src[i];
}

__global__ void __launch_bounds__(64) k_attach_capture(BodyParams B, SimParams P, DevPtrs D, const unsigned char *__restrict__ mask /*[N] or nullptr: all*/,
                                                       float *__restrict__ table) {
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][RAY_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    const int N = P.N, tid = threadIdx.x;
    const int env = min((int)blockIdx.x, N - 1);
    dist_stage_frames<1, 64>(B, D, N, env, tid, s_st, s_fr, s_ob);
    if (tid >= NOBJ || (mask && !mask[env])) return;
    float *row = table + ((size_t)env * NOBJ + tid) * ATT_ROW;
    const int at = __float_as_int(row[ATT_BODY]);
    if (at <= 0) return;
    const int b = min(at, NB) - 1;
    m3 Rb, Ro;
#pragma unroll
    for (int k = 0; k < 9; k++) { Rb.m[k] = s_fr[0][9 * b + k]; Ro.m[k] = s_ob[0][12 * tid + k]; }
    const v3 pb = mk(s_fr[0][RAY_FR_P + 3 * b], s_fr[0][RAY_FR_P + 3 * b + 1], s_fr[0][RAY_FR_P + 3 * b + 2]);
    const v3 po = mk(s_ob[0][12 * tid + 9], s_ob[0][12 * tid + 10], s_ob[0][12 * tid + 11]);
    const m3 Rr = nc::mul(transpose(Rb), Ro);
    const v3 tr = nc::tmulv(Rb, nc::sub(po, pb));
#pragma unroll
    for (int k = 0; k < 9; k++) row[k] = Rr.m[k];
    row[9] = tr.x; row[10] = tr.y; row[11] = tr.z;
}

// Phase 2 of the carry variants for object o (threads 1..NOBJ, behind the barrier that follows the forward kinematics): its frame into
// ob[12 o ..], and b + 1 of its body (0: free) back.  The free branch is the originals' text.
__device__ __forceinline__ int carry_stage_object(const float *__restrict__ att, const int env, const int o, float (*s_st)[1], const float *fr, float *s_ob) {
    const float *ar = att + ((size_t)env * NOBJ + o) * ATT_ROW;
    const int at = min(max(__float_as_int(ar[ATT_BODY]), 0), NB);
    float *ob = s_ob + 12 * o;
    if (at > 0) {
        const int b = at - 1;
        m3 Rb, Rr;
#pragma unroll
        for (int k = 0; k < 9; k++) { Rb.m[k] = fr[9 * b + k]; Rr.m[k] = ar[k]; }
        const m3 Ro = nc::mul(Rb, Rr);
        const v3 po = nc::add(mk(fr[RAY_FR_P + 3 * b], fr[RAY_FR_P + 3 * b + 1], fr[RAY_FR_P + 3 * b + 2]), nc::mulv(Rb, mk(ar[9], ar[10], ar[11])));
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = po.x; ob[10] = po.y; ob[11] = po.z;
    } else {
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][0], s_st[21 + 4 * o][0], s_st[22 + 4 * o][0], s_st[23 + 4 * o][0]);
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][0]; ob[10] = s_st[12 + 3 * o][0]; ob[11] = s_st[13 + 3 * o][0];
    }
    return at;
}

__global__ void __launch_bounds__(PC_THREADS) k_posture_clearance_carry(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                        const float *__restrict__ postures /*[N][K][11]*/, int K,
                                                                        float4 *__restrict__ out_near /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                        float *__restrict__ out_dist /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/,
                                                                        const float *__restrict__ att /*[N][NOBJ][ATT_ROW]*/) {
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
    }
    __syncthreads();
    if (tid >= 1 && tid < 1 + NOBJ) carry_stage_object(att, env, tid - 1, s_st, s_fr[0], s_ob[0]);
    __syncthreads();
    // 3
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    float key = INFINITY;
    int bj = wave, bst = 0, ba = -1, bb = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0, b2 = b0;
    for (int j = wave; j < Q; j += PC_WAVES) {
        const DistItem R = dist_pair(S, tab, j, s_fr[0], s_ob[0], cull, maxd, lane);
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

__global__ void __launch_bounds__(SD_THREADS) k_signed_distance_carry(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                      const float *__restrict__ postures /*[N][K][11] or null: the present state, K = 1*/, int K,
                                                                      float4 *__restrict__ out_deep /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                      float *__restrict__ out_signed /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/,
                                                                      float4 *__restrict__ out_pts /*[N][Q][3] or null*/, const float *__restrict__ att /*[N][NOBJ][ATT_ROW]*/) {
    static_assert(RAY_ST == 32 && NB == 11 && ST_OPOS == 2 * NB, "staged slot s is joint s (s < 11) or state slot s + 11");
    static_assert(64 * DIST_TRIPS == VMAXC && 4 + SD_TRIP_CAP <= 64, "a lane holds three vertices of a shape and one of the polytope");
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][RAY_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    __shared__ float s_best[SD_WAVES][SD_PARK];
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row = blockIdx.x;                                    // e * K + k
    const int env = min((int)(row / (size_t)K), N - 1);
    // 1
    if (tid < RAY_ST) s_st[tid][0] = tid < NB ? (postures ? postures[row * NB + tid] : D.state[(size_t)tid * N + env]) : D.state[(size_t)(tid + NB) * N + env];
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
    }
    __syncthreads();
    if (tid >= 1 && tid < 1 + NOBJ) carry_stage_object(att, env, tid - 1, s_st, s_fr[0], s_ob[0]);
    __syncthreads();
    // 3
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    float key = INFINITY;
    int bj = wave, bst = 0, ba = -1, bb = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0, b2 = b0;
    for (int j = wave; j < Q; j += SD_WAVES) {
        const SdItem R = sd_pair(S, tab, j, s_fr[0], s_ob[0], cull, maxd, lane);
        if (lane == 0) {
            out_signed[row * Q + j] = R.o0.x;
            out_status[row * Q + j] = (R.status & 255) | ((R.iters & 255) << 8) | ((R.trips & 255) << 16);
            if (out_pts) { out_pts[3 * (row * Q + j)] = R.o0; out_pts[3 * (row * Q + j) + 1] = R.o1; out_pts[3 * (row * Q + j) + 2] = R.o2; }
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
        for (int w = 1; w < SD_WAVES; w++) {
            const bool lower = s_best[w][12] < s_best[win][12] ||
                               (s_best[w][12] == s_best[win][12] && __float_as_int(s_best[w][13]) < __float_as_int(s_best[win][13]));
            win = (w < Q && lower) ? w : win;                               // a wave behind the table's end had no pair
        }
        const float *w = s_best[win];
        out_deep[3 * row] = make_float4(w[0], w[1], w[2], w[3]);
        out_deep[3 * row + 1] = make_float4(w[4], w[5], w[6], w[7]);
        out_deep[3 * row + 2] = make_float4(w[8], w[9], w[10], w[11]);
        out_id[row] = make_int4(__float_as_int(w[14]), __float_as_int(w[13]), __float_as_int(w[15]), __float_as_int(w[16]));
    }
}

__global__ void __launch_bounds__(SD_THREADS) k_signed_gradient_carry(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                      const float *__restrict__ postures /*[N][K][11] or null: the present state, K = 1*/, int K,
                                                                      float4 *__restrict__ out_deep /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                      float *__restrict__ out_signed /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/,
                                                                      float4 *__restrict__ out_pts /*[N][Q][3] or null*/, float margin,
                                                                      float *__restrict__ out_grad /*[N][K][12]*/, float *__restrict__ out_cost /*[N][K][12]*/,
                                                                      float *__restrict__ out_pgrad /*[N][Q][12] or null*/, const float *__restrict__ att /*[N][NOBJ][ATT_ROW]*/) {
    static_assert(RAY_ST == 32 && NB == 11 && ST_OPOS == 2 * NB, "staged slot s is joint s (s < 11) or state slot s + 11");
    static_assert(64 * DIST_TRIPS == VMAXC && 4 + SD_TRIP_CAP <= 64, "a lane holds three vertices of a shape and one of the polytope");
    static_assert(NB + 1 == SG_ROW && SG_ROW <= 64, "a lane per column of a row");
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][SG_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    __shared__ float s_best[SD_WAVES][SD_PARK];
    __shared__ float s_grad[SD_WAVES][2][SG_ROW];              // per wave: its best pair's row, its accumulator
    __shared__ int s_att[NOBJ];                                // b + 1 of every object's body, 0: free
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row = blockIdx.x;                                    // e * K + k
    const int env = min((int)(row / (size_t)K), N - 1);
    // 1
    if (tid < RAY_ST) s_st[tid][0] = tid < NB ? (postures ? postures[row * NB + tid] : D.state[(size_t)tid * N + env]) : D.state[(size_t)(tid + NB) * N + env];
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
            const v3 aw = nc::mulv(Rj, ax);
#pragma unroll
            for (int k = 0; k < 9; k++) fr[9 * b + k] = Rb.m[k];
            fr[RAY_FR_P + 3 * b] = pb.x; fr[RAY_FR_P + 3 * b + 1] = pb.y; fr[RAY_FR_P + 3 * b + 2] = pb.z;
            fr[SG_FR_AX + 3 * b] = aw.x; fr[SG_FR_AX + 3 * b + 1] = aw.y; fr[SG_FR_AX + 3 * b + 2] = aw.z;
        }
    }
    __syncthreads();
    if (tid >= 1 && tid < 1 + NOBJ) s_att[tid - 1] = carry_stage_object(att, env, tid - 1, s_st, s_fr[0], s_ob[0]);
    __syncthreads();
    // 3
    int at[NOBJ];
#pragma unroll
    for (int o = 0; o < NOBJ; o++) at[o] = __builtin_amdgcn_readfirstlane(s_att[o]);
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    float key = INFINITY;
    int bj = wave, bst = 0, ba = -1, bb = -1;
    float4 b0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b1 = b0, b2 = b0;
    const int jk = min(lane, NB - 1);                                 // this lane's joint (lanes behind the row read joint 10's and store nothing)
    if (lane < SG_ROW) { s_grad[wave][0][lane] = 0.0f; s_grad[wave][1][lane] = 0.0f; }     // (a lane reads back its own floats only: no barrier)
    for (int j = wave; j < Q; j += SD_WAVES) {
        const SdItem R = sd_pair(S, tab, j, s_fr[0], s_ob[0], cull, maxd, lane);
        if (lane == 0) {
            out_signed[row * Q + j] = R.o0.x;
            out_status[row * Q + j] = (R.status & 255) | ((R.iters & 255) << 8) | ((R.trips & 255) << 16);
            if (out_pts) { out_pts[3 * (row * Q + j)] = R.o0; out_pts[3 * (row * Q + j) + 1] = R.o1; out_pts[3 * (row * Q + j) + 2] = R.o2; }
        }
        const float4 u0 = pc_uniform(R.o0), u1 = pc_uniform(R.o1), u2 = pc_uniform(R.o2);
        const int st = __builtin_amdgcn_readfirstlane(R.status);
        // the body that moves each shape: its own for a robot shape, the carrying one for a shape of an attached object, none otherwise
        const int oba = __builtin_amdgcn_readfirstlane(R.ota == 2 ? R.oia : -1), obb = __builtin_amdgcn_readfirstlane(R.otb == 2 ? R.oib : -1);
        int ca = 0, cb = 0;
#pragma unroll
        for (int o = 0; o < NOBJ; o++) { ca = oba == o ? at[o] : ca; cb = obb == o ? at[o] : cb; }
        const int boda = __builtin_amdgcn_readfirstlane(R.ota == 1 ? R.oia : ca - 1), bodb = __builtin_amdgcn_readfirstlane(R.otb == 1 ? R.oib : cb - 1);
        // the joints that move each shape's body: the compile-time table read by a compare chain, no mask without a match
        unsigned ma = 0u, mb = 0u;
#pragma unroll
        for (int q = 0; q < NB; q++) { ma = boda == q ? KIN_ANC.m[q] : ma; mb = bodb == q ? KIN_ANC.m[q] : mb; }
        // the joint's world axis and position, read behind the pair through an index the compiler cannot see through (rr_grad.inc)
        int jq = jk;
        asm volatile("" : "+v"(jq));
        const v3 jax = mk(s_fr[0][SG_FR_AX + 3 * jq], s_fr[0][SG_FR_AX + 3 * jq + 1], s_fr[0][SG_FR_AX + 3 * jq + 2]);
        const v3 jp = mk(s_fr[0][RAY_FR_P + 3 * jq], s_fr[0][RAY_FR_P + 3 * jq + 1], s_fr[0][RAY_FR_P + 3 * jq + 2]);
        const v3 xa = mk(u0.z, u0.w, u1.x), xb = mk(u1.y, u1.z, u1.w), n = mk(u2.x, u2.y, u2.z);
        const float ga = dot(n, cross(jax, xa - jp)), gb = dot(n, cross(jax, xb - jp));
        const float gm = (((ma >> jk) & 1u) ? ga : 0.0f) - (((mb >> jk) & 1u) ? gb : 0.0f);
        const float g = (st == 4 || lane >= NB) ? 0.0f : gm;          // lane 11: the row's twelfth float
        if (out_pgrad && lane < SG_ROW) out_pgrad[(row * Q + j) * SG_ROW + lane] = g;
        const float c = margin - u0.x;
        if (c > 0.0f && lane < SG_ROW) { const float acc = s_grad[wave][1][lane]; s_grad[wave][1][lane] = lane < NB ? acc - c * g : acc + 0.5f * c * c; }
        const float d = u0.x;
        const bool nearer = d < key;
        if (nearer || j == wave) {                                      // (uniform in the wave)
            bj = j; bst = st;
            ba = __builtin_amdgcn_readfirstlane(R.ota == 0 ? -1 : (R.ota == 1 ? R.oia : 16 + R.oia));
            bb = __builtin_amdgcn_readfirstlane(R.otb == 0 ? -1 : (R.otb == 1 ? R.oib : 16 + R.oib));
            b0 = u0; b1 = u1; b2 = u2;
            if (lane < SG_ROW) s_grad[wave][0][lane] = g;
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
    if (tid < SG_ROW) {
        int win = 0;
        for (int w = 1; w < SD_WAVES; w++) {
            const bool lower = s_best[w][12] < s_best[win][12] ||
                               (s_best[w][12] == s_best[win][12] && __float_as_int(s_best[w][13]) < __float_as_int(s_best[win][13]));
            win = (w < Q && lower) ? w : win;                               // a wave behind the table's end had no pair
        }
        if (tid == 0) {
            const float *w = s_best[win];
            out_deep[3 * row] = make_float4(w[0], w[1], w[2], w[3]);
            out_deep[3 * row + 1] = make_float4(w[4], w[5], w[6], w[7]);
            out_deep[3 * row + 2] = make_float4(w[8], w[9], w[10], w[11]);
            out_id[row] = make_int4(__float_as_int(w[14]), __float_as_int(w[13]), __float_as_int(w[15]), __float_as_int(w[16]));
        }
        out_grad[row * SG_ROW + tid] = s_grad[win][0][tid];
        float sum = s_grad[0][1][tid];                                      // (a wave without a pair parked +0.0)
#pragma unroll
        for (int w = 1; w < SD_WAVES; w++) sum += s_grad[w][1][tid];
        out_cost[row * SG_ROW + tid] = sum;
    }
}
