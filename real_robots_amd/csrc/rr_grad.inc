// rr_grad.inc -- part of realrobot.hip (included there, behind rr_signed.inc; not a stand-alone translation unit).
// k_signed_gradient: k_signed_distance plus, per row, the JOINT GRADIENT of the deepest pair's signed distance, a hinge collision cost
// over all pairs and that cost's gradient, both reduced on the device; a present-state query also gets every pair's gradient
// (rr_signed_gradient, realrobot.h).  Read-only on the simulation like its sibling; launched by rr_signed_gradient alone, never by a step.
//
// The launch shape, the staging, the frames, the pair (sd_pair of rr_signed.inc, called, not restated) and the reduction of the record
// are k_signed_distance's: the five RR_SD_* buffers get the same bytes.  What is added:
//   phase 2  also keeps the WORLD AXIS of every joint, nc::mulv(Rj, ax) as k_kinematics forms it, in 33 more LDS floats behind the frames;
//   phase 3  behind sd_pair the record is made wave-uniform, and lanes 0..10 compute one column each,
//                g_k = [k moves A's body] n . (a_k x (a - p_k)) - [k moves B's body] n . (a_k x (b - p_k)),
//            in plain float32, the two masks out of a compare chain over the body index on the compile-time ancestor table KIN_ANC (a
//            static shape or an object has no mask: +0.0 - +0.0); a touching pair (status 4) gets +0.0.  Lanes 0..11 write the pair's row
//            {g_0..10, +0.0} (present state only), keep the row of the wave's best pair under the rule that carries the record
//            (nearer || j == wave), and, with c = margin - s where that is > 0, add -c g_k (lanes 0..10) and c^2 / 2 (lane 11) to a
//            per-lane accumulator: a pair with c not > 0 -- a NaN among them -- adds nothing.  The kept row and the accumulator live in
//            LDS, a float per lane that only that lane touches before the barrier: in registers the two floats, live across sd_pair,
//            took the kernel from 125 to 129 VGPRs and from four waves per SIMD to three (the lane's joint axis and position are read
//            behind the pair for the same reason);
//   phase 4  behind the one barrier thread k < 12 picks the winning wave's row by thread 0's rule and sums the four waves'
//            accumulators in the order 0, 1, 2, 3.
// The sums run in a fixed order (a wave's pairs j = w, w + 4, ... ascending from +0.0, then the waves in order), in float32, without
// atomics: identical from call to call and independent of N, K and the row's place; a permuted table sums in another order.
// No value of the tensor or the state forms an address: LDS is indexed by the lane number and by the masked body indices sd_pair returns.
// With carried objects the kernel is a template <bool CARRY> like its sibling (rr_posture.inc's header, rr_carry.inc's header): <true>
// stages the objects behind one more barrier in phase 2 and keeps every object's b + 1 (s_att, 12 bytes of LDS that <false> does not
// have); in phase 3 a shape of an attached object takes the joint mask of the carrying body, picked by a compare chain over the masked
// object index and fed to the one compare chain over the body index.  <false> is the text above and nothing else: ca - 1 is the -1 of
// "no body" there.
#define SG_FR_AX RAY_FR              // the world axes behind an env's frames: 33 floats
#define SG_FR (RAY_FR + 3 * NB)
#define SG_ROW 12                    // floats of a gradient row: eleven joints and one more (+0.0, or the cost)

template <bool CARRY>
__global__ void __launch_bounds__(SD_THREADS) k_signed_gradient(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                const float *__restrict__ postures /*[N][K][11] or null: the present state, K = 1*/, int K,
                                                                float4 *__restrict__ out_deep /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                float *__restrict__ out_signed /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/,
                                                                float4 *__restrict__ out_pts /*[N][Q][3] or null*/, float margin,
                                                                float *__restrict__ out_grad /*[N][K][12]*/, float *__restrict__ out_cost /*[N][K][12]*/,
                                                                float *__restrict__ out_pgrad /*[N][Q][12] or null*/,
                                                                const float *__restrict__ att /*[N][NOBJ][ATT_ROW]; null and unread without CARRY*/) {
    static_assert(RAY_ST == 32 && NB == 11 && ST_OPOS == 2 * NB, "staged slot s is joint s (s < 11) or state slot s + 11");
    static_assert(64 * DIST_TRIPS == VMAXC && 4 + SD_TRIP_CAP <= 64, "a lane holds three vertices of a shape and one of the polytope");
    static_assert(NB + 1 == SG_ROW && SG_ROW <= 64, "a lane per column of a row");
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][SG_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    __shared__ float s_best[SD_WAVES][SD_PARK];
    __shared__ float s_grad[SD_WAVES][2][SG_ROW];              // per wave: its best pair's row, its accumulator
    __shared__ int s_att[CARRY ? NOBJ : 1];                    // b + 1 of every object's body, 0: free (never named without CARRY: no LDS then)
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
    } else if (!CARRY && tid < 1 + NOBJ) {
        const int o = tid - 1;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][0], s_st[21 + 4 * o][0], s_st[22 + 4 * o][0], s_st[23 + 4 * o][0]);
        float *ob = s_ob[0] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][0]; ob[10] = s_st[12 + 3 * o][0]; ob[11] = s_st[13 + 3 * o][0];
    }
    __syncthreads();
    if constexpr (CARRY) {
        if (tid >= 1 && tid < 1 + NOBJ) s_att[tid - 1] = carry_stage_object(att, env, tid - 1, s_st, s_fr[0], s_ob[0]);
        __syncthreads();
    }
    // 3
    int at[NOBJ];                                                     // the objects' b + 1, wave-uniform (filled and read with CARRY only)
    if constexpr (CARRY) {
#pragma unroll
        for (int o = 0; o < NOBJ; o++) at[o] = __builtin_amdgcn_readfirstlane(s_att[o]);
    }
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
        int ca = 0, cb = 0;                                             // b + 1 of the carrying body
        if constexpr (CARRY) {
            const int oba = __builtin_amdgcn_readfirstlane(R.ota == 2 ? R.oia : -1), obb = __builtin_amdgcn_readfirstlane(R.otb == 2 ? R.oib : -1);
#pragma unroll
            for (int o = 0; o < NOBJ; o++) { ca = oba == o ? at[o] : ca; cb = obb == o ? at[o] : cb; }
        }
        const int boda = __builtin_amdgcn_readfirstlane(R.ota == 1 ? R.oia : ca - 1), bodb = __builtin_amdgcn_readfirstlane(R.otb == 1 ? R.oib : cb - 1);
        // the joints that move each shape's body: the compile-time table read by a compare chain, no mask without a match
        unsigned ma = 0u, mb = 0u;
#pragma unroll
        for (int q = 0; q < NB; q++) { ma = boda == q ? KIN_ANC.m[q] : ma; mb = bodb == q ? KIN_ANC.m[q] : mb; }
        // the joint's world axis and position, read behind the pair through an index the compiler cannot see through: with a plain index
        // the six loads are hoisted out of the loop and stay live across sd_pair (131 VGPRs, three waves per SIMD)
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
