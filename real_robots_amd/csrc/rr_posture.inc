// rr_posture.inc -- part of realrobot.hip (included there, behind rr_dist.inc and rr_carry.inc; not a stand-alone translation unit).
// k_posture_clearance: the clearance of K candidate joint postures per env of the whole batch (rr_posture_clearance, realrobot.h):
// posture (e, k) is env e's present state with its eleven joint columns taken from the caller's tensor, the objects where they are;
// per posture the distance and status of every pair of the table (rr_set_distance_pairs) and the full record of the NEAREST pair,
// reduced on the device.  Read-only on the simulation (D.state's object columns, the model constants, the pair table and the
// tensor; never the preparation record); launched by rr_posture_clearance alone, never by a step.
//
// One 256-thread workgroup per (env, posture), grid N * K exactly; its four waves take every fourth pair, ONE WAVE64 PER PAIR, and a
// pair is steps a to c of rr_dist.inc's header (cull, vertices about the sphere centre, GJK with float64 norms): that file's
// dist_pair, the function k_closest_points runs, so an item has that kernel's bits (the tests assert it).
//   1  the 32 staged floats into LDS: slots 0..10 from the posture's 44-byte row of the tensor, 11..31 (object positions and
//      quaternions) from D.state;
//   2  the rolled forward kinematics on one lane and the object rotations on three -- dist_stage_frames' phase 2 restated (the nc::
//      twins in the step's order), that function reads its joints from D.state.  One function for this phase and one for phases 3
//      and 4, shared with k_signed_distance, were built and measured: this kernel then compiled to other scalar code and was 0.2 %
//      slower on the collision table, so the phases keep their text here (DESIGN.md);
//   3  per pair, lane 0 stores the distance and the status word {status, iterations << 8}; the wave carries its best pair so far in
//      wave-uniform registers (v_readfirstlane: scalar registers) -- the key, j, the record's three float4, status and bodies --,
//      taken when the distance is strictly below the key, over ascending j.  The key starts at +inf and the record at the wave's
//      first pair, so a NaN distance never displaces a number and a wave always has a record;
//   4  lane 0 of each wave parks its best in LDS; behind one barrier thread 0 picks over the waves that had a pair by (key, j) --
//      the first minimum of the row -- and writes RR_PC_NEAREST / RR_PC_ID.  Every wave reaches the barrier: the grid is exact and
//      the pair loop has no early exit.
// No atomics, fixed order: row (e, k) is a function of (env e's objects, posture (e, k), the table) alone.  Loop bounds are
// constants or Q; no value of the tensor or the state forms an address.
//
// WITH CARRIED OBJECTS (rr_set_attachments; rr_carry.inc's header).  The kernel is a template <bool CARRY>: <false> is the text above and
// nothing else, <true> is launched in its place while the handle's attachments are on.  Phase 2 then has one more barrier: thread 0
// rolls the forward kinematics, and behind the barrier threads 1..NOBJ stage the objects with carry_stage_object, an attached one from
// the frames just rolled and its table row, a free one by the operations of <false>.  Everything else is the one text; the carry-only
// statements sit under `if constexpr (CARRY)`, the staging of <false> under `!CARRY`, and the phases stay written out inside the
// template: both instantiations then compile to the instructions of two kernels written out separately (tools/compare_kernel_asm.py
// --map), which a phase shared through a function did not (phase 2 above, DESIGN.md).  att, the table, is the last argument, null and
// unread without CARRY.
#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / 64)
#define PC_PARK 20           // floats a wave parks: the record 0..11, key 12, j 13, status 14, body A 15, body B 16

__device__ __forceinline__ float pc_uniform(const float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ float4 pc_uniform(const float4 x) { return make_float4(pc_uniform(x.x), pc_uniform(x.y), pc_uniform(x.z), pc_uniform(x.w)); }

template <bool CARRY>
__global__ void __launch_bounds__(PC_THREADS) k_posture_clearance(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                  const float *__restrict__ postures /*[N][K][11]*/, int K,
                                                                  float4 *__restrict__ out_near /*[N][K][3]*/, int4 *__restrict__ out_id /*[N][K]*/,
                                                                  float *__restrict__ out_dist /*[N][K][Q]*/, int *__restrict__ out_status /*[N][K][Q]*/,
                                                                  const float *__restrict__ att /*[N][NOBJ][ATT_ROW]; null and unread without CARRY*/) {
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
        if (tid >= 1 && tid < 1 + NOBJ) carry_stage_object(att, env, tid - 1, s_st, s_fr[0], s_ob[0]);
        __syncthreads();
    }
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
