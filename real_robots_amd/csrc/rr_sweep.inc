// rr_sweep.inc -- part of realrobot.hip (included there, behind rr_posture.inc; not a stand-alone translation unit).
// k_swept_clearance: K joint-space segments per env of the whole batch, q(t) = q0 + t (q1 - q0), t in [0, 1], decided by conservative
// advancement (rr_swept_clearance, realrobot.h): is the motion free of the pair table by `safety`, and if not, where does it first
// touch and what.  Read-only on the simulation (D.state's object columns, the model constants, the pair table, the reach table and
// the tensor; never the preparation record); launched by rr_swept_clearance alone, never by a step.
//
// ONE WAVE64 PER (env, segment): a 64-thread workgroup per row, grid N * K exactly.  k_posture_clearance's shape -- a 256-thread
// workgroup per row, the due pairs of a step spread over four waves -- was built first and measured against this one (the same text
// with SWEEP_THREADS 256): behind the first step one or two pairs are due, three waves of four only wait at the barriers, and the
// row takes four times the wave slots of this shape; it was 7 % faster where every row ends after one step and 2.3 x where most rows run
// to the step cap (DESIGN.md).  The text keeps the general form: wave w takes the due entries w, w + SWEEP_WAVES, ...  A pair is
// rr_dist.inc's dist_pair, the function k_closest_points and k_posture_clearance run, so a record has those kernels' bits (the tests
// assert it).
//   1  the staged floats into LDS: q0 and dq = q1 - q0 from the segment's 88-byte row, slots 11..31 (object positions and
//      quaternions) from D.state; the object rotations on three lanes, once; a thread per pair j the motion bound B_j:
//      sum over the joints k that are an ancestor-or-self of exactly one of the two shapes' bodies (masks out of PARENT) of
//      |dq_k| (R[k][a] + R[k][b]), ascending k in float32, times 1 + 2^-20 (rounding never lowers it); horizon free_j = 0;
//   2  a step: lanes 0..10 store q_k = fma(t, dq_k, q0_k) into slots 0..10; the rolled forward kinematics on one lane --
//      k_posture_clearance's phase 2 restated (its operations in its order: the bits of rr_posture_clearance at q_stop);
//   3  the due pairs (free_j <= t) from the step's list, one after the other, all 64 lanes on a pair; lane 0 stores the pair's
//      proved lower bound (the `lower` column of the record);
//   4  wave 0 alone, behind a barrier: lane l looks at the pairs l and l + 64.  A pair evaluated in this step with
//      g = lower - safety hits unless g > tolerance (a NaN hits), else free_j = t + g / B_j (+inf where B_j == 0).  A hit: the
//      lowest hit index (ballot), status 1.  Else the first minimum of the horizons over ascending j (a butterfly over (value,
//      index) that prefers the lower value and among equals the lower index; a NaN never wins): at or beyond 1 the row is free,
//      status 0; the step cap, status 3; else t = that minimum and the due list of the next step, in ascending j (ballot and
//      population count).  A row that stops with status 1 or 3 gets ONE more pass of phase 3 over the reported pair alone, at the
//      frames of the last step: RR_SW_HIT;
//   5  a thread per pair writes min(free_j, 1), lanes 0..11 of wave 0 the stop row, lane 0 the id row.
// The loop's conditions are read from LDS behind a barrier: uniform in the workgroup, every wave reaches every barrier; at most
// RR_SW_MAX_STEPS postures are evaluated whatever the data.  No atomics, fixed order: row (e, k) is a function of (env e's objects,
// segment (e, k), the tables, safety, tolerance) alone.  Loop bounds are constants or Q; no value of the tensor or the state forms
// an address (a due list holds pair indices below Q).
#ifndef SWEEP_THREADS
#define SWEEP_THREADS 64         // one wave per row; 256 (four waves share a row's due pairs) was measured slower (DESIGN.md)
#endif
#define SWEEP_WAVES (SWEEP_THREADS / 64)

// the device copy of the handle's reach table (rr_sweep_reach): R[k][s], 0 where joint k does not move shape s
struct SweepReach { float r[NB][MAXSHAPES]; };

// ancestors-or-self of the body of a robot shape as a bit mask over the joints; 0 for statics and objects
__device__ __forceinline__ unsigned sw_joint_mask(const int otype, const int oidx) {
    unsigned m = 0;
    int b = otype == 1 ? min(max(oidx, 0), NB - 1) : -1;
    for (int i = 0; i < NB; i++) {
        if (b >= 0) { m |= 1u << b; b = PARENT[b]; }
    }
    return m;
}

__global__ void __launch_bounds__(SWEEP_THREADS) k_swept_clearance(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                const SweepReach *__restrict__ reach, const float *__restrict__ segments /*[N][K][2][11]*/, int K,
                                                                float safety, float tolerance,
                                                                float *__restrict__ out_stop /*[N][K][12]*/, float4 *__restrict__ out_hit /*[N][K][3]*/,
                                                                int4 *__restrict__ out_id /*[N][K]*/, float *__restrict__ out_free /*[N][K][Q]*/) {
    static_assert(RAY_ST == 32 && NB == 11 && ST_OPOS == 2 * NB, "staged slot s is the posture's column s (s < 11) or state slot s + 11");
    static_assert(RR_DIST_MAX <= 128 && SWEEP_THREADS >= 64, "phase 4: a lane of wave 0 looks at two pairs");
    __shared__ float s_st[RAY_ST][1];
    __shared__ float s_fr[1][RAY_FR];
    __shared__ float s_ob[1][12 * NOBJ + 1];
    __shared__ float s_q0[NB], s_dq[NB];
    __shared__ float s_bound[RR_DIST_MAX], s_free[RR_DIST_MAX], s_low[RR_DIST_MAX];
    __shared__ int s_due[RR_DIST_MAX];
    __shared__ int s_ndue, s_mode, s_steps, s_evals;                   // s_mode: 0 advance, 1 the record pass of a stopped row, 2 done
    __shared__ float s_t;
    const ShapeData *__restrict__ S = D.shapes;
    const int N = P.N, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row = blockIdx.x;                                    // e * K + k
    const int env = min((int)(row / (size_t)K), N - 1);
    // 1
    if (tid < RAY_ST) {
        if (tid < NB) {
            const float a = segments[row * (2 * NB) + tid], b = segments[row * (2 * NB) + NB + tid];
            s_q0[tid] = a; s_dq[tid] = b - a;
            s_st[tid][0] = a;
        } else {
            s_st[tid][0] = D.state[(size_t)(tid + NB) * N + env];
        }
    }
    if (tid == 0) { s_t = 0.0f; s_mode = 0; s_steps = 0; s_evals = 0; s_ndue = Q; }
    __syncthreads();
    if (tid >= 1 && tid < 1 + NOBJ) {
        const int o = tid - 1;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][0], s_st[21 + 4 * o][0], s_st[22 + 4 * o][0], s_st[23 + 4 * o][0]);
        float *ob = s_ob[0] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][0]; ob[10] = s_st[12 + 3 * o][0]; ob[11] = s_st[13 + 3 * o][0];
    }
    for (int j = tid; j < Q; j += SWEEP_THREADS) {
        const int sa = min(max(tab->a[j], 0), MAXSHAPES - 1), sb = min(max(tab->b[j], 0), MAXSHAPES - 1);
        const unsigned ma = sw_joint_mask(S->otype[sa], S->oidx[sa]), mb = sw_joint_mask(S->otype[sb], S->oidx[sb]);
        const unsigned one = ma ^ mb;
        float bsum = 0.0f;
        for (int k = 0; k < NB; k++) {
            const float term = fabsf(s_dq[k]) * (reach->r[k][sa] + reach->r[k][sb]);
            bsum += ((one >> k) & 1u) ? term : 0.0f;
        }
        s_bound[j] = bsum * (1.0f + 0x1p-20f);
        s_free[j] = 0.0f;
        s_low[j] = 0.0f;
        s_due[j] = j;
    }
    const float maxd = tab->max_distance;
    const bool cull = maxd > 0.0f && maxd < INFINITY;
    for (int trip = 0; trip < RR_SW_MAX_STEPS + 1; trip++) {          // (the record pass is a trip: the cap + 1 bounds the loop on its own)
        __syncthreads();
        const int mode = s_mode;
        if (mode == 2) break;                                           // (uniform in the workgroup)
        // 2
        if (mode == 0) {
            if (tid < NB) s_st[tid][0] = __fmaf_rn(s_t, s_dq[tid], s_q0[tid]);
            __syncthreads();
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
        }
        // 3
        const int ndue = min(max(s_ndue, 0), Q);
        for (int i = wave; i < ndue; i += SWEEP_WAVES) {
            const int j = min(max(__builtin_amdgcn_readfirstlane(s_due[i]), 0), Q - 1);
            const DistItem R = dist_pair(S, tab, j, s_fr[0], s_ob[0], cull, maxd, lane);
            if (lane == 0) {
                if (mode == 0) {
                    s_low[j] = R.o0.y;
                } else {
                    out_hit[3 * row] = R.o0; out_hit[3 * row + 1] = R.o1; out_hit[3 * row + 2] = R.o2;
                }
            }
        }
        __syncthreads();
        // 4
        if (wave == 0) {
            if (mode != 0) {
                if (lane == 0) s_mode = 2;
            } else {
                const float t = s_t;
                const int steps = s_steps + 1, evals = s_evals + ndue;
                bool hit[2];
                float fr_[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int j = lane + 64 * h;
                    const bool in = j < Q;
                    const int jj = in ? j : 0;
                    float f = s_free[jj];
                    const bool due = in && f <= t;
                    const float g = s_low[jj] - safety, bj = s_bound[jj];
                    hit[h] = due && !(g > tolerance);
                    if (due && !hit[h]) {
                        f = bj > 0.0f ? t + g / bj : INFINITY;
                        s_free[jj] = f;
                    }
                    fr_[h] = in ? f : INFINITY;
                }
                const unsigned long long h0 = __ballot(hit[0]), h1 = __ballot(hit[1]);
                // the first minimum of the horizons: the lane's two (the lower index first), then the butterfly
                float best = fr_[0];
                int bi = lane;
                if (fr_[1] < best || !(best == best)) { best = fr_[1]; bi = lane + 64; }
                if (!(best == best)) best = INFINITY;                   // (both NaN: never wins)
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    const float ov = __shfl_xor(best, m);
                    const int oi = __shfl_xor(bi, m);
                    const bool take = ov < best || (ov == best && oi < bi);
                    best = take ? ov : best;
                    bi = take ? oi : bi;
                }
                bi = min(max(__builtin_amdgcn_readfirstlane(bi), 0), Q - 1);
                int next_mode = 0, pair = -1;
                if (h0 != 0ull || h1 != 0ull) {
                    next_mode = 1;
                    pair = h0 != 0ull ? __ffsll((long long)h0) - 1 : 64 + __ffsll((long long)h1) - 1;
                } else if (best >= 1.0f) {
                    next_mode = 2;
                } else if (steps >= RR_SW_MAX_STEPS) {
                    next_mode = 1;
                    pair = bi;
                }
                const int status = next_mode == 0 ? 3 : (next_mode == 2 ? 0 : (h0 != 0ull || h1 != 0ull ? 1 : 3));
                if (next_mode == 0) {
                    const bool d0 = fr_[0] <= best, d1 = fr_[1] <= best;
                    const unsigned long long m0 = __ballot(d0), m1 = __ballot(d1);
                    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
                    if (d0) s_due[__popcll(m0 & below)] = lane;
                    if (d1) s_due[__popcll(m0) + __popcll(m1 & below)] = lane + 64;
                    if (lane == 0) { s_ndue = __popcll(m0) + __popcll(m1); s_t = best; }
                } else if (lane == 0) {
                    s_due[0] = max(pair, 0); s_ndue = next_mode == 1 ? 1 : 0;
                }
                if (lane == 0) { s_mode = next_mode; s_steps = steps; s_evals = evals; }
                // 5 (the row's last step only; a later trip writes RR_SW_HIT alone)
                if (next_mode != 0) {
                    if (lane < 12) out_stop[row * 12 + lane] = lane == 0 ? (status == 0 ? 1.0f : t) : s_st[lane - 1][0];
                    if (lane == 0) out_id[row] = make_int4(status, pair, steps, evals);
                    if (next_mode == 2 && lane < 3) out_hit[3 * row + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < Q; j += SWEEP_THREADS) out_free[row * Q + j] = fminf(s_free[j], 1.0f);
}
