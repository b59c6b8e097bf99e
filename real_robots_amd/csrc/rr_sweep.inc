// rr_sweep.inc -- part of realrobot.hip (included there, behind rr_carry.inc and rr_posture.inc; not a stand-alone translation unit).
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
//
// WITH CARRIED OBJECTS (rr_carried_sweep, realrobot.h).  The kernel is a template <bool CARRY>: k_swept_clearance<false> is the text
// above and nothing else -- every carry-only statement and the one carry-only LDS array sit under `if constexpr (CARRY)` --, and
// rr_swept_clearance launches it; k_swept_clearance<true> is launched by rr_carried_sweep alone while the handle's attachments are on
// (rr_set_attachments).  An object attached to a link moves with that link along q(t), and the motion bound of a pair knows it.  It
// reads in addition the attachment table and the chain table.  The LDS arrays, phases 3, 4 and 5 and the dist_pair call are the one
// text.  Three things differ with CARRY:
//   phase 1  the env's NOBJ table rows go to LDS (s_att); the objects are NOT staged here.  A thread per pair j computes B_j as the
//            plain kernel does -- ascending k, float32, the exclusive-or of the two masks, times 1 + 2^-20 -- with, for a shape s of an
//            object attached to body b, the mask "ancestors-or-self of b" (sw_joint_mask of a robot shape on b) and, for joint k,
//            the reach chain[k][b] + rho in place of reach->r[k][s]; a robot shape, a static and a shape of a free object read
//            reach->r as before.  A carried shape against a shape on its own body, and two carried objects on one body, have equal
//            masks: B_j = 0, horizon +inf after one look.  Two carried objects on different bodies work through the exclusive-or.
//   phase 2  at EVERY step, behind the forward kinematics on lane 0 and a barrier, lanes 1..NOBJ stage the objects with rr_carry.inc's
//            carry_stage_object from the LDS copy of the rows (a one-env table, env 0): an attached object as R_o = R_b R_rel,
//            p_o = p_b + R_b t_rel from the frames just rolled, a free one by the plain kernel's operations.  The record pass of a
//            stopped row uses the frames and objects of the last step: RR_SW_HIT has the bits of rr_posture_clearance at q_stop on the
//            same attached handle (k_posture_clearance<true> runs the same function on the same numbers).
//   the table pointer  att [N][NOBJ][ATT_ROW] and chain [NB][NB] are the last two arguments, null and unread without CARRY.  The
//            table's body index is clamped to [0, NB) before it indexes the frames in LDS and the chain table; no other value of the
//            table forms an address.
// An env with no attachment runs, in every row, the plain kernel's operations in the plain kernel's order on the plain kernel's inputs:
// its bytes are rr_swept_clearance's on a handle that never attached.  No atomics, fixed order: row (e, k) is a function of (env e's
// objects, env e's table rows, segment (e, k), the tables, safety, tolerance) alone.  Loop bounds are constants or Q.
//
// THE REACH OF A CARRIED SHAPE.  chain[k][b], built once on the host in float64 and rounded up (rr_host.inc), is the sum of |jpos[m]|
// over the bodies m from b up to, but not including, k: the term rr_create's reach loop adds.  With (c, r) the bounding sphere of
// shape s in the object's frame and (R, t) the row's R_rel, t_rel, a point x of the shape sits in body b's frame at t + R x, so its
// distance from b's origin is at most |t + R c| + ||R||_2 r: rho.  chain[k][b] + rho then bounds its distance from joint k's origin
// at any posture, as R[k][s] does for a robot shape.
// The device computes rho per row from the table row (a captured row never visits the host) in float32, and must not come out
// below that number.  With u = 2^-24 and v = t + R c:
//   * ||R||_2 is not assumed to be 1: a captured R_rel is a float32 product of float32 frames, orthonormal to rounding only, and the
//     rounding of an eleven-body chain has no useful a-priori bound.  It is MEASURED: ||R||_2^2 <= ||R^T R||_inf, the largest absolute
//     row sum of the Gram matrix; nr = sqrt of that, computed with relative error below 5 u.
//   * v is three products and three sums per component: |dv| <= 4 u (|t| + || |R| |c| ||) <= 4 u |v| + 4 u (1 + sqrt 3) nr |c|,
//     because |t| <= |v| + nr |c| and || |R| || <= sqrt 3 nr.  A cancelling t and R c leave |v| small and this error not: it is
//     covered by an ABSOLUTE term, r is raised by 2^-20 |c|_1 = 16 u |c|_1 >= 11 u |c|.
//   * what is left is relative: 4 u (v) + 3 u (the length: a dot product and a root) + 5 u (nr) + 4 u (the sum |c|_1, its product,
//     its sum with r, the product with nr) + 1 u (the final sum) + 1 u (chain + rho in phase 1) + 1 u (the product with the factor
//     itself): below 20 u to first order.
// CS_INFLATE = 1 + 2^-18 = 1 + 64 u covers it three times over and is a quarter of the 1 + 2^-16 the interface allows.  The 1 + 2^-20
// on B_j covers what it covered before: the two-term sum, the product and the eleven-term accumulation of the original's text.
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

// ---- carried objects (rr_carried_sweep): the reach of a carried shape -------------------------------------------------------------------
#define CS_INFLATE (1.0f + 0x1p-18f)

// the device copy of the handle's chain table (rr_carried_sweep): c[k][b], 0 where joint k is not an ancestor-or-self of body b
struct SweepChain { float c[NB][NB]; };

// rho of a shape with bounding sphere sph = {c, r} (the object's frame) carried at the table row ar = {R_rel, t_rel}: see the header above
__device__ __forceinline__ float cs_rho(const float *ar, const float *__restrict__ sph) {
    const float cx = sph[0], cy = sph[1], cz = sph[2], r = sph[3];
    const float vx = ar[9] + (ar[0] * cx + ar[1] * cy + ar[2] * cz);
    const float vy = ar[10] + (ar[3] * cx + ar[4] * cy + ar[5] * cz);
    const float vz = ar[11] + (ar[6] * cx + ar[7] * cy + ar[8] * cz);
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    const float g00 = ar[0] * ar[0] + ar[3] * ar[3] + ar[6] * ar[6], g11 = ar[1] * ar[1] + ar[4] * ar[4] + ar[7] * ar[7], g22 = ar[2] * ar[2] + ar[5] * ar[5] + ar[8] * ar[8];
    const float g01 = fabsf(ar[0] * ar[1] + ar[3] * ar[4] + ar[6] * ar[7]), g02 = fabsf(ar[0] * ar[2] + ar[3] * ar[5] + ar[6] * ar[8]);
    const float g12 = fabsf(ar[1] * ar[2] + ar[4] * ar[5] + ar[7] * ar[8]);
    const float nr = sqrtf(fmaxf(fmaxf(g00 + g01 + g02, g01 + g11 + g12), g02 + g12 + g22));
    return (len + nr * (r + 0x1p-20f * (fabsf(cx) + fabsf(cy) + fabsf(cz)))) * CS_INFLATE;
}

// The body that carries shape s (-1: none -- a robot shape, a static, a shape of a free object) and, for a carried shape, its joint
// mask and rho.  rows: the env's NOBJ table rows in LDS.
__device__ __forceinline__ int cs_carried(const ShapeData *__restrict__ S, const int s, const float *rows, unsigned &mask, float &rho) {
    if (S->otype[s] != 2) return -1;
    const float *ar = rows + min(max(S->oidx[s], 0), NOBJ - 1) * ATT_ROW;
    const int at = min(max(__float_as_int(ar[ATT_BODY]), 0), NB);
    if (at == 0) return -1;
    mask = sw_joint_mask(1, at - 1);
    rho = cs_rho(ar, S->sphere[s]);
    return at - 1;
}

template <bool CARRY>
__global__ void __launch_bounds__(SWEEP_THREADS) k_swept_clearance(BodyParams B, SimParams P, DevPtrs D, const DistTable *__restrict__ tab, int Q,
                                                                const SweepReach *__restrict__ reach, const float *__restrict__ segments /*[N][K][2][11]*/, int K,
                                                                float safety, float tolerance,
                                                                float *__restrict__ out_stop /*[N][K][12]*/, float4 *__restrict__ out_hit /*[N][K][3]*/,
                                                                int4 *__restrict__ out_id /*[N][K]*/, float *__restrict__ out_free /*[N][K][Q]*/,
                                                                const float *__restrict__ att /*[N][NOBJ][ATT_ROW]; null and unread without CARRY*/,
                                                                const SweepChain *__restrict__ chain /*null and unread without CARRY*/) {
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
    __shared__ float s_att[CARRY ? NOBJ * ATT_ROW : 1];                // the env's table rows, a one-env table for carry_stage_object (never named without CARRY: no LDS then)
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
    if constexpr (CARRY) {
        for (int i = tid; i < NOBJ * ATT_ROW; i += SWEEP_THREADS) s_att[i] = att[(size_t)env * (NOBJ * ATT_ROW) + i];
    }
    if (tid == 0) { s_t = 0.0f; s_mode = 0; s_steps = 0; s_evals = 0; s_ndue = Q; }
    __syncthreads();
    if (!CARRY && tid >= 1 && tid < 1 + NOBJ) {                       // (carried objects are staged at every step instead: phase 2)
        const int o = tid - 1;
        const m3 Ro = nc::quat_to_m3(s_st[20 + 4 * o][0], s_st[21 + 4 * o][0], s_st[22 + 4 * o][0], s_st[23 + 4 * o][0]);
        float *ob = s_ob[0] + 12 * o;
#pragma unroll
        for (int k = 0; k < 9; k++) ob[k] = Ro.m[k];
        ob[9] = s_st[11 + 3 * o][0]; ob[10] = s_st[12 + 3 * o][0]; ob[11] = s_st[13 + 3 * o][0];
    }
    for (int j = tid; j < Q; j += SWEEP_THREADS) {
        const int sa = min(max(tab->a[j], 0), MAXSHAPES - 1), sb = min(max(tab->b[j], 0), MAXSHAPES - 1);
        unsigned ma = sw_joint_mask(S->otype[sa], S->oidx[sa]), mb = sw_joint_mask(S->otype[sb], S->oidx[sb]);
        float bsum = 0.0f;
        if constexpr (CARRY) {
            float rho_a = 0.0f, rho_b = 0.0f;
            const int ca = cs_carried(S, sa, s_att, ma, rho_a), cb = cs_carried(S, sb, s_att, mb, rho_b);
            const unsigned one = ma ^ mb;
            for (int k = 0; k < NB; k++) {
                // (like R[k][s], a carried shape's reach is 0 where joint k does not move it: the other shape's joints see a point at rest)
                const float ra = ca >= 0 ? (((ma >> k) & 1u) ? chain->c[k][ca] + rho_a : 0.0f) : reach->r[k][sa];
                const float rb = cb >= 0 ? (((mb >> k) & 1u) ? chain->c[k][cb] + rho_b : 0.0f) : reach->r[k][sb];
                const float term = fabsf(s_dq[k]) * (ra + rb);
                bsum += ((one >> k) & 1u) ? term : 0.0f;
            }
        } else {
            const unsigned one = ma ^ mb;
            for (int k = 0; k < NB; k++) {
                const float term = fabsf(s_dq[k]) * (reach->r[k][sa] + reach->r[k][sb]);
                bsum += ((one >> k) & 1u) ? term : 0.0f;
            }
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
            if constexpr (CARRY) {
                if (tid >= 1 && tid < 1 + NOBJ) carry_stage_object(s_att, 0, tid - 1, s_st, s_fr[0], s_ob[0]);
                __syncthreads();
            }
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
