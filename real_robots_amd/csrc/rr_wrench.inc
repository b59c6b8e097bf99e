// rr_wrench.inc -- part of realrobot.hip (included there, behind rr_torque.inc; not a stand-alone translation unit).
// External wrenches of the step (rr_set_external_wrenches, realrobot.h): the handle holds a table w f32 [N][14][6] -- rows 0..10 the
// eleven moving robot bodies (row j: the body joint j moves, the rows of S_BR), rows 11..13 the objects --, a row {Fx, Fy, Fz, Tx, Ty,
// Tz} in the WORLD frame, the force at the body's centre of mass, the torque about it.  While wrenches are set every rr_step launches
// k_ext_wrench in front of its solve, behind k_joint_torque.
//
// k_ext_wrench.  A force is linear in the unconstrained velocities the preparation leaves in the env's record, so -- like the joint
// torques (rr_torque.inc) -- the step adds its term to the record behind the preparation: no existing kernel changes, the look-ahead
// stays valid when the table changes every step.
//   object i:  v*' = v* + dt F / m_i,  w*' = w* + dt Iinv_i T      m_i the env's own mass (D.obj_dyn), Iinv_i the record's S_OIINV: the
//              world inverse inertia of the pose that counts (the home pose for an object the out-of-bounds rule sends home);
//   robot:     tau_k = sum over the bodies b that joint k moves of a_k . ((c_b - p_k) x F_b + T_b),  c_b = p_b + R_b com_b,
//              a_k, p_k the record's S_BAX, S_BP;  qd*' = qd* + dt M^-1 tau, the product of k_joint_torque.
// One 16-lane group per env.  Lane b < 14 loads its body's row as one 24-byte span.  Robot lanes form c_b; lane k < 11 then sums its
// tau_k from 0.0f over b in ASCENDING order, the bodies' nine values {c, F, T} broadcast within the group, which bodies it sums over
// a compile-time mask from PARENT; then sum_j M^-1[k][j] tau[j] from 0.0f in ascending j with fused multiply-adds.  Object lanes do
// their three-by-three product and two stores.  No atomics, no LDS, no value of the table forms an address: an env's result depends
// on its own record and rows alone.
// Table layout: [N][14][6] compact, the layout of the ABI -- the zero-copy view is the table itself.
// Not touched (the zero rule, per target, decided from the group's ballot before any store): S_QDS of an env whose eleven robot rows
// are all zero (either sign; a NaN is not zero), S_OVS / S_OWS of an object whose row is zero, everything of a frozen env (errflags &
// 1: the preparation has not written its record).  The rows of objects the handle does not have are never read.
#define XW_THREADS 256       // sixteen envs per workgroup
static_assert(XW_THREADS % 64 == 0 && RR_XW_BODIES == NB + NOBJ && RR_XW_BODIES <= 16, "whole waves of four 16-lane groups; a body per lane");

// bit b of xw_moved(k): joint k moves body b (b is k or one of its descendants in PARENT)
__host__ __device__ constexpr unsigned xw_moved(int k) {
    unsigned m = 0;
    for (int b = 0; b < NB; b++) {
        int a = b;
        while (a >= 0 && a != k) a = PARENT[a];
        if (a == k) m |= 1u << b;
    }
    return m;
}
static_assert(xw_moved(0) == 0x7ffu && xw_moved(6) == 0x7c0u && xw_moved(7) == 0x180u && xw_moved(8) == 0x100u && xw_moved(9) == 0x600u && xw_moved(10) == 0x400u,
              "chain 0..6, fingers 7 -> 8 and 9 -> 10 from body 6");

__global__ void __launch_bounds__(XW_THREADS) k_ext_wrench(SimParams P, DevPtrs D, const float *__restrict__ table /*[N][14][6]*/) {
    const int l = threadIdx.x & 15;
    const int env = (int)((blockIdx.x * (unsigned)XW_THREADS + threadIdx.x) >> 4);
    const bool in = env < P.N;
    const bool has_row = in && l < NB + P.nobj;      // (the rows of objects the handle does not have are never read)
    float2 w0 = make_float2(0.0f, 0.0f), w1 = w0, w2 = w0;
    if (has_row) {
        const float2 *row = (const float2 *)(table + ((size_t)env * RR_XW_BODIES + l) * 6);      // (24-byte rows: 8-byte aligned)
        w0 = row[0]; w1 = row[1]; w2 = row[2];
    }
    const v3 F = mk(w0.x, w0.y, w1.x), T = mk(w1.y, w2.x, w2.y);
    // the group's sixteen bits of the wave's ballot: the rows with an entry that is not +-0 (a NaN counts: it is not zero)
    const bool mine = F.x != 0.0f || F.y != 0.0f || F.z != 0.0f || T.x != 0.0f || T.y != 0.0f || T.z != 0.0f;
    const unsigned long long nz = __ballot(mine);
    const unsigned grp = (unsigned)(nz >> (threadIdx.x & 48)) & 0xffffu;
    if (!in || grp == 0u || (D.errflags[env] & 1u)) return;      // (uniform in the group: the broadcasts below see all sixteen lanes)
    float *scratch = D.scratch;
    const float dt = P.dt;
    if (l >= NB && mine) {      // ---- an object lane with a non-zero row
        const int i = l - NB;
        const float m = D.obj_dyn[(size_t)(4 * i) * P.N + env];
        const float *I = &SCR(S_OIINV + 9 * i);
        const v3 a = mk(I[0] * T.x + I[1] * T.y + I[2] * T.z, I[3] * T.x + I[4] * T.y + I[5] * T.z, I[6] * T.x + I[7] * T.y + I[8] * T.z);
        SCR(S_OVS + 3 * i) += dt * F.x / m; SCR(S_OVS + 3 * i + 1) += dt * F.y / m; SCR(S_OVS + 3 * i + 2) += dt * F.z / m;
        SCR(S_OWS + 3 * i) += dt * a.x; SCR(S_OWS + 3 * i + 1) += dt * a.y; SCR(S_OWS + 3 * i + 2) += dt * a.z;
    }
    if ((grp & ((1u << NB) - 1u)) == 0u) return;      // all eleven robot rows zero: S_QDS keeps its bits (uniform in the group)
    // ---- the robot: lane b's centre of mass, lane k's joint
    const int lb = l < NB ? l : 0;      // (lanes 11..15 alias body 0; they store nothing and nobody reads them)
    const float *bt = D.body_tab + lb * BT_STRIDE + BT_COM;
    const float *R = &SCR(S_BR + 9 * lb);
    const v3 p = mk(SCR(S_BP + 3 * lb), SCR(S_BP + 3 * lb + 1), SCR(S_BP + 3 * lb + 2));
    const v3 ax = mk(SCR(S_BAX + 3 * lb), SCR(S_BAX + 3 * lb + 1), SCR(S_BAX + 3 * lb + 2));
    const v3 com = mk(bt[0], bt[1], bt[2]);
    const v3 c = mk(p.x + (R[0] * com.x + R[1] * com.y + R[2] * com.z), p.y + (R[3] * com.x + R[4] * com.y + R[5] * com.z),
                    p.z + (R[6] * com.x + R[7] * com.y + R[8] * com.z));
    unsigned moved = 0u;
#pragma unroll
    for (int k = 0; k < NB; k++) moved = l == k ? xw_moved(k) : moved;
    // (lane b of the group is lane (threadIdx.x & 48) + b of the wave; the builtin, not __shfl: see rr_torque.inc)
    const int grp_addr = (int)(threadIdx.x & 48u) << 2;
#define XW_BCAST(b, v) __int_as_float(__builtin_amdgcn_ds_bpermute(grp_addr + 4 * (b), __float_as_int(v)))
    float tau = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const v3 cb = mk(XW_BCAST(b, c.x), XW_BCAST(b, c.y), XW_BCAST(b, c.z));
        const v3 Fb = mk(XW_BCAST(b, F.x), XW_BCAST(b, F.y), XW_BCAST(b, F.z));
        const v3 Tb = mk(XW_BCAST(b, T.x), XW_BCAST(b, T.y), XW_BCAST(b, T.z));
        const float term = dot(ax, cross(cb - p, Fb) + Tb);
        tau = (moved >> b) & 1u ? tau + term : tau;
    }
    const float *mrow = &SCR(S_MINV + lb * NB);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; j++) acc = __builtin_fmaf(mrow[j], XW_BCAST(j, tau), acc);
#undef XW_BCAST
    if (l < NB) SCR(S_QDS + l) += dt * acc;
}

// The table's rows of the masked envs from a caller's tensor [N][14][6] (src == nullptr: zeros), one thread per entry.
__global__ void __launch_bounds__(256) k_ext_wrench_set(int N, const float *__restrict__ src /*[N][14][6] or nullptr*/,
                                                        const unsigned char *__restrict__ mask /*[N] or nullptr: all*/, float *__restrict__ table) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N * (RR_XW_BODIES * 6)) return;
    if (mask && !mask[i / (RR_XW_BODIES * 6)]) return;
    table[i] = src ? src[i] : 0.0f;
}
