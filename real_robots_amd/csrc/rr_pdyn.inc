// rr_pdyn.inc -- part of realrobot.hip (included there, behind rr_pkin.inc; not a stand-alone translation unit).
// k_posture_dynamics: the joint-space dynamics at K candidate joint postures per env of the whole batch (rr_posture_dynamics,
// realrobot.h): the mass matrix M(q), the gravity torques G(q), the bias G + C(q, qd), the inverse dynamics M qdd + bias and, on
// request, M^-1.  Read-only on the simulation: it reads the tensors (or, in the present-state form, the joint columns of D.state), the
// model constants and the handle's body table, never the preparation record; launched by rr_posture_dynamics alone, never by a step.
//
// A row is a posture (e, k); the N * K rows of [N, K, 11] are one flat list, and so are the rows of the five outputs.  The layout is
// k_prep_b16's: sixteen lanes per row, four rows per wave, everything per body on the lane of that body (lanes 0..10), the tree sums
// by DPP inside the 16-lane row -- no value ever crosses from one row's lanes to another's.  The arithmetic is prep16_body's joint-space
// part, COPIED here (rr_prep.inc is untouched: the preparation's kernels keep their instructions): the chain of frames, the composite
// bodies, column j of the mass matrix on lane j, the Newton-Euler bias along the lane's own root path with the force pass as subtree
// sums, the Cholesky factor and the columns of M^-1.  Its small helpers (p16_merge, the P16_*_BCAST macros, P16_SYNC, the PL_* record)
// are used as they are.  What differs from the preparation:
//   * q, qd, qdd come from the tensors, nothing from the env's state (present-state form: q and qd from the state's columns, by stride);
//   * the gravity torques are a pass of their own with w = al = 0 (a body's force is m g z, its torque r x F) through the same force
//     pass; without velocities `bias` IS that value (one register, the same bytes), without accelerations `torque` IS `bias`;
//   * M is mirrored: lane j writes M[j][i] and M[i][j] for its ancestors-or-self i -- one value, two places: symmetric bit for bit --
//     and +0.0 where i is neither an ancestor nor a descendant of j (the two finger branches); every entry is written exactly once;
//   * no joint damping, no motors, no unconstrained velocities;
//   * the Cholesky factor and M^-1 only in the instantiation with INV.
// Outputs.  A row's LDS record (PL_TOTAL floats) is dead part by part as the row goes on, and the outputs are staged into the dead
// parts: M over the local joint rotations (PL_RAA), M^-1 over the composite bodies (PL_CI, PL_CC), the three vectors and qdd in the
// slot of the preparation's M^-1 rows (PL_X).  Behind one workgroup barrier all threads store each field's span of the workgroup's
// PD_ROWS consecutive rows -- one contiguous run that starts on a 16-byte boundary, PD_ROWS being a multiple of 4 -- as float4, scalar
// stores for the ragged end of the last workgroup only (k_posture_kinematics' phase 4).
// Every thread reaches every barrier; a row behind the list's end computes the last row again and stores nothing.  No atomics; nothing
// indexes memory by a value of the tensors: a non-finite row gets non-finite outputs like any other's.  Loop bounds are constants and
// the row count.
#ifndef PD_ROWS
#define PD_ROWS 16           // rows per workgroup: a multiple of 4 (whole waves; the spans of the store phase start on 16-byte boundaries)
#endif
#define PD_THREADS (16 * PD_ROWS)
static_assert(PD_ROWS % 4 == 0 && PD_ROWS >= 4 && PD_THREADS <= 1024, "whole waves of four rows; a field's span of a workgroup starts on a 16-byte boundary");
// the staged outputs inside a row's record
enum { PD_M = PL_RAA, PD_MINV = PL_CI, PD_G = PL_X, PD_B = PL_X + NB, PD_T = PL_X + 2 * NB, PD_QDD = PL_X + 3 * NB };
static_assert(NB * NB <= PL_CI - PL_RAA && NB * NB <= PL_X - PL_CI && 4 * NB <= PL_TOTAL - PL_X, "the staged outputs fit the dead parts of the record");

// q / qd of row r, joint j at [r * rs + j * cs]: (11, 1) for a tensor [rows][11], (1, N) for the joint columns of the state; qdd is
// always a tensor [rows][11].  qd / qdd may be null: zero.
struct PdIn { const float *q, *qd, *qdd; size_t rs, cs; };
struct PdOut { float *mass, *gravity, *bias, *torque, *minv; };

template <typename F>
__device__ __forceinline__ void pd_store(float *__restrict__ dst, int n, F f) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += PD_THREADS) ((float4 *)dst)[i] = make_float4(f(4 * i), f(4 * i + 1), f(4 * i + 2), f(4 * i + 3));
    for (int i = 4 * n4 + threadIdx.x; i < n; i += PD_THREADS) dst[i] = f(i);
}

// RNEA's force pass of prep16_body as subtree sums: a body's force F and its torque Nn about its own joint, referred to the wrist
// (body 6's joint at o), summed over the body's subtree leaf to root -- a tree edge child -> parent is "lane l takes lane l + 1"
// (row_shl:1) except 9 -> 6 --, then referred back to the body's own joint and projected on its axis.
__device__ __forceinline__ float pd_force_pass(int l, v3 F, v3 Nn, v3 bp, v3 bax, v3 o) {
    const v3 ro = bp - o;
    const v3 G = Nn + cross(ro, F);
    float s0 = l < NB ? F.x : 0.0f, s1 = l < NB ? F.y : 0.0f, s2 = l < NB ? F.z : 0.0f, s3 = l < NB ? G.x : 0.0f, s4 = l < NB ? G.y : 0.0f, s5 = l < NB ? G.z : 0.0f;
#define PD_EDGE(DPP, MASK)                                                                                          \
    {                                                                                                               \
        const float m_ = (MASK) ? 1.0f : 0.0f;                                                                      \
        asm("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %6 " DPP " row_mask:0xf bank_mask:0xf\n\tv_fmac_f32_dpp %1, %1, %6 " DPP " row_mask:0xf bank_mask:0xf\n\t" \
            "v_fmac_f32_dpp %2, %2, %6 " DPP " row_mask:0xf bank_mask:0xf\n\tv_fmac_f32_dpp %3, %3, %6 " DPP " row_mask:0xf bank_mask:0xf\n\t"           \
            "v_fmac_f32_dpp %4, %4, %6 " DPP " row_mask:0xf bank_mask:0xf\n\tv_fmac_f32_dpp %5, %5, %6 " DPP " row_mask:0xf bank_mask:0xf"               \
            : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4), "+v"(s5) : "v"(m_));                                \
    }
    PD_EDGE("row_shl:1", l == 9 || l == 7)          // 10 -> 9, 8 -> 7
    PD_EDGE("row_newbcast:9", l == 6)               // 9 -> 6
    PD_EDGE("row_shl:1", l == 6)                    // 7 -> 6
    PD_EDGE("row_shl:1", l == 5) PD_EDGE("row_shl:1", l == 4) PD_EDGE("row_shl:1", l == 3) PD_EDGE("row_shl:1", l == 2)
    PD_EDGE("row_shl:1", l == 1) PD_EDGE("row_shl:1", l == 0)
#undef PD_EDGE
    const v3 Nt = mk(s3, s4, s5) - cross(ro, mk(s0, s1, s2));
    return dot(bax, Nt);
}

template <bool INV>
__global__ void __launch_bounds__(PD_THREADS) k_posture_dynamics(BodyParams B, const float *__restrict__ body_tab, float gravity, PdIn I, int rows, PdOut O) {
    __shared__ __attribute__((aligned(16))) float s_pd[PD_ROWS * PL_TOTAL];
    const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
    const size_t row0 = (size_t)blockIdx.x * PD_ROWS;
    const int nr = (int)min((size_t)PD_ROWS, (size_t)rows - row0);      // live rows of this workgroup (>= 1 by the grid)
    const size_t row = min(row0 + grp, (size_t)rows - 1);               // a group behind the list's end runs along on the last row
    float *lds = s_pd + grp * PL_TOTAL;
    const int lb = l < NB ? l : 0;                          // the body of this lane (lanes 11..15 alias body 0; they stage nothing)
    const bool has_vel = I.qd != nullptr, has_acc = I.qdd != nullptr;
    // ---- stage-in: the lane's joint, its body's constants
    const float q_l = I.q[row * I.rs + lb * I.cs];
    const float qd_l = has_vel ? I.qd[row * I.rs + lb * I.cs] : 0.0f;
    const float qdd_l = has_acc ? I.qdd[row * NB + lb] : 0.0f;
    const float4 *bt = (const float4 *)(body_tab + lb * BT_STRIDE);
    const float4 t0 = bt[0], t1 = bt[1], t2 = bt[2], t3 = bt[3];
    const v3 com_l = mk(t0.x, t0.y, t0.z);
    const float inertia_l[6] = {t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
    const float mass_l = t2.y;
    const v3 axis_l = mk(t2.w, t3.x, t3.y);
    // ---- the local rotation of this lane's joint, to LDS for the chain
    {
        const m3 raa = nc::axis_angle(axis_l, q_l);
        if (l < NB) {
            float4 *ra4 = (float4 *)&lds[PL_RAA + 12 * l];
            ra4[0] = make_float4(raa.m[0], raa.m[1], raa.m[2], raa.m[3]);
            ra4[1] = make_float4(raa.m[4], raa.m[5], raa.m[6], raa.m[7]);
            ra4[2] = make_float4(raa.m[8], 0.0f, 0.0f, 0.0f);
            lds[PL_BQ + 8 * l + 3] = qd_l;
            lds[PD_QDD + l] = qdd_l;
        }
    }
    P16_SYNC();
    // ---- forward kinematics: row r of the frame at hand on lane r (chain A: lanes 0..2, and every other lane redundantly;
    // chain B: lanes 3..5 from the fork at body 6 on); fk_all's operations in its order, contraction-free
    {
        const int r = l % 3;
        const bool chB = l >= 3 && l < 6;
        float a0 = r == 0 ? 1.0f : 0.0f, a1 = r == 1 ? 1.0f : 0.0f, a2 = r == 2 ? 1.0f : 0.0f;
        float pr = r == 0 ? B.robot_pos[0] : (r == 1 ? B.robot_pos[1] : B.robot_pos[2]);
#define PD_LEVEL(BA, BB)                                                                                                       \
        {                                                                                                                      \
            float jr[9], jp[3], ax[3];                                                                                         \
            _Pragma("unroll") for (int k = 0; k < 9; k++) jr[k] = (BA) == (BB) ? B.jrot[BA][k] : (chB ? B.jrot[BB][k] : B.jrot[BA][k]); \
            _Pragma("unroll") for (int k = 0; k < 3; k++) {                                                                    \
                jp[k] = (BA) == (BB) ? B.jpos[BA][k] : (chB ? B.jpos[BB][k] : B.jpos[BA][k]);                                  \
                ax[k] = (BA) == (BB) ? B.axis[BA][k] : (chB ? B.axis[BB][k] : B.axis[BA][k]);                                  \
            }                                                                                                                  \
            const int body = chB ? (BB) : (BA);                                                                                \
            const float4 *ra4 = (const float4 *)&lds[PL_RAA + 12 * body];                                                      \
            const float4 ra0 = ra4[0], ra1 = ra4[1];                                                                           \
            const float ra8 = lds[PL_RAA + 12 * body + 8];                                                                     \
            const float j0 = nc::row3(a0, a1, a2, jr[0], jr[3], jr[6]), j1 = nc::row3(a0, a1, a2, jr[1], jr[4], jr[7]),        \
                        j2 = nc::row3(a0, a1, a2, jr[2], jr[5], jr[8]);                                                        \
            const float pb = nc::add1(pr, nc::row3(a0, a1, a2, jp[0], jp[1], jp[2]));                                          \
            const float r0 = nc::row3(j0, j1, j2, ra0.x, ra0.w, ra1.z), r1 = nc::row3(j0, j1, j2, ra0.y, ra1.x, ra1.w),        \
                        r2 = nc::row3(j0, j1, j2, ra0.z, ra1.y, ra8);                                                          \
            const float aw = nc::row3(j0, j1, j2, ax[0], ax[1], ax[2]);                                                        \
            if (l < 3 || (chB && (BA) != (BB))) {                                                                              \
                lds[PL_R + 9 * body + 3 * r] = r0; lds[PL_R + 9 * body + 3 * r + 1] = r1; lds[PL_R + 9 * body + 3 * r + 2] = r2; \
                lds[PL_BQ + 8 * body + r] = aw; lds[PL_BQ + 8 * body + 4 + r] = pb;                                            \
            }                                                                                                                  \
            a0 = r0; a1 = r1; a2 = r2; pr = pb;                                                                                \
        }
        PD_LEVEL(0, 0) PD_LEVEL(1, 1) PD_LEVEL(2, 2) PD_LEVEL(3, 3) PD_LEVEL(4, 4) PD_LEVEL(5, 5) PD_LEVEL(6, 6)
        PD_LEVEL(7, 9) PD_LEVEL(8, 10)
#undef PD_LEVEL
    }
    P16_SYNC();
    // ---- per body: frame, centre of mass, world inertia (lane b)
    m3 bR; v3 bp, bax;
    {
#pragma unroll
        for (int k = 0; k < 9; k++) bR.m[k] = lds[PL_R + 9 * lb + k];
        const float4 q0 = *(const float4 *)&lds[PL_BQ + 8 * lb], q1 = *(const float4 *)&lds[PL_BQ + 8 * lb + 4];
        bax = mk(q0.x, q0.y, q0.z); bp = mk(q1.x, q1.y, q1.z);
    }
    const v3 bcom = bp + mulv(bR, com_l);
    const m3 bI = inertia_world(bR, inertia_l);
    // ---- composite bodies, leaf to root: the nodes go to LDS (lane b), then nine lanes hold one inertia entry each
    if (l < NB) {
#pragma unroll
        for (int k = 0; k < 9; k++) lds[PL_CI + 9 * l + k] = bI.m[k];
        *(float4 *)&lds[PL_CC + 4 * l] = make_float4(bcom.x, bcom.y, bcom.z, mass_l);
    }
    P16_SYNC();
    {
        const int e9 = l < 9 ? l : 0, ei = e9 / 3, ej = e9 % 3;
        auto node = [&](int b) { const float4 c = *(const float4 *)&lds[PL_CC + 4 * b]; P16Comp n; n.m = c.w; n.c = mk(c.x, c.y, c.z); n.I = lds[PL_CI + 9 * b + e9]; return n; };
        auto put = [&](int b, const P16Comp &n) { if (l < 9) lds[PL_CI + 9 * b + e9] = n.I; if (l == 0) *(float4 *)&lds[PL_CC + 4 * b] = make_float4(n.c.x, n.c.y, n.c.z, n.m); };
        // (every child into its parent, in the order of a loop b = 10 .. 1 over PARENT: 10 -> 9, 9 -> 6, 8 -> 7, 7 -> 6, 6 -> 5, ... 1 -> 0)
        const P16Comp n9 = p16_merge(node(9), node(10), ei, ej);
        P16Comp n6 = p16_merge(node(6), n9, ei, ej);
        const P16Comp n7 = p16_merge(node(7), node(8), ei, ej);
        n6 = p16_merge(n6, n7, ei, ej);
        put(9, n9); put(7, n7); put(6, n6);
        P16Comp acc = n6;
#pragma unroll
        for (int b = 5; b >= 0; b--) { acc = p16_merge(node(b), acc, ei, ej); put(b, acc); }
    }
    P16_SYNC();
    // ---- mass matrix: lane j computes M[i][j] = M[j][i] for the ancestors-or-self i of j -- row j of the lower triangle -- and
    // stages it mirrored (PD_M lies over PL_RAA, which nothing reads behind the chain)
    float Mrow[NB];
    {
        m3 cI;
#pragma unroll
        for (int k = 0; k < 9; k++) cI.m[k] = lds[PL_CI + 9 * lb + k];
        const float4 c4 = *(const float4 *)&lds[PL_CC + 4 * lb];
        const v3 cc = mk(c4.x, c4.y, c4.z);
        const float cm = c4.w;
        const unsigned anc = lb <= 6 ? (2u << lb) - 1u : (lb == 7 ? 0x0ffu : (lb == 8 ? 0x1ffu : (lb == 9 ? 0x27fu : 0x67fu)));
        // the bodies joint lb moves: itself and its descendants
        const unsigned desc = lb <= 6 ? 0x7ffu & ~((1u << lb) - 1u) : (lb == 7 ? 0x180u : (lb == 8 ? 0x100u : (lb == 9 ? 0x600u : 0x400u)));
        const v3 Ia = mulv(cI, bax);
        const v3 f = cross(bax, cc - bp) * cm;
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const float4 q0 = *(const float4 *)&lds[PL_BQ + 8 * i], q1 = *(const float4 *)&lds[PL_BQ + 8 * i + 4];      // body i: axis, position
            const v3 nn = Ia + cross(cc - mk(q1.x, q1.y, q1.z), f);
            const float v = dot(mk(q0.x, q0.y, q0.z), nn);
            Mrow[i] = ((anc >> i) & 1u) ? v : 0.0f;
        }
        if (l < NB) {
#pragma unroll
            for (int i = 0; i < NB; i++) {
                if ((anc >> i) & 1u) { lds[PD_M + NB * l + i] = Mrow[i]; lds[PD_M + NB * i + l] = Mrow[i]; }
                else if (!((desc >> i) & 1u)) lds[PD_M + NB * l + i] = 0.0f;
            }
        }
    }
    // ---- the body's own terms of the two Newton-Euler passes (base acceleration +g), then the force pass of each
    float grav_l, bias_l;
    {
        const float4 o4 = *(const float4 *)&lds[PL_BQ + 8 * 6 + 4];
        const v3 o = mk(o4.x, o4.y, o4.z);
        const v3 r = bcom - bp;
        {   // gravity: w = al = 0, every body's acceleration is (0, 0, g)
            const v3 F = mk(0.0f, 0.0f, gravity * mass_l);
            const v3 Nn = mk(r.y * F.z, -(r.x * F.z), 0.0f);        // r x F
            grav_l = pd_force_pass(l, F, Nn, bp, bax, o);
        }
        bias_l = grav_l;
        if (has_vel) {      // (uniform) the velocity recursion along this lane's own root path, level by level
            v3 w = mk(0, 0, 0), al = mk(0, 0, 0), ap = mk(0, 0, gravity), pp = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]);
            const int plen = lb <= 6 ? lb + 1 : (lb == 7 || lb == 9 ? 8 : 9);      // bodies on the path root .. b
            const bool second = lb >= 9;                                          // the path runs through body 9 (not 7)
#define PD_RNEA_LEVEL(K, BA, BB)                                                                                    \
            {                                                                                                       \
                const int node = (BA) == (BB) ? (BA) : (second ? (BB) : (BA));                                      \
                const float4 q0 = *(const float4 *)&lds[PL_BQ + 8 * node], q1 = *(const float4 *)&lds[PL_BQ + 8 * node + 4]; \
                const v3 ax_ = mk(q0.x, q0.y, q0.z), p_ = mk(q1.x, q1.y, q1.z);                                     \
                const float qd_ = q0.w;                                                                             \
                const v3 wn = w + ax_ * qd_;                                                                        \
                const v3 aln = al + cross(w, ax_) * qd_;                                                            \
                const v3 d = p_ - pp;                                                                               \
                const v3 apn = ap + cross(al, d) + cross(w, cross(w, d));                                           \
                const bool on = (K) < plen;                                                                         \
                w = p16_sel3(on, wn, w); al = p16_sel3(on, aln, al); ap = p16_sel3(on, apn, ap); pp = p16_sel3(on, p_, pp); \
            }
            PD_RNEA_LEVEL(0, 0, 0) PD_RNEA_LEVEL(1, 1, 1) PD_RNEA_LEVEL(2, 2, 2) PD_RNEA_LEVEL(3, 3, 3) PD_RNEA_LEVEL(4, 4, 4)
            PD_RNEA_LEVEL(5, 5, 5) PD_RNEA_LEVEL(6, 6, 6) PD_RNEA_LEVEL(7, 7, 9) PD_RNEA_LEVEL(8, 8, 10)
#undef PD_RNEA_LEVEL
            const v3 ac = ap + cross(al, r) + cross(w, cross(w, r));
            const v3 F = ac * mass_l;
            const v3 Nn = mulv(bI, al) + cross(w, mulv(bI, w)) + cross(r, F);
            bias_l = pd_force_pass(l, F, Nn, bp, bax, o);
        }
    }
    P16_SYNC();
    // ---- torque = M qdd + bias: row l of the mirrored M against the staged qdd, in a fixed order
    {
        float t = bias_l;
        if (has_acc) {      // (uniform)
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < NB; i++) s += lds[PD_M + NB * lb + i] * lds[PD_QDD + i];
            t = s + bias_l;
        }
        if (l < NB) { lds[PD_G + l] = grav_l; lds[PD_B + l] = bias_l; lds[PD_T + l] = t; }
    }
    if (INV) {
        // ---- Cholesky M = L L^T, row l of L on lane l, column by column (v_rsq_f32 for the diagonal: 1 ulp)
        float Lr[NB], idiag = 0.0f;
#define PD_CHOL_COL(J)                                                                               \
        {                                                                                            \
            float s = Mrow[J];                                                                       \
            _Pragma("unroll") for (int k = 0; k < (J); k++) P16_FNMAC_BCAST(J, s, Lr[k], Lr[k]);     \
            const float idj = __builtin_amdgcn_rsqf(s), dj = s * idj;                                \
            idiag = l == (J) ? idj : idiag;                                                          \
            float off;                                                                               \
            P16_MUL_BCAST(J, off, idj, s);                                                           \
            Lr[J] = l == (J) ? dj : (l > (J) ? off : 0.0f);                                          \
        }
        PD_CHOL_COL(0) PD_CHOL_COL(1) PD_CHOL_COL(2) PD_CHOL_COL(3) PD_CHOL_COL(4) PD_CHOL_COL(5) PD_CHOL_COL(6) PD_CHOL_COL(7)
        PD_CHOL_COL(8) PD_CHOL_COL(9) PD_CHOL_COL(10)
#undef PD_CHOL_COL
        // ---- M^-1: lane c solves L y = e_c, L^T x = y for column c (the factor's rows broadcast from their lanes, folded into the multiply-adds)
        float xc[NB], y[NB];
#define PD_FWD(I_)                                                                                   \
        {                                                                                            \
            float s = l == (I_) ? 1.0f : 0.0f;                                                       \
            _Pragma("unroll") for (int k = 0; k < (I_); k++) P16_FNMAC_BCAST(I_, s, Lr[k], y[k]);    \
            P16_MUL_BCAST(I_, y[I_], idiag, s);                                                      \
        }
        PD_FWD(0) PD_FWD(1) PD_FWD(2) PD_FWD(3) PD_FWD(4) PD_FWD(5) PD_FWD(6) PD_FWD(7) PD_FWD(8) PD_FWD(9) PD_FWD(10)
#undef PD_FWD
#define PD_BWD(I_)                                                                                   \
        {                                                                                            \
            float s = y[I_];                                                                         \
            if ((I_) < 1) P16_FNMAC_BCAST(1, s, Lr[I_], xc[1]);                                      \
            if ((I_) < 2) P16_FNMAC_BCAST(2, s, Lr[I_], xc[2]);                                      \
            if ((I_) < 3) P16_FNMAC_BCAST(3, s, Lr[I_], xc[3]);                                      \
            if ((I_) < 4) P16_FNMAC_BCAST(4, s, Lr[I_], xc[4]);                                      \
            if ((I_) < 5) P16_FNMAC_BCAST(5, s, Lr[I_], xc[5]);                                      \
            if ((I_) < 6) P16_FNMAC_BCAST(6, s, Lr[I_], xc[6]);                                      \
            if ((I_) < 7) P16_FNMAC_BCAST(7, s, Lr[I_], xc[7]);                                      \
            if ((I_) < 8) P16_FNMAC_BCAST(8, s, Lr[I_], xc[8]);                                      \
            if ((I_) < 9) P16_FNMAC_BCAST(9, s, Lr[I_], xc[9]);                                      \
            if ((I_) < 10) P16_FNMAC_BCAST(10, s, Lr[I_], xc[10]);                                   \
            P16_MUL_BCAST(I_, xc[I_], idiag, s);                                                     \
        }
        PD_BWD(10) PD_BWD(9) PD_BWD(8) PD_BWD(7) PD_BWD(6) PD_BWD(5) PD_BWD(4) PD_BWD(3) PD_BWD(2) PD_BWD(1) PD_BWD(0)
#undef PD_BWD
        // lane c holds column c: entry (i, c) (PD_MINV lies over the composite bodies, which nothing reads behind the mass matrix)
        if (l < NB) {
#pragma unroll
            for (int i = 0; i < NB; i++) lds[PD_MINV + NB * i + l] = xc[i];
        }
    }
    __syncthreads();
    // ---- all threads: each field's span of the workgroup's rows, float4 where whole
    auto mat = [&](int off) { return [=](int i) { const int e = i / (NB * NB); return s_pd[e * PL_TOTAL + off + (i - e * (NB * NB))]; }; };
    auto vec = [&](int off) { return [=](int i) { const int e = i / NB; return s_pd[e * PL_TOTAL + off + (i - e * NB)]; }; };
    pd_store(O.mass + row0 * (NB * NB), nr * (NB * NB), mat(PD_M));
    pd_store(O.gravity + row0 * NB, nr * NB, vec(PD_G));
    pd_store(O.bias + row0 * NB, nr * NB, vec(PD_B));
    pd_store(O.torque + row0 * NB, nr * NB, vec(PD_T));
    if (INV) pd_store(O.minv + row0 * (NB * NB), nr * (NB * NB), mat(PD_MINV));
}
