// rr_pkin.inc -- part of realrobot.hip (included there, behind rr_kin.inc; not a stand-alone translation unit).
// k_posture_kinematics: the link poses, the point positions and the 6 x 11 point Jacobians at K candidate joint postures per env of the
// whole batch (rr_posture_kinematics, realrobot.h): what k_kinematics writes into RR_KIN_LINK_POSE, RR_KIN_POINT_POS and RR_KIN_JACOBIAN if
// the env's joints were the candidate.  Read-only on the simulation: it reads the tensor, the model constants and the points (a kernel
// argument), never D.state or the preparation record; launched by rr_posture_kinematics alone, never by a step.
//
// A row is a posture (e, k); the N * K rows of [N, K, 11] are one flat list, and so are the rows of the three outputs.  PK_ROWS
// consecutive rows per 256-thread workgroup; 11 floats in and 146 (one point) .. 671 (eight) floats out per row.  The four phases of
// k_kinematics without its velocity fields, a barrier behind each of the first three, every thread at every barrier (a row behind the
// list's end reads the last row's posture and stores nothing):
//   1  all threads: the 11 floats of the workgroup's rows into LDS -- PK_ROWS * 11 consecutive floats of the tensor, one coalesced
//      read --, and per link / point its URDF link and the 11-bit mask of the joints that move it (KIN_ANC, PARENT at compile time);
//   2  threads 0 .. PK_ROWS-1 (one wave): the forward kinematics of one row each -- k_kinematics' phase 2 restated, fk_all's operations
//      in its order (the nc:: twins, det_sincosf), the serial chain of eleven frames as a loop that reads the parent's frame back from
//      the lane's LDS record -- R, p and world axes into LDS (the layout of k_kinematics: KIN_FR, an odd stride);
//   3  one thread per (row, link or point): the expression of k_link_poses for the link's COM frame; quaternion and world position
//      staged in LDS, once;
//   4  all threads walk each field's span of the workgroup's rows -- PK_ROWS consecutive rows: one contiguous run of floats that starts
//      on a 32-byte boundary for every row length, PK_ROWS being a multiple of 8 -- as float4, scalar stores for the ragged end of the
//      last workgroup only.  One output float is a function of (row, index in the row) and the LDS records alone; kin_column is
//      k_kinematics' own: column k of a point at x is [a_k x (x - p_k); a_k] if joint k moves the point's link, +0.0 otherwise.
// A candidate equal to the env's present joints gets the bits of k_kinematics (the tests assert it).  No atomics; nothing indexes
// memory by a value of the tensor: a non-finite posture gets non-finite rows like any other's.  Loop bounds are constants, the row
// count and the point count.
#ifndef PK_ROWS
#define PK_ROWS 16           // rows per workgroup: a multiple of 8 (phase 4's alignment), at most 64 (phase 2 is one wave); DESIGN.md has the measurements
#endif
#define PK_THREADS 256
static_assert(PK_ROWS % 8 == 0 && PK_ROWS >= 8 && PK_ROWS <= 64, "the spans of phase 4 start on 32-byte boundaries; phase 2 runs on one wave");
static_assert(PK_ROWS * RR_KIN_MAX_POINTS * 8 < 65536, "phase 4: the 16-bit reciprocal of the point count is exact below 65536 / 8");
static_assert(PK_THREADS == KIN_THREADS, "phase 4 stores with kin_store");

struct PkOut { float *link_pose, *point_pos, *jacobian; };

__global__ void __launch_bounds__(PK_THREADS) k_posture_kinematics(BodyParams B, const RenderModel *RMp, const float *__restrict__ postures /*[rows][11]*/,
                                                                  int rows, PkOut O, KinPoints pts, int np) {
    static_assert(ST_Q == 0, "the chain reads joint b of a row from column b of the tensor");
    __shared__ float s_q[PK_ROWS * NB];
    __shared__ float s_fr[PK_ROWS][KIN_FR];
    __shared__ float s_x[PK_ROWS][KIN_ITEMS][3];          // world position of a link's COM frame (0 .. KIN_LINKS-1) / of a point
    __shared__ float s_quat[PK_ROWS][KIN_LINKS][4];
    __shared__ unsigned s_mask[KIN_ITEMS];
    __shared__ int s_link[KIN_ITEMS], s_body[KIN_ITEMS];   // of a link / point: its URDF link, and that link's moving body (< 0: rigid with the world)
    __shared__ float s_local[RR_KIN_MAX_POINTS][3];
    const RenderModel &RM = *RMp;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * PK_ROWS;
    const int nr = (int)min((size_t)PK_ROWS, (size_t)rows - row0);      // live rows of this workgroup (>= 1 by the grid)
    const int ni = KIN_LINKS + np;
    // 1
    for (int i = tid; i < PK_ROWS * NB; i += PK_THREADS) s_q[i] = postures[min(row0 + i / NB, (size_t)rows - 1) * NB + i % NB];
    if (tid < ni) {
        // (the points are a kernel argument: every entry is read at a compile-time index and the VALUE is selected)
        int pl = 0;
#pragma unroll
        for (int j = 0; j < RR_KIN_MAX_POINTS; j++) pl = tid - KIN_LINKS == j ? pts.link[j] : pl;
        const int l = tid < KIN_LINKS ? tid : min(max(pl, 0), KIN_LINKS - 1);
        // link_body < NB is checked on the host (rr_posture_kinematics refuses another model); the min only keeps phase 3's LDS index
        // in range whatever the blob says.  The compile-time table is read by a compare chain: a body without a match has no mask.
        const int b = min(RM.link_body[l], NB - 1);
        unsigned mask = 0u;
#pragma unroll
        for (int bb = 0; bb < NB; bb++) mask = b == bb ? KIN_ANC.m[bb] : mask;
        s_mask[tid] = mask;
        s_link[tid] = l;
        s_body[tid] = b;
    }
    if (tid >= 64 && tid < 64 + 3 * RR_KIN_MAX_POINTS) {
        float v = 0.0f;
#pragma unroll
        for (int j = 0; j < 3 * RR_KIN_MAX_POINTS; j++) v = tid - 64 == j ? pts.local[j / 3][j % 3] : v;
        s_local[(tid - 64) / 3][(tid - 64) % 3] = v;
    }
    __syncthreads();
    // 2
    if (tid < PK_ROWS) {
        // k_kinematics' phase 2: fk_all's operations in its order, as a LOOP over the bodies -- a parent comes before its children and
        // its frame is read back from this lane's LDS record; the floats are the same
        float *fr = s_fr[tid];
        const float *q = s_q + tid * NB;
        for (int b = 0; b < NB; b++) {
            const int p = PARENT[b];
            m3 Rp = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
            v3 pp = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]);
            if (p >= 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) Rp.m[k] = fr[9 * p + k];
                pp = mk(fr[KIN_FR_P + 3 * p], fr[KIN_FR_P + 3 * p + 1], fr[KIN_FR_P + 3 * p + 2]);
            }
            m3 jr;
#pragma unroll
            for (int k = 0; k < 9; k++) jr.m[k] = B.jrot[b][k];
            const m3 Rj = nc::mul(Rp, jr);
            const v3 ax = mk(B.axis[b][0], B.axis[b][1], B.axis[b][2]);
            const v3 pb = nc::add(pp, nc::mulv(Rp, mk(B.jpos[b][0], B.jpos[b][1], B.jpos[b][2])));
            const m3 Rb = nc::mul(Rj, nc::axis_angle(ax, q[ST_Q + b]));
            const v3 aw = nc::mulv(Rj, ax);
#pragma unroll
            for (int k = 0; k < 9; k++) fr[9 * b + k] = Rb.m[k];
            fr[KIN_FR_P + 3 * b] = pb.x; fr[KIN_FR_P + 3 * b + 1] = pb.y; fr[KIN_FR_P + 3 * b + 2] = pb.z;
            fr[KIN_FR_AX + 3 * b] = aw.x; fr[KIN_FR_AX + 3 * b + 1] = aw.y; fr[KIN_FR_AX + 3 * b + 2] = aw.z;
        }
    }
    __syncthreads();
    // 3
    for (int i = tid; i < PK_ROWS * ni; i += PK_THREADS) {
        const int e = i / ni, j = i - e * ni;
        const int l = s_link[j], b = s_body[j];
        m3 lr;
#pragma unroll
        for (int k = 0; k < 9; k++) lr.m[k] = RM.link_rot[l][k];
        const v3 lp = mk(RM.link_pos[l][0], RM.link_pos[l][1], RM.link_pos[l][2]);
        m3 R = lr;
        v3 p = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]) + lp;
        if (b >= 0) {
            const float *fr = s_fr[e];
            m3 Rb;
#pragma unroll
            for (int k = 0; k < 9; k++) Rb.m[k] = fr[9 * b + k];
            const v3 pb = mk(fr[KIN_FR_P + 3 * b], fr[KIN_FR_P + 3 * b + 1], fr[KIN_FR_P + 3 * b + 2]);
            R = mul(Rb, lr);
            p = mulv(Rb, lp) + pb;
        }
        if (j < KIN_LINKS) {
            float qq[4];
            m3_to_quat(R, qq);
            s_quat[e][j][0] = qq[0]; s_quat[e][j][1] = qq[1]; s_quat[e][j][2] = qq[2]; s_quat[e][j][3] = qq[3];
        } else {
            const float *lc = s_local[j - KIN_LINKS];
            p = p + mulv(R, mk(lc[0], lc[1], lc[2]));
        }
        s_x[e][j][0] = p.x; s_x[e][j][1] = p.y; s_x[e][j][2] = p.z;
    }
    __syncthreads();
    // 4
    // (row, point) = ej / np, ej % np for ej < PK_ROWS * np by a 16-bit reciprocal: exact, m * np - 65536 < np <= 8 and ej * 8 < 65536
    const unsigned rcp = (65536u + (unsigned)np - 1u) / (unsigned)np;
    kin_store(O.link_pose + row0 * (KIN_LINKS * 7), nr * (KIN_LINKS * 7), [&](int i) {
        const int el = i / 7, c = i % 7, e = el / KIN_LINKS, l = el % KIN_LINKS;
        return c < 3 ? s_x[e][l][c] : s_quat[e][l][c < 3 ? 0 : c - 3];
    });
    kin_store(O.point_pos + row0 * (size_t)(3 * np), nr * 3 * np, [&](int i) {
        const int ej = i / 3, c = i % 3, e = (int)(((unsigned)ej * rcp) >> 16), j = ej - e * np;
        return s_x[e][KIN_LINKS + j][c];
    });
    kin_store(O.jacobian + row0 * (size_t)(6 * NB * np), nr * 6 * NB * np, [&](int i) {
        const int ej = i / (6 * NB), r = i % (6 * NB), c = r / NB, k = r % NB, e = (int)(((unsigned)ej * rcp) >> 16), j = ej - e * np;
        const float v = kin_column(s_fr[e], s_x[e][KIN_LINKS + j], k, c);
        return ((s_mask[KIN_LINKS + j] >> k) & 1u) ? v : 0.0f;
    });
}
