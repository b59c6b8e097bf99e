// rr_kin.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_kinematics: the kinematic side of the present state as whole-batch observations (rr_kinematic_observations, realrobot.h):
// joint velocities, the pose and the velocity of every URDF link's COM frame, object twists, and for up to RR_KIN_MAX_POINTS
// points (link, position in the link's COM frame) the world position, velocity and 6 x 11 geometric Jacobian -- pybullet's
// getJointState, getLinkState(computeLinkVelocity=1), getBaseVelocity and calculateJacobian.  Read-only on the simulation (it
// reads D.state, the model constants and the points, never the preparation record); launched by rr_kinematic_observations
// alone, never by a step.
//
// KIN_ENVS envs per 256-thread workgroup; 40 floats in and 325 (one point) .. 850 (eight) floats out per env.  Four phases, a
// barrier behind each of the first three, every thread at every barrier (an env behind the batch's end reads the last env's
// state and stores nothing):
//   1  all threads: the 40 state floats of the workgroup's envs into LDS (STT(slot) is [slot][N]: KIN_ENVS consecutive floats per
//      slot), and per link / point its URDF link and the 11-bit mask of the joints that move it (PARENT at compile time);
//   2  threads 0 .. KIN_ENVS-1: the forward kinematics of one env each -- fk_all's operations in its order, the serial chain of
//      eleven frames as a loop -- R, p and world axes into LDS;
//   3  one thread per (env, link or point): the expression of k_link_poses for the link's COM frame; the quaternion of a link and
//      the world position of a link / point are staged in LDS, once;
//   4  all threads walk each field's span of the workgroup's envs -- KIN_ENVS consecutive rows of [N, row]: one contiguous,
//      32-byte aligned run of floats -- as float4 (scalar stores only for the ragged end of the last workgroup).  One output
//      float is a function of (env, row index) and the LDS records alone:
//          column k of a point at x:  [a_k x (x - p_k); a_k] if joint k moves the point's link, +0.0 otherwise
//          velocity at x:             the sum over those k, ascending, of qd_k times that column, from +0.0
//      in plain float32; a link rigid with the world has an empty mask: all +0.0.  RR_KIN_JOINT_VEL and RR_KIN_OBJ_VEL are the
//      staged state floats, bit for bit.
// Nothing indexes memory by a state value: an env with a non-finite state gets non-finite rows like any other env's.
#define KIN_ENVS 8           // envs per workgroup (the spans of phase 4 then start on 32-byte boundaries for every row length); two workgroups per CU at 4096 envs
#define KIN_THREADS 256
#define KIN_LINKS 17         // URDF links: the rows of rr_link_poses (rr_kinematic_observations refuses another model)
#define KIN_ITEMS (KIN_LINKS + RR_KIN_MAX_POINTS)
#define KIN_ST 40            // staged state floats per env: q 0..10, qd 11..21, object linear 22..30 and angular 31..39 velocities
#define KIN_FR 165           // floats of an env's frames: R 0..98, p 99..131, world axes 132..164 (an odd stride: phase 2's lanes hit distinct banks)
#define KIN_FR_P 99
#define KIN_FR_AX 132

struct KinPoints { int link[RR_KIN_MAX_POINTS]; float local[RR_KIN_MAX_POINTS][3]; };      // the device copy of the handle's points
struct KinOut { float *joint_vel, *link_pose, *link_vel, *obj_vel, *point_pos, *point_vel, *jacobian; };

// the joints that move body b (b itself and its ancestors), one bit each
struct KinAnc { unsigned m[NB]; };
constexpr KinAnc kin_anc_table() {
    KinAnc t = {};
    for (int b = 0; b < NB; b++) t.m[b] = (1u << b) | (PARENT[b] >= 0 ? t.m[PARENT[b] >= 0 ? PARENT[b] : 0] : 0u);      // (a parent comes before its children)
    return t;
}
__device__ constexpr KinAnc KIN_ANC = kin_anc_table();
static_assert(KIN_ANC.m[8] == 0x1ffu && KIN_ANC.m[10] == 0x67fu, "finger_01 hangs on the whole chain, finger_11 on bodies 0..6, 9, 10");

// row c (0..2 linear, 3..5 angular) of the Jacobian column of joint k for a point at x; fr: the env's frames, x: three floats in LDS
__device__ __forceinline__ float kin_column(const float *fr, const float *x, int k, int c) {
    const float *a = fr + KIN_FR_AX + 3 * k, *p = fr + KIN_FR_P + 3 * k;
    const int c0 = c >= 3 ? c - 3 : c, c1 = c0 == 2 ? 0 : c0 + 1, c2 = c0 == 0 ? 2 : c0 - 1;
    const float lin = a[c1] * (x[c2] - p[c2]) - a[c2] * (x[c1] - p[c1]);
    return c >= 3 ? a[c0] : lin;
}
// row c of the velocity of a point at x on a link moved by the joints of `mask`; qd: the env's joint velocities, KIN_ENVS floats apart
__device__ __forceinline__ float kin_velocity(const float *fr, const float *qd, const float *x, unsigned mask, int c) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const float t = acc + qd[k * KIN_ENVS] * kin_column(fr, x, k, c);
        acc = ((mask >> k) & 1u) ? t : acc;
    }
    return acc;
}
// n floats f(0) .. f(n - 1) to a 16-byte aligned run, by all threads of the workgroup
template <typename F>
__device__ __forceinline__ void kin_store(float *__restrict__ dst, int n, F f) {
    const int n4 = n >> 2;
    for (int i = threadIdx.x; i < n4; i += KIN_THREADS) ((float4 *)dst)[i] = make_float4(f(4 * i), f(4 * i + 1), f(4 * i + 2), f(4 * i + 3));
    for (int i = 4 * n4 + threadIdx.x; i < n; i += KIN_THREADS) dst[i] = f(i);
}

__global__ void __launch_bounds__(KIN_THREADS) k_kinematics(BodyParams B, SimParams P, const RenderModel *RMp, DevPtrs D, KinOut O,
                                                           const KinPoints *__restrict__ pts, int np) {
    static_assert(ST_OVEL - 22 == 21 && ST_OANG - 31 == 21 && ST_QD == NB, "staged slot s is state slot s (s < 22) or s + 21");
    __shared__ float s_st[KIN_ST][KIN_ENVS];
    __shared__ float s_fr[KIN_ENVS][KIN_FR];
    __shared__ float s_x[KIN_ENVS][KIN_ITEMS][3];          // world position of a link's COM frame (0 .. KIN_LINKS-1) / of a point
    __shared__ float s_quat[KIN_ENVS][KIN_LINKS][4];
    __shared__ unsigned s_mask[KIN_ITEMS];
    __shared__ int s_link[KIN_ITEMS], s_body[KIN_ITEMS];   // of a link / point: its URDF link, and that link's moving body (< 0: rigid with the world)
    const RenderModel &RM = *RMp;
    const int N = P.N, tid = threadIdx.x;
    const int env0 = blockIdx.x * KIN_ENVS;
    const int ne = min(KIN_ENVS, N - env0);                // live envs of this workgroup (>= 1 by the grid)
    const int ni = KIN_LINKS + np;
    // 1
    for (int i = tid; i < KIN_ST * KIN_ENVS; i += KIN_THREADS) {
        const int s = i / KIN_ENVS, e = i % KIN_ENVS;
        s_st[s][e] = D.state[(size_t)(s < 22 ? s : s + 21) * N + min(env0 + e, N - 1)];
    }
    if (tid < ni) {
        const int l = tid < KIN_LINKS ? tid : pts->link[tid - KIN_LINKS];
        // link_body < NB is checked on the host (ensure_kinematics refuses another model); the min only keeps phase 3's LDS index
        // in range whatever the blob says.  The compile-time table is read by a compare chain: a body without a match has no mask.
        const int b = min(RM.link_body[l], NB - 1);
        unsigned mask = 0u;
#pragma unroll
        for (int bb = 0; bb < NB; bb++) mask = b == bb ? KIN_ANC.m[bb] : mask;
        s_mask[tid] = mask;
        s_link[tid] = l;
        s_body[tid] = b;
    }
    __syncthreads();
    // 2
    if (tid < KIN_ENVS) {
        // fk_all's operations in its order (the nc:: twins, det_sincosf: the same floats), as a LOOP over the bodies -- a parent comes
        // before its children and its frame is read back from this lane's LDS record.  Rolled, the chain keeps no frame in registers:
        // 99 VGPRs and no SGPR spill, against 158 and 114 with fk_all's unrolled register arrays; the floats are the same.
        float *fr = s_fr[tid];
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
            const m3 Rb = nc::mul(Rj, nc::axis_angle(ax, s_st[ST_Q + b][tid]));
            const v3 aw = nc::mulv(Rj, ax);
#pragma unroll
            for (int k = 0; k < 9; k++) fr[9 * b + k] = Rb.m[k];
            fr[KIN_FR_P + 3 * b] = pb.x; fr[KIN_FR_P + 3 * b + 1] = pb.y; fr[KIN_FR_P + 3 * b + 2] = pb.z;
            fr[KIN_FR_AX + 3 * b] = aw.x; fr[KIN_FR_AX + 3 * b + 1] = aw.y; fr[KIN_FR_AX + 3 * b + 2] = aw.z;
        }
    }
    __syncthreads();
    // 3
    for (int i = tid; i < KIN_ENVS * ni; i += KIN_THREADS) {
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
            const float *lc = pts->local[j - KIN_LINKS];
            p = p + mulv(R, mk(lc[0], lc[1], lc[2]));
        }
        s_x[e][j][0] = p.x; s_x[e][j][1] = p.y; s_x[e][j][2] = p.z;
    }
    __syncthreads();
    // 4
    const float *qd0 = &s_st[ST_QD][0];
    kin_store(O.joint_vel + (size_t)env0 * NB, ne * NB, [&](int i) { return s_st[ST_QD + i % NB][i / NB]; });
    kin_store(O.link_pose + (size_t)env0 * (KIN_LINKS * 7), ne * (KIN_LINKS * 7), [&](int i) {
        const int el = i / 7, c = i % 7, e = el / KIN_LINKS, l = el % KIN_LINKS;
        return c < 3 ? s_x[e][l][c] : s_quat[e][l][c < 3 ? 0 : c - 3];
    });
    kin_store(O.link_vel + (size_t)env0 * (KIN_LINKS * 6), ne * (KIN_LINKS * 6), [&](int i) {
        const int el = i / 6, c = i % 6, e = el / KIN_LINKS, l = el % KIN_LINKS;
        return kin_velocity(s_fr[e], qd0 + e, s_x[e][l], s_mask[l], c);
    });
    const int no6 = 6 * P.nobj;
    kin_store(O.obj_vel + (size_t)env0 * no6, ne * no6, [&](int i) {
        const int eo = i / 6, c = i % 6, e = eo / P.nobj, o = eo % P.nobj;
        return s_st[22 + 3 * o + c + (c >= 3 ? 6 : 0)][e];
    });
    kin_store(O.point_pos + (size_t)env0 * (3 * np), ne * 3 * np, [&](int i) {
        const int ej = i / 3, c = i % 3, e = ej / np, j = ej % np;
        return s_x[e][KIN_LINKS + j][c];
    });
    kin_store(O.point_vel + (size_t)env0 * (6 * np), ne * 6 * np, [&](int i) {
        const int ej = i / 6, c = i % 6, e = ej / np, j = ej % np;
        return kin_velocity(s_fr[e], qd0 + e, s_x[e][KIN_LINKS + j], s_mask[KIN_LINKS + j], c);
    });
    kin_store(O.jacobian + (size_t)env0 * (6 * NB * np), ne * 6 * NB * np, [&](int i) {
        const int ej = i / (6 * NB), r = i % (6 * NB), c = r / NB, k = r % NB, e = ej / np, j = ej % np;
        const float v = kin_column(s_fr[e], s_x[e][KIN_LINKS + j], k, c);
        return ((s_mask[KIN_LINKS + j] >> k) & 1u) ? v : 0.0f;
    });
}
