// rr_pik.inc -- part of realrobot.hip (included there, behind rr_pkin.inc; not a stand-alone translation unit).
// k_posture_ik: damped-least-squares inverse kinematics for K target tool poses per env of the whole batch (rr_posture_ik, realrobot.h):
// the first stage of the posture pipeline -- its output is the [N, K, 11] tensor every posture query reads.  Read-only on the
// simulation: it reads the two tensors (or, without seeds, columns 0..10 of D.state), the model constants and the points (a kernel
// argument), never the preparation record; launched by rr_posture_ik alone, never by a step.
//
// A row is a (target, seed) pair (e, k); the N * K rows are one flat list.  One LANE per row, 64-thread workgroups; a lane behind the
// list's end loads and stores nothing.  7 + 11 floats in and 11 + 4 + 2 values out per row, lane l of a wave at row l of the
// wave's 64 consecutive rows; everything between the loads and the stores lives in registers with compile-time indices.
//
// Once per row:
//   the point's link and local offset by compare chains over the point table (a kernel argument: every entry is read at a compile-time
//   index and the VALUE is selected), the link's body, `ab`, the deepest ARM body (0..6) that carries it (-1: rigid with the world; a
//   finger hangs on body 6), and the constant transform (Rc, pc) from body ab to the tool frame: the finger sub-chain at the seed's
//   finger joints, the link's COM frame, the local offset.  All of that is uniform over the wave except the finger angles.
// Per iteration (ik_dls' operations, rr_ik.inc): the chain of the seven arm bodies, the tool frame of body ab, the residual, the
//   6 x 7 (position only: 3 x 7) Jacobian with column k zeroed for k > ab, J J^T + lambda^2 I, its Cholesky factor, two
//   triangular solves, dq = J^T x, the cap on |dq|inf, the clamp or the wrap.
// The constants of the arm chain (7 x (jpos, jrot, axis), the base position, the arm's limits: PIK_C floats) are copied from the kernel
// argument into LDS once per workgroup and read from there in every iteration -- uniform addresses, a broadcast --: held in scalar
// registers across the loop they do not fit (105 + 17 values beside the addresses) and the allocator spills them through vector lanes.
// A wave runs as long as its slowest lane: a lane that has stopped idles (EXEC) until the wave's last lane stops.
// No atomics; no tensor value forms an address; the loop bounds are constants and max_iterations.

struct PikOut { float *posture, *result; int *info; };
struct PikOpt { int point, max_it; float tol, lam2, max_step; unsigned flags; };

#define PIK_BODY 15          // floats per arm body in the LDS table: jpos 0..2, jrot 3..11, axis 12..14
#define PIK_BASE 105         // robot_pos
#define PIK_LIM 108          // limits[7][2]
#define PIK_C 122

// the tool pose of the arm posture q[0..6]: joint origins p[], world axes ax[] of the seven arm bodies, tool frame (Re, pe) = frame of
// body ab (the world frame at the robot's base for ab < 0) times (Rc, pc); cm: the LDS table
__device__ __forceinline__ void pik_fk(const float *cm, const float *q, int ab, const m3 &Rc, v3 pc, v3 *p, v3 *ax, m3 &Re, v3 &pe) {
    m3 R = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    v3 pp = mk(cm[PIK_BASE], cm[PIK_BASE + 1], cm[PIK_BASE + 2]);
    m3 Ra = R;
    v3 pa = pp;
#pragma unroll
    for (int b = 0; b < 7; b++) {
        const float *cb = cm + PIK_BODY * b;
        m3 jr;
#pragma unroll
        for (int k = 0; k < 9; k++) jr.m[k] = cb[3 + k];
        const m3 Rj = mul(R, jr);
        const v3 a = mk(cb[12], cb[13], cb[14]);
        pp = pp + mulv(R, mk(cb[0], cb[1], cb[2]));
        p[b] = pp;
        ax[b] = mulv(Rj, a);
        R = mul(Rj, nc::axis_angle(a, q[b]));
        if (b == ab) { Ra = R; pa = pp; }       // (ab is uniform over the wave)
    }
    Re = mul(Ra, Rc);
    pe = pa + mulv(Ra, pc);
}

// body `b` (7..10) in the frame of its parent: (R, p) <- (R, p) o (jpos[b], jrot[b] rot(axis[b], ang))
__device__ __forceinline__ void pik_hop(const BodyParams &B, int b, float ang, m3 &R, v3 &p) {
    m3 jr;
#pragma unroll
    for (int k = 0; k < 9; k++) jr.m[k] = B.jrot[b][k];
    p = p + mulv(R, mk(B.jpos[b][0], B.jpos[b][1], B.jpos[b][2]));
    R = mul(mul(R, jr), nc::axis_angle(mk(B.axis[b][0], B.axis[b][1], B.axis[b][2]), ang));
}

template <int POS_ONLY>
__device__ __forceinline__ void pik_row(const BodyParams &B, const float *cm, const RenderModel &RM, const float *__restrict__ targets, const float *__restrict__ seeds,
                                        const float *__restrict__ state, int N, int K, int row, const PikOut &O, const KinPoints &pts, const PikOpt &opt) {
    static_assert(PARENT[7] == 6 && PARENT[8] == 7 && PARENT[9] == 6 && PARENT[10] == 9, "the two fingers hang on arm body 6");
    constexpr int M = POS_ONLY ? 3 : 6;
    // ---- the row's inputs
    float q[NB], t[7];
    if (seeds) {
#pragma unroll
        for (int k = 0; k < NB; k++) q[k] = seeds[(size_t)row * NB + k];
    } else {
        const int env = row / K;
#pragma unroll
        for (int k = 0; k < NB; k++) q[k] = STT(ST_Q + k);
    }
#pragma unroll
    for (int k = 0; k < 7; k++) t[k] = targets[(size_t)row * 7 + k];
    const v3 tp = mk(t[0], t[1], t[2]);
    // (rr_ik's quat_target: a zero quaternion gives NaNs, and with them status 2 in full-pose mode)
    const float qn = rsqrtf(t[3] * t[3] + t[4] * t[4] + t[5] * t[5] + t[6] * t[6]);
    const m3 Rt = quat_to_m3(t[3] * qn, t[4] * qn, t[5] * qn, t[6] * qn);
    // ---- the tool frame in its arm body (uniform but for the finger angles)
    int pl = 0;
    v3 loc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < RR_KIN_MAX_POINTS; j++)
        if (opt.point == j) { pl = pts.link[j]; loc = mk(pts.local[j][0], pts.local[j][1], pts.local[j][2]); }
    const int l = min(max(pl, 0), KIN_LINKS - 1);
    const int body = min(RM.link_body[l], NB - 1);          // (< NB is checked on the host; < 0: the link is rigid with the world)
    const int ab = body < 7 ? body : 6;
    m3 lr;
#pragma unroll
    for (int k = 0; k < 9; k++) lr.m[k] = RM.link_rot[l][k];
    m3 Rc = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    v3 pc = mk(0.0f, 0.0f, 0.0f);
    if (body == 7 || body == 8) pik_hop(B, 7, q[7], Rc, pc);
    if (body == 8) pik_hop(B, 8, q[8], Rc, pc);
    if (body == 9 || body == 10) pik_hop(B, 9, q[9], Rc, pc);
    if (body == 10) pik_hop(B, 10, q[10], Rc, pc);
    pc = pc + mulv(Rc, mk(RM.link_pos[l][0], RM.link_pos[l][1], RM.link_pos[l][2]) + mulv(lr, loc));
    Rc = mul(Rc, lr);
    // ---- the seed's arm joints into the limits (a non-finite one stays as it is: its row ends with status 2)
    const bool clamp = (opt.flags & RR_PIK_CLAMP_LIMITS) != 0u;
    if (clamp) {
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = fabsf(q[k]) < INFINITY ? fminf(fmaxf(q[k], cm[PIK_LIM + 2 * k]), cm[PIK_LIM + 2 * k + 1]) : q[k];
    }
    // ---- the iteration
    int status = 1, it = 0;
    float err, ep, w2, c;
    for (;; it++) {
        asm volatile("" ::: "memory");          // the table is read again in every iteration, not kept in registers across the loop
        v3 p[7], ax[7], pe;
        m3 Re;
        pik_fk(cm, q, ab, Rc, pc, p, ax, Re, pe);
        const v3 dp = tp - pe;
        float e[M];
        e[0] = dp.x; e[1] = dp.y; e[2] = dp.z;
        ep = sqrtf(dot(dp, dp));
        const m3 Rerr = mul(Rt, transpose(Re));
        const v3 w = mk(0.5f * (Rerr.m[7] - Rerr.m[5]), 0.5f * (Rerr.m[2] - Rerr.m[6]), 0.5f * (Rerr.m[3] - Rerr.m[1]));
        w2 = dot(w, w);
        c = 0.5f * (Rerr.m[0] + Rerr.m[4] + Rerr.m[8] - 1.0f);       // cos of the orientation error; sqrt(w2) is its sine
        if (POS_ONLY) {
            err = ep;                   // (w and c only feed the reported angle)
        } else {
            e[M - 3] = w.x; e[M - 2] = w.y; e[M - 1] = w.z;
            err = sqrtf(dot(dp, dp) + w2);
        }
        if (!(fabsf(err) < INFINITY)) { status = 2; break; }
        if (err < opt.tol && (POS_ONLY || c > 0.0f)) { status = 0; break; }       // (w vanishes at a half-turn too: c < 0 there)
        if (it >= opt.max_it) break;
        float J[M][7];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const v3 jl = cross(ax[k], pe - p[k]);
            const bool on = k <= ab;
            J[0][k] = on ? jl.x : 0.0f; J[1][k] = on ? jl.y : 0.0f; J[2][k] = on ? jl.z : 0.0f;
            if (!POS_ONLY) { J[M - 3][k] = on ? ax[k].x : 0.0f; J[M - 2][k] = on ? ax[k].y : 0.0f; J[M - 1][k] = on ? ax[k].z : 0.0f; }
        }
        // Cholesky factor of A = J J^T + lambda^2 I, row by row, and A x = e
        float L[M][M], y[M], x[M];
#pragma unroll
        for (int i = 0; i < M; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                float s = (i == j) ? opt.lam2 : 0.0f;
#pragma unroll
                for (int k = 0; k < 7; k++) s += J[i][k] * J[j][k];
#pragma unroll
                for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
                if (i == j) L[i][i] = rsqrtf(s);            // (the reciprocal of the diagonal: every division below is a product)
                else L[i][j] = s * L[j][j];
            }
#pragma unroll
        for (int i = 0; i < M; i++) {
            float s = e[i];
#pragma unroll
            for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
            y[i] = s * L[i][i];
        }
#pragma unroll
        for (int i = M - 1; i >= 0; i--) {
            float s = y[i];
#pragma unroll
            for (int k = i + 1; k < M; k++) s -= L[k][i] * x[k];
            x[i] = s * L[i][i];
        }
        float dq[7], mx = 0.0f;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < M; i++) s += J[i][k] * x[i];
            dq[k] = s;
            mx = fmaxf(mx, fabsf(s));
        }
        const float sc = mx > opt.max_step ? opt.max_step / mx : 1.0f;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            float v = q[k] + dq[k] * sc;
            if (clamp) {
                const float lo = cm[PIK_LIM + 2 * k], hi = cm[PIK_LIM + 2 * k + 1];
                v = v < lo ? lo : (v > hi ? hi : v);      // (a NaN stays a NaN: status 2 at the next residual)
            } else {
                // into (-pi, pi]: pi - ((pi - v) mod 2 pi)
                v = 3.14159265358979f - v;
                v = v - 6.28318530717959f * floorf(v * 0.159154943091895f);
                v = 3.14159265358979f - v;
                v = v > 3.14159265358979f || v <= -3.14159265358979f ? 3.14159265358979f : v;      // (the rounding of the two lines above)
            }
            q[k] = k <= ab ? v : q[k];           // a joint that does not move the link keeps its seed value
        }
    }
    // ---- the row's outputs
#pragma unroll
    for (int k = 0; k < NB; k++) O.posture[(size_t)row * NB + k] = q[k];
    O.result[(size_t)row * 4 + 0] = err;
    O.result[(size_t)row * 4 + 1] = ep;
    O.result[(size_t)row * 4 + 2] = atan2f(sqrtf(w2), c);
    O.result[(size_t)row * 4 + 3] = 0.0f;
    O.info[(size_t)row * 2 + 0] = status;
    O.info[(size_t)row * 2 + 1] = it;
}

template <int POS_ONLY>
__global__ void __launch_bounds__(64) k_posture_ik(BodyParams B, const RenderModel *RMp, const float *__restrict__ targets /*[rows][7]*/,
                                                   const float *__restrict__ seeds /*[rows][11] or null*/, const float *__restrict__ state, int N, int K,
                                                   PikOut O, KinPoints pts, PikOpt opt) {
    static_assert(ST_Q == 0, "joint b of an env is state slot b");
    __shared__ float s_c[PIK_C];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int b = 0; b < 7; b++) {
#pragma unroll
            for (int k = 0; k < 3; k++) { s_c[PIK_BODY * b + k] = B.jpos[b][k]; s_c[PIK_BODY * b + 12 + k] = B.axis[b][k]; }
#pragma unroll
            for (int k = 0; k < 9; k++) s_c[PIK_BODY * b + 3 + k] = B.jrot[b][k];
            s_c[PIK_LIM + 2 * b] = B.limits[b][0]; s_c[PIK_LIM + 2 * b + 1] = B.limits[b][1];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) s_c[PIK_BASE + k] = B.robot_pos[k];
    }
    __syncthreads();
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row < N * K) pik_row<POS_ONLY>(B, s_c, *RMp, targets, seeds, state, N, K, row, O, pts, opt);
}
