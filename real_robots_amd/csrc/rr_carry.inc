// rr_carry.inc -- part of realrobot.hip (included there, behind rr_dist.inc and in front of rr_posture.inc; not a stand-alone translation unit).
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
// carry_stage_object what the CARRY instantiations of the posture kernels call -- k_posture_clearance<true>, k_signed_distance<true>,
//                    k_signed_gradient<true> and k_swept_clearance<true> (rr_posture.inc, rr_signed.inc, rr_grad.inc, rr_sweep.inc),
//                    launched in place of the <false> ones while the handle's attachments are on (e->att_on).  Each kernel is ONE
//                    template <bool CARRY>: launch shape, staging, pair function, reduction, summation order and stores are one text,
//                    and the carry-only statements sit under `if constexpr (CARRY)`, so <false> compiles to the instructions the kernel
//                    had before it knew of carried objects (tools/compare_kernel_asm.py; DESIGN.md on why a template and not a shared
//                    function).  Two things differ with CARRY:
//   phase 2  one more barrier: thread 0 rolls the forward kinematics, and BEHIND the barrier threads 1..NOBJ stage the objects
//            (carry_stage_object).  A free object by exactly the plain kernel's operations -- its bits are the plain kernel's --, an attached
//            one as R_o = R_b R_rel, p_o = p_b + R_b t_rel from the frames just rolled (contraction off), not from D.state.  Thread 0 and
//            threads 1..3 are lanes of one wave, so the plain kernel's two branches ran one after the other as well: the order costs the
//            barrier and nothing else (DESIGN.md).
//   phase 3  (gradient only) a shape of an attached object takes the joint mask KIN_ANC.m[b] of its body: the objects' b + 1 are made
//            wave-uniform behind phase 2, picked by a compare chain over the masked object index sd_pair returns, and fed to the
//            plain kernel's compare chain over the body index.  A free object has no mask, as before.
// The sweep's own differences (the motion bound of a carried shape, staging at every step) are in rr_sweep.inc's header.
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

// Phase 2 of the CARRY instantiations for object o (threads 1..NOBJ, behind the barrier that follows the forward kinematics): its frame
// into ob[12 o ..], and b + 1 of its body (0: free) back.  The free branch is the text of the plain kernels' phase 2.
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
