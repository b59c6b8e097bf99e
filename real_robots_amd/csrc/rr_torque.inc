// rr_torque.inc -- part of realrobot.hip (included there, behind rr_pdyn.inc; not a stand-alone translation unit).
// Joint torque inputs of the step (rr_set_joint_torques, realrobot.h): the handle holds a table tau f32 [N][11] over the eleven
// independent joints, and while torques are set every rr_step launches k_joint_torque in front of its solve.
//
// k_joint_torque.  The preparation leaves the unconstrained joint velocities qd* = qd + dt M^-1 (-bias - damping qd) and M^-1 in the
// env's record (S_QDS, S_MINV; rr_prep.inc, end of prep16_body).  A joint torque is linear in that formula, so the step adds
//   qd*' = qd* + dt M^-1 tau
// to the record behind the preparation instead of feeding tau through it: no existing kernel changes, and the look-ahead -- the
// preparation of step t + 1 that runs during step t -- stays valid when the torques change every step.  One 16-lane group per env,
// as in the preparation; lane i < 11 reads row i of M^-1 as the preparation stored it (the rows its own qd* was formed with) and
// forms sum_j M^-1[i][j] tau[j] from 0.0f in ASCENDING j with fused multiply-adds, tau[j] broadcast from lane j of the group.  No
// atomics, no LDS: an env's result depends on its own record and row alone.
// Table layout: [N][11] compact, the layout of the ABI -- the zero-copy view is the table itself, a group reads its row as one
// 44-byte span, and a caller's [N, 11] tensor is copied span for span.
// Not touched: an env whose row is all zero (either sign; tested before any store, so its S_QDS keeps its bits) and a frozen env
// (errflags & 1: the preparation has not written its record).  Both tests are uniform in the group.
#define JT_THREADS 256       // sixteen envs per workgroup
static_assert(JT_THREADS % 64 == 0 && NB <= 16, "whole waves of four 16-lane groups; a joint per lane");

__global__ void __launch_bounds__(JT_THREADS) k_joint_torque(SimParams P, DevPtrs D, const float *__restrict__ tau /*[N][11]*/) {
    const int l = threadIdx.x & 15;
    const int env = (int)((blockIdx.x * (unsigned)JT_THREADS + threadIdx.x) >> 4);
    const bool in = env < P.N;
    const float t = in && l < NB ? tau[(size_t)env * NB + l] : 0.0f;
    // the group's sixteen bits of the wave's ballot: any entry of the row that is not +-0 (a NaN counts: it is not zero)
    const unsigned long long nz = __ballot(t != 0.0f);
    const unsigned grp = (unsigned)(nz >> (threadIdx.x & 48)) & 0xffffu;
    if (!in || grp == 0u || (D.errflags[env] & 1u)) return;      // (uniform in the group: the broadcasts below see all sixteen lanes)
    float *scratch = D.scratch;
    const float *row = &SCR(S_MINV + (l < NB ? l : 0) * NB);
    // (lane j of the group is lane (threadIdx.x & 48) + j of the wave; the builtin, not __shfl: a second width among the callers of
    // that header function changes the instructions the other kernels get for theirs)
    const int grp_addr = (int)(threadIdx.x & 48u) << 2;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; j++) acc = __builtin_fmaf(row[j], __int_as_float(__builtin_amdgcn_ds_bpermute(grp_addr + 4 * j, __float_as_int(t))), acc);
    if (l < NB) SCR(S_QDS + l) += P.dt * acc;
}

// The table's rows of the masked envs from a caller's tensor [N][11] (src == nullptr: zeros), one thread per entry.
__global__ void __launch_bounds__(256) k_joint_torque_set(int N, const float *__restrict__ src /*[N][11] or nullptr*/,
                                                          const unsigned char *__restrict__ mask /*[N] or nullptr: all*/, float *__restrict__ table) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N * NB) return;
    if (mask && !mask[i / NB]) return;
    table[i] = src ? src[i] : 0.0f;
}
