// rr_prep.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_prep: the state part of a step (forward kinematics, object terms, joint-space dynamics)
// ---------------------------------------------------------------------------------------------- k_prep
// Which env a work item of a per-class launch handles: sel 0 all envs (idx = env); 1 the light envs (idx = env, others are
// skipped); 2 / 3 entry idx of the heavy / very heavy list of the CURRENT contact frame.  -1: nothing to do.
__device__ __forceinline__ int pick_env(const DevPtrs &D, int sel, int idx, int N) {
    if (idx >= N) return -1;
    if (sel == 0) return idx;
    if (sel == 1) return D.hgflag[idx] == 0 ? idx : -1;
    if (sel == 2) return idx < D.hcount[0] ? D.hlist[idx] : -1;
    return idx < D.hcount2[0] ? D.hlist2[idx] : -1;
}

// The out-of-bounds rule of control_objects_limits (env.py:257-264) as a function of the object's position.
__device__ __forceinline__ bool object_out_of_bounds(float x, float z, float table_z) { return z < table_z || (x > 0.11f && z < 0.29f); }

// Object terms of object i of `env` -- rotation, world inverse inertia, unconstrained velocities -- of the pose that counts: an object
// the out-of-bounds rule (env.py:257-264) sends home is taken at its home pose, at rest (the solve kernel writes that pose into the
// state when the step starts).  One function for every kernel of the preparation (k_prep_a16 in line, k_prep_ab16 ahead): the same
// expressions, hence the same bits.
// (the object's principal inertias: the env's own, D.obj_dyn -- rr_set_object_dynamics)
// Contraction-free: which products the compiler fuses into multiply-adds depends on the code it is inlined into -- a loop-invariant
// product hoisted in one caller, fused in another -- and the forms of a step must agree bit for bit.  The bits themselves are
// recorded: tests/golden/prep_thread_per_env.npz holds them as a loop over the objects on one thread computed them.
#pragma clang fp contract(off)
__device__ __forceinline__ void object_terms(const BodyParams &B, const SimParams &P, const DevPtrs &D, int env, int i, bool store = true) {
    const int N = P.N;
    const float *od = D.obj_dyn + env;
    const float ixx = od[(4 * i + 1) * N], iyy = od[(4 * i + 2) * N], izz = od[(4 * i + 3) * N];
    const float *state = D.state;
    float *scratch = D.scratch;
    float px = STT(ST_OPOS + 3 * i), py = STT(ST_OPOS + 3 * i + 1), pz = STT(ST_OPOS + 3 * i + 2);
    float qx = STT(ST_OQUAT + 4 * i), qy = STT(ST_OQUAT + 4 * i + 1), qz = STT(ST_OQUAT + 4 * i + 2), qw = STT(ST_OQUAT + 4 * i + 3);
    v3 v = mk(STT(ST_OVEL + 3 * i), STT(ST_OVEL + 3 * i + 1), STT(ST_OVEL + 3 * i + 2));
    v3 om = mk(STT(ST_OANG + 3 * i), STT(ST_OANG + 3 * i + 1), STT(ST_OANG + 3 * i + 2));
    if (object_out_of_bounds(px, pz, B.table_z)) {
        px = D.obj_home[(size_t)(7 * i) * N + env]; py = D.obj_home[(size_t)(7 * i + 1) * N + env]; pz = D.obj_home[(size_t)(7 * i + 2) * N + env];
        qx = D.obj_home[(size_t)(7 * i + 3) * N + env]; qy = D.obj_home[(size_t)(7 * i + 4) * N + env];
        qz = D.obj_home[(size_t)(7 * i + 5) * N + env]; qw = D.obj_home[(size_t)(7 * i + 6) * N + env];
        v = mk(0, 0, 0); om = mk(0, 0, 0);
    }
    m3 R = nc::quat_to_m3(qx, qy, qz, qw);
    // (the nc:: twins throughout: an operator or helper defined outside this region would carry its own `contract` flags in)
    const m3 Id = {{ixx, 0, 0, 0, iyy, 0, 0, 0, izz}}, Iid = {{1.0f / ixx, 0, 0, 0, 1.0f / iyy, 0, 0, 0, 1.0f / izz}};
    const m3 Rt = transpose(R);
    const m3 Iw = nc::mul(nc::mul(R, Id), Rt), Iinv = nc::mul(nc::mul(R, Iid), Rt);
    const float vn = sqrtf(nc::dot(v, v)), wn = sqrtf(nc::dot(om, om));
    v3 vs = nc::add(v, nc::scale(nc::scale(v, -(P.lin_damp + P.lin_damp * vn)), P.dt));
    vs.z = vs.z - P.dt * P.gravity;
    const v3 alo = nc::mulv(Iinv, nc::cross(om, nc::mulv(Iw, om)));
    const v3 ws = nc::add(om, nc::scale(nc::sub(nc::scale(alo, -1.0f), nc::scale(om, P.ang_damp + P.ang_damp * wn)), P.dt));
    if (!store) return;
#pragma unroll
    for (int k = 0; k < 9; k++) { SCR(S_OR + 9 * i + k) = R.m[k]; SCR(S_OIINV + 9 * i + k) = Iinv.m[k]; }
    SCR(S_OVS + 3 * i) = vs.x; SCR(S_OVS + 3 * i + 1) = vs.y; SCR(S_OVS + 3 * i + 2) = vs.z;
    SCR(S_OWS + 3 * i) = ws.x; SCR(S_OWS + 3 * i + 1) = ws.y; SCR(S_OWS + 3 * i + 2) = ws.z;
    SCR(S_OP + 3 * i) = px; SCR(S_OP + 3 * i + 1) = py; SCR(S_OP + 3 * i + 2) = pz;
}
#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------------------------- k_prep16: sixteen lanes per env
// The state part of the preparation -- everything of a step that does NOT need the action, i.e. a function of the state the
// previous step left: PHASE 1 = forward kinematics and object terms (rotation, world inverse inertia, unconstrained
// velocities; the out-of-bounds rule decides which object pose counts) -- all the collision kernel needs -- and PHASE 2 =
// joint-space dynamics (mass matrix, bias forces, Cholesky, M^-1, unconstrained velocities), which only the solver needs.
// Together with k_collide they form the LOOK-AHEAD of a step: rr_step launches them for step t+1 behind the solve of step t,
// class by class (sel, pick_env), under the render of step t; only when the state was changed from outside in between
// (reset, set_state, teleports) do they run in line at the start of the step.  (When the kernels are timed one by one the
// two phases run back to back and are reported together as "k_prep".)
// One env per 16-lane group, four envs per wave: the joint-space dynamics of an env are ~7 000 operations, and ONE thread walking
// them at a lone wave's issue rate (rounds 1-5) was the tail of every step (0.030 ms alone, 0.080 ms under overlap -- each of its
// 64 waves wanted a whole SIMD at 194 VGPRs) and a third of the chain of one env (BASELINE configs 1 and 2).  Here the work is
// spread the way north_star asks for -- the chain of frames and the per-body records through LDS, per-body reductions through DPP:
//   * forward kinematics: lanes 0..2 walk the chain, lane r holding ROW r of the frame at hand (lanes 3..5 take the second finger
//     pair, bodies 9 and 10, from body 6 on); the joints' local rotations are computed by the lanes of their bodies and read back
//     from LDS.  Every output is fk_all's operations in fk_all's order, contraction-free: the same bits as fk_all (the collision
//     pass compares its decisions bit for bit with the oracle);
//   * everything per body -- centre of mass, world inertia, the body's own RNEA terms, its column of the mass matrix, its row of
//     the Cholesky factor, its column of M^-1 -- on the lane of that body (lanes 0..10);
//   * the velocity recursion of RNEA: every body lane walks ITS OWN root path in lock step (level k = body k up to the fork at
//     body 6, then 7 / 9 and 8 / 10), the node's record {axis, joint velocity, position} read from LDS;
//   * RNEA's force pass as subtree sums: every body's force and its torque about the wrist (body 6's joint), summed leaf to root
//     with one masked DPP multiply-add per value and tree edge, then referred back to the body's own joint;
//   * the composite bodies: nine lanes hold one entry of the 3 x 3 inertia each, the merges run leaf to root;
//   * the objects: a second wave of the workgroup, lane (env, object), each through object_terms.
// ~2 700 issue slots where the one-thread walk took ~9 000 (ISA counts), 128-thread workgroups of <= 128 VGPRs that fit beside the
// render's.  The dynamics are contractable fp32, with v_rcp / v_rsq (1 ulp) for the composite masses and the Cholesky diagonal: NOT
// bit for bit a plain IEEE evaluation's, equal to it to rounding -- tests/test_gpu_round6.py compares frames and object terms bit
// for bit, M^-1 and the unconstrained velocities to rounding, with a record of the one-thread kernels (tests/golden/
// prep_thread_per_env.npz), tests/test_gpu_numpy_step.py every field with a float64 numpy preparation; every form of a step uses
// this one kernel family, so the placements of a step stay bitwise equal.
#define P16_ENVS 4
// LDS record of an env: frames R [11][9]; per-body record BQ [11][8] = {axis xyz, joint velocity, position xyz, -}; local joint
// rotations RAA [11][12]; composite bodies CI [11][9] and CC [11][4] = {centre xyz, mass}; M^-1 rows X [11][12]
enum { PL_R = 0, PL_BQ = PL_R + 100, PL_RAA = PL_BQ + 88, PL_CI = PL_RAA + 132, PL_CC = PL_CI + 100, PL_X = PL_CC + 44, PL_TOTAL = PL_X + 132 };
static_assert(PL_BQ % 4 == 0 && PL_RAA % 4 == 0 && PL_CC % 4 == 0 && PL_X % 4 == 0 && PL_TOTAL % 4 == 0, "float4 parts of the preparation's LDS record");
// per-body constants of the body lanes, D.body_tab [NB][16]: com (3), inertia xx yy zz xy xz yz (6), mass, joint damping, axis (3), -, -
enum { BT_COM = 0, BT_INERTIA = 3, BT_MASS = 9, BT_DAMP = 10, BT_AXIS = 11, BT_STRIDE = 16 };

template <int J> __device__ __forceinline__ float p16_bcast(float v) {      // lane J of the 16-lane group, in every lane of it
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + J, 0xf, 0xf, true));
}
template <int J> __device__ __forceinline__ v3 p16_bcast3(v3 v) { return mk(p16_bcast<J>(v.x), p16_bcast<J>(v.y), p16_bcast<J>(v.z)); }
// (component-wise: a ?: on the struct itself selects between two ADDRESSES and sends both operands to private memory)
__device__ __forceinline__ v3 p16_sel3(bool c, v3 a, v3 b) { return mk(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
#pragma clang fp contract(off)
namespace nc {
// a0 b0 + a1 b1 + a2 b2, the association of nc::mul / nc::mulv
__device__ __forceinline__ float row3(float a0, float a1, float a2, float b0, float b1, float b2) { return a0 * b0 + a1 * b1 + a2 * b2; }
__device__ __forceinline__ float add1(float a, float b) { return a + b; }
}
#pragma clang fp contract(fast)
#define P16_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// acc += (lane J's a) * b / acc -= (lane J's a) * b in ONE instruction (VOP2 with a DPP operand; the compiler folds a row_newbcast into
// its user only now and then).  The compiler's hazard recogniser does not look inside the asm: the `s_nop 1` in front covers "a VALU
// instruction wrote the DPP source within the last two wait states" whatever the scheduler or a register copy put there; the
// five-wait-state hazard behind a VALU write of EXEC is excluded by the build gate (tools/check_dpp_hazard.py).
#define P16_FMAC_BCAST(J, acc, a, b) asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(b))
#define P16_FNMAC_BCAST(J, acc, a, b) asm("s_nop 1\n\tv_fmac_f32_dpp %0, -%1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(b))
#define P16_MUL_BCAST(J, dst, a, b) asm("s_nop 1\n\tv_mul_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "=v"(dst) : "v"(a), "v"(b))

// One merge of the composite-body pass: node b folded into its parent p, about the common centre of mass -- entry (ei, ej) of the
// inertia on this lane, the scalars on every lane.  (1 / m: v_rcp_f32, 1 ulp -- a centre of mass to 1e-7 relative.)
struct P16Comp { float m; v3 c; float I; };
__device__ __forceinline__ P16Comp p16_merge(const P16Comp &p, const P16Comp &b, int ei, int ej) {
    P16Comp o;
    o.m = p.m + b.m;
    o.c = (p.c * p.m + b.c * b.m) * __builtin_amdgcn_rcpf(o.m);
    const v3 d1 = p.c - o.c, d2 = b.c - o.c;
    const float s1 = dot(d1, d1), s2 = dot(d2, d2);
    const float d1i = ei == 0 ? d1.x : (ei == 1 ? d1.y : d1.z), d1j = ej == 0 ? d1.x : (ej == 1 ? d1.y : d1.z);
    const float d2i = ei == 0 ? d2.x : (ei == 1 ? d2.y : d2.z), d2j = ej == 0 ? d2.x : (ej == 1 ? d2.y : d2.z);
    const float e = ei == ej ? 1.0f : 0.0f;
    o.I = p.I + b.I + p.m * (s1 * e - d1i * d1j) + b.m * (s2 * e - d2i * d2j);
    return o;
}

// The object wave of k_prep_ab16: lane t < 12 takes object t % 3 of the workgroup's env t / 3.
__device__ __forceinline__ void prep16_objects(const BodyParams &B, const SimParams &P, const DevPtrs &D, int sel) {
    const int t = (int)threadIdx.x - 64;
    if (t >= 3 * P16_ENVS) return;
    const int o = t % 3;
    const int env = pick_env(D, sel, (int)blockIdx.x * P16_ENVS + t / 3, P.N);
    if (env < 0 || o >= P.nobj || (D.errflags[env] & 1u)) return;
    object_terms(B, P, D, env, o);
}

template <int PHASE>       // 0: everything (k_prep_ab16: wave 0 the robots, wave 1 the objects); 1: frames + objects (k_prep_a16); 2: joint-space dynamics only (k_prep_b16)
__device__ __forceinline__ void prep16_body(const BodyParams &B, const SimParams &P, const DevPtrs &D, int sel) {
    __shared__ __attribute__((aligned(16))) float s_p16[P16_ENVS * PL_TOTAL];
    const int N = P.N;
    const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int env_raw = pick_env(D, sel, (int)blockIdx.x * P16_ENVS + grp, N);
    bool mine = env_raw >= 0;
    const int env = mine ? env_raw : 0;                    // groups without an env run along on env 0's data and store nothing
    if (mine && (D.errflags[env] & 1u)) mine = false;       // frozen env
    if (__ballot(mine) == 0ull) return;
    const float *state = D.state;
    float *scratch = D.scratch;
    float *lds = s_p16 + grp * PL_TOTAL;
    const int lb = l < NB ? l : 0;                          // the body of this lane (lanes 11..15 alias body 0; they store nothing)
    const bool body_lane = mine && l < NB;
    // ---- stage-in: the lane's joint, its body's constants
    const float q_l = STT(ST_Q + lb), qd_l = STT(ST_QD + lb);
    const float4 *bt = (const float4 *)(D.body_tab + lb * BT_STRIDE);
    const float4 t0 = bt[0], t1 = bt[1], t2 = bt[2], t3 = bt[3];
    const v3 com_l = mk(t0.x, t0.y, t0.z);
    const float inertia_l[6] = {t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
    const float mass_l = t2.y;
    const float damp_l = D.env_act[(size_t)(3 * NB + lb) * N + env];      // the env's own joint damping (rr_set_env_actuators; BT_DAMP is the blob's)
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
        }
    }
    P16_SYNC();
    // ---- forward kinematics: row r of the frame at hand on lane r (chain A: lanes 0..2, and every other lane redundantly;
    // chain B: lanes 3..5 from the fork at body 6 on)
    {
        const int r = l % 3;
        const bool chB = l >= 3 && l < 6;
        float a0 = r == 0 ? 1.0f : 0.0f, a1 = r == 1 ? 1.0f : 0.0f, a2 = r == 2 ? 1.0f : 0.0f;
        float pr = r == 0 ? B.robot_pos[0] : (r == 1 ? B.robot_pos[1] : B.robot_pos[2]);
#define P16_LEVEL(BA, BB)                                                                                                      \
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
                if (PHASE != 2 && mine) {                                                                                      \
                    SCR(S_BR + 9 * body + 3 * r) = r0; SCR(S_BR + 9 * body + 3 * r + 1) = r1; SCR(S_BR + 9 * body + 3 * r + 2) = r2; \
                    SCR(S_BP + 3 * body + r) = pb; SCR(S_BAX + 3 * body + r) = aw;                                             \
                }                                                                                                              \
            }                                                                                                                  \
            a0 = r0; a1 = r1; a2 = r2; pr = pb;                                                                                \
        }
        P16_LEVEL(0, 0) P16_LEVEL(1, 1) P16_LEVEL(2, 2) P16_LEVEL(3, 3) P16_LEVEL(4, 4) P16_LEVEL(5, 5) P16_LEVEL(6, 6)
        P16_LEVEL(7, 9) P16_LEVEL(8, 10)
#undef P16_LEVEL
        static_assert(PARENT[7] == 6 && PARENT[9] == 6 && PARENT[8] == 7 && PARENT[10] == 9, "the two finger chains fork at body 6");
    }
    if (PHASE == 1) return;
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
    // ---- mass matrix: lane j computes M[i][j] = M[j][i] for the ancestors-or-self i of j -- row j of the lower triangle
    float Mrow[NB];
    {
        m3 cI;
#pragma unroll
        for (int k = 0; k < 9; k++) cI.m[k] = lds[PL_CI + 9 * lb + k];
        const float4 c4 = *(const float4 *)&lds[PL_CC + 4 * lb];
        const v3 cc = mk(c4.x, c4.y, c4.z);
        const float cm = c4.w;
        const unsigned anc = lb <= 6 ? (2u << lb) - 1u : (lb == 7 ? 0x0ffu : (lb == 8 ? 0x1ffu : (lb == 9 ? 0x27fu : 0x67fu)));
        const v3 Ia = mulv(cI, bax);
        const v3 f = cross(bax, cc - bp) * cm;
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const float4 q0 = *(const float4 *)&lds[PL_BQ + 8 * i], q1 = *(const float4 *)&lds[PL_BQ + 8 * i + 4];      // body i: axis, position
            const v3 nn = Ia + cross(cc - mk(q1.x, q1.y, q1.z), f);
            const float v = dot(mk(q0.x, q0.y, q0.z), nn);
            Mrow[i] = ((anc >> i) & 1u) ? v : 0.0f;
        }
    }
    // ---- RNEA bias (qdd = 0, base acceleration +g): the velocity recursion along this lane's own root path, level by level
    float bias_l;
    {
        v3 w = mk(0, 0, 0), al = mk(0, 0, 0), ap = mk(0, 0, P.gravity), pp = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]);
        const int plen = lb <= 6 ? lb + 1 : (lb == 7 || lb == 9 ? 8 : 9);      // bodies on the path root .. b
        const bool second = lb >= 9;                                          // the path runs through body 9 (not 7)
#define P16_RNEA_LEVEL(K, BA, BB)                                                                                   \
        {                                                                                                           \
            const int node = (BA) == (BB) ? (BA) : (second ? (BB) : (BA));                                          \
            const float4 q0 = *(const float4 *)&lds[PL_BQ + 8 * node], q1 = *(const float4 *)&lds[PL_BQ + 8 * node + 4]; \
            const v3 ax_ = mk(q0.x, q0.y, q0.z), p_ = mk(q1.x, q1.y, q1.z);                                         \
            const float qd_ = q0.w;                                                                                 \
            const v3 wn = w + ax_ * qd_;                                                                            \
            const v3 aln = al + cross(w, ax_) * qd_;                                                                \
            const v3 d = p_ - pp;                                                                                   \
            const v3 apn = ap + cross(al, d) + cross(w, cross(w, d));                                               \
            const bool on = (K) < plen;                                                                             \
            w = p16_sel3(on, wn, w); al = p16_sel3(on, aln, al); ap = p16_sel3(on, apn, ap); pp = p16_sel3(on, p_, pp); \
        }
        P16_RNEA_LEVEL(0, 0, 0) P16_RNEA_LEVEL(1, 1, 1) P16_RNEA_LEVEL(2, 2, 2) P16_RNEA_LEVEL(3, 3, 3) P16_RNEA_LEVEL(4, 4, 4)
        P16_RNEA_LEVEL(5, 5, 5) P16_RNEA_LEVEL(6, 6, 6) P16_RNEA_LEVEL(7, 7, 9) P16_RNEA_LEVEL(8, 8, 10)
#undef P16_RNEA_LEVEL
        const v3 r = bcom - bp;
        const v3 ac = ap + cross(al, r) + cross(w, cross(w, r));
        const v3 F = ac * mass_l;
        const v3 Nn = mulv(bI, al) + cross(w, mulv(bI, w)) + cross(r, F);
        // the force pass as subtree sums: a body's force and its torque about the wrist (body 6's joint: the reference point sits
        // where the small torques are), summed over the body's subtree leaf to root -- a tree edge child -> parent is "lane l takes
        // lane l + 1" (row_shl:1) except 9 -> 6 --, then referred back to the body's own joint: N = G - (p - o) x F
        const float4 o4 = *(const float4 *)&lds[PL_BQ + 8 * 6 + 4];
        const v3 ro = bp - mk(o4.x, o4.y, o4.z);
        const v3 G = Nn + cross(ro, F);
        float s0 = l < NB ? F.x : 0.0f, s1 = l < NB ? F.y : 0.0f, s2 = l < NB ? F.z : 0.0f, s3 = l < NB ? G.x : 0.0f, s4 = l < NB ? G.y : 0.0f, s5 = l < NB ? G.z : 0.0f;
#define P16_EDGE(DPP, MASK)                                                                                         \
        {                                                                                                           \
            const float m_ = (MASK) ? 1.0f : 0.0f;                                                                  \
            asm("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %6 " DPP " row_mask:0xf bank_mask:0xf\n\tv_fmac_f32_dpp %1, %1, %6 " DPP " row_mask:0xf bank_mask:0xf\n\t" \
                "v_fmac_f32_dpp %2, %2, %6 " DPP " row_mask:0xf bank_mask:0xf\n\tv_fmac_f32_dpp %3, %3, %6 " DPP " row_mask:0xf bank_mask:0xf\n\t"           \
                "v_fmac_f32_dpp %4, %4, %6 " DPP " row_mask:0xf bank_mask:0xf\n\tv_fmac_f32_dpp %5, %5, %6 " DPP " row_mask:0xf bank_mask:0xf"               \
                : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4), "+v"(s5) : "v"(m_));                            \
        }
        P16_EDGE("row_shl:1", l == 9 || l == 7)          // 10 -> 9, 8 -> 7
        P16_EDGE("row_newbcast:9", l == 6)               // 9 -> 6
        P16_EDGE("row_shl:1", l == 6)                    // 7 -> 6
        P16_EDGE("row_shl:1", l == 5) P16_EDGE("row_shl:1", l == 4) P16_EDGE("row_shl:1", l == 3) P16_EDGE("row_shl:1", l == 2)
        P16_EDGE("row_shl:1", l == 1) P16_EDGE("row_shl:1", l == 0)
#undef P16_EDGE
        const v3 Nt = mk(s3, s4, s5) - cross(ro, mk(s0, s1, s2));
        bias_l = dot(bax, Nt);
    }
    // ---- Cholesky M = L L^T, row l of L on lane l, column by column (v_rsq_f32 for the diagonal: 1 ulp)
    float Lr[NB], idiag = 0.0f;
#define P16_CHOL_COL(J)                                                                              \
    {                                                                                                \
        float s = Mrow[J];                                                                           \
        _Pragma("unroll") for (int k = 0; k < (J); k++) P16_FNMAC_BCAST(J, s, Lr[k], Lr[k]);         \
        const float idj = __builtin_amdgcn_rsqf(s), dj = s * idj;                                    \
        idiag = l == (J) ? idj : idiag;                                                              \
        float off;                                                                                   \
        P16_MUL_BCAST(J, off, idj, s);                                                               \
        Lr[J] = l == (J) ? dj : (l > (J) ? off : 0.0f);                                              \
    }
    P16_CHOL_COL(0) P16_CHOL_COL(1) P16_CHOL_COL(2) P16_CHOL_COL(3) P16_CHOL_COL(4) P16_CHOL_COL(5) P16_CHOL_COL(6) P16_CHOL_COL(7)
    P16_CHOL_COL(8) P16_CHOL_COL(9) P16_CHOL_COL(10)
#undef P16_CHOL_COL
    // ---- M^-1: lane c solves L y = e_c, L^T x = y for column c (the factor's rows broadcast from their lanes, folded into the multiply-adds)
    float xc[NB];
    {
        float y[NB];
#define P16_FWD(I)                                                                                   \
        {                                                                                            \
            float s = l == (I) ? 1.0f : 0.0f;                                                        \
            _Pragma("unroll") for (int k = 0; k < (I); k++) P16_FNMAC_BCAST(I, s, Lr[k], y[k]);      \
            P16_MUL_BCAST(I, y[I], idiag, s);                                                        \
        }
        P16_FWD(0) P16_FWD(1) P16_FWD(2) P16_FWD(3) P16_FWD(4) P16_FWD(5) P16_FWD(6) P16_FWD(7) P16_FWD(8) P16_FWD(9) P16_FWD(10)
#undef P16_FWD
#define P16_BWD(I)                                                                                   \
        {                                                                                            \
            float s = y[I];                                                                          \
            if ((I) < 1) P16_FNMAC_BCAST(1, s, Lr[I], xc[1]);                                        \
            if ((I) < 2) P16_FNMAC_BCAST(2, s, Lr[I], xc[2]);                                        \
            if ((I) < 3) P16_FNMAC_BCAST(3, s, Lr[I], xc[3]);                                        \
            if ((I) < 4) P16_FNMAC_BCAST(4, s, Lr[I], xc[4]);                                        \
            if ((I) < 5) P16_FNMAC_BCAST(5, s, Lr[I], xc[5]);                                        \
            if ((I) < 6) P16_FNMAC_BCAST(6, s, Lr[I], xc[6]);                                        \
            if ((I) < 7) P16_FNMAC_BCAST(7, s, Lr[I], xc[7]);                                        \
            if ((I) < 8) P16_FNMAC_BCAST(8, s, Lr[I], xc[8]);                                        \
            if ((I) < 9) P16_FNMAC_BCAST(9, s, Lr[I], xc[9]);                                        \
            if ((I) < 10) P16_FNMAC_BCAST(10, s, Lr[I], xc[10]);                                     \
            P16_MUL_BCAST(I, xc[I], idiag, s);                                                       \
        }
        P16_BWD(10) P16_BWD(9) P16_BWD(8) P16_BWD(7) P16_BWD(6) P16_BWD(5) P16_BWD(4) P16_BWD(3) P16_BWD(2) P16_BWD(1) P16_BWD(0)
#undef P16_BWD
    }
    // ---- outputs: M^-1 (lane c stores column c: eleven consecutive floats per row across the lanes), the unconstrained velocities
    // qd* = qd + dt M^-1 (-bias - damping qd), row i of M^-1 through LDS
    if (l < NB) {
#pragma unroll
        for (int i = 0; i < NB; i++) {
            if (body_lane) SCR(S_MINV + i * NB + l) = xc[i];
            lds[PL_X + 12 * i + l] = xc[i];
        }
    }
    P16_SYNC();
    {
        const float rhs_l = -bias_l - damp_l * qd_l;
        const float4 x0 = *(const float4 *)&lds[PL_X + 12 * lb], x1 = *(const float4 *)&lds[PL_X + 12 * lb + 4], x2 = *(const float4 *)&lds[PL_X + 12 * lb + 8];
        float qdd = 0.0f;
        P16_FMAC_BCAST(0, qdd, rhs_l, x0.x); P16_FMAC_BCAST(1, qdd, rhs_l, x0.y); P16_FMAC_BCAST(2, qdd, rhs_l, x0.z); P16_FMAC_BCAST(3, qdd, rhs_l, x0.w);
        P16_FMAC_BCAST(4, qdd, rhs_l, x1.x); P16_FMAC_BCAST(5, qdd, rhs_l, x1.y); P16_FMAC_BCAST(6, qdd, rhs_l, x1.z); P16_FMAC_BCAST(7, qdd, rhs_l, x1.w);
        P16_FMAC_BCAST(8, qdd, rhs_l, x2.x); P16_FMAC_BCAST(9, qdd, rhs_l, x2.y); P16_FMAC_BCAST(10, qdd, rhs_l, x2.z);
        if (body_lane) SCR(S_QDS + l) = qd_l + P.dt * qdd;
    }
}
template <int PHASE>
__device__ __forceinline__ void prep16_class(const BodyParams &B, const SimParams &P, const DevPtrs &D, int sel, int order_n) {
    if (order_n > 0 && (int)blockIdx.x >= (int)gridDim.x - 8) {
        if (threadIdx.x < 64) dispatch_order_class<64>((int)blockIdx.x - ((int)gridDim.x - 8), order_n, 1, (order_n + 7) >> 3, D.collide_cost, D.collide_bin, D.collide_perm);
        return;
    }
    if (PHASE != 2 && threadIdx.x >= 64) { prep16_objects(B, P, D, sel); return; }
    prep16_body<PHASE>(B, P, D, sel);
}
__global__ void __launch_bounds__(128) k_prep_a16(BodyParams B, SimParams P, DevPtrs D, int sel, int zero_counts, int order_n) {
    if (zero_counts && blockIdx.x == 0 && threadIdx.x == 0) {       // in-line pass: the frame k_collide is about to fill holds stale counts
        D.hcount_next[0] = 0; D.hcount_next[1] = 0; D.hcount2_next[0] = 0; D.hcount2_next[1] = 0;
    }
    prep16_class<1>(B, P, D, sel, order_n);
}
__global__ void __launch_bounds__(64) k_prep_b16(BodyParams B, SimParams P, DevPtrs D, int sel) { prep16_class<2>(B, P, D, sel, 0); }
__global__ void __launch_bounds__(128) k_prep_ab16(BodyParams B, SimParams P, DevPtrs D, int sel, int order_n) { prep16_class<0>(B, P, D, sel, order_n); }
