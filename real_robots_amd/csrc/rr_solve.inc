// rr_solve.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_solve / k_solve_rs / k_solve_light_ow: command part, row build, projected Gauss-Seidel, integration
// ---------------------------------------------------------------------------------------------- k_solve
__device__ __forceinline__ void plane_space(v3 n, v3 &p, v3 &q) {   // btPlaneSpace1
    if (fabsf(n.z) > 0.70710678118654752440f) {
        float a = n.y * n.y + n.z * n.z;
        float k = 1.0f / sqrtf(a);
        p = mk(0, -n.z * k, n.y * k);
        q = mk(a * k, -n.x * p.z, n.x * p.y);
    } else {
        float a = n.x * n.x + n.y * n.y;
        float k = 1.0f / sqrtf(a);
        p = mk(-n.y * k, n.x * k, 0);
        q = mk(-n.z * p.y, n.z * p.x, a * k);
    }
}

// ---- solver ------------------------------------------------------------------------------------------------------
// One env per 16-lane group (4 envs per wavefront, SGRP groups per workgroup).  The PGS chain of an env is sequential
// (Gauss-Seidel, Bullet's order: motors, limits, all normals, all lateral frictions, all torsional frictions), each SIMD
// runs a single wave, so the kernel lasts as long as the longest chain: what counts is the number of (dependent)
// instructions per row step.  Three kinds of rows:
//   * motor / joint-limit rows: lane j < 11 owns joint j (dq), rows in registers (MOTOR_STEP, LIMIT_STEP);
//   * object-vs-static contacts (objects resting on table / shelf): lane 11 + o owns the
//     velocity change (dv, dw) of object o and sweeps that object's rows on its own -- rows of different objects touch
//     disjoint variables, so the three object lanes run side by side and no cross-lane sum is needed; up to KOS contacts
//     per object, all six rows of each in registers (an object's further contacts with statics take the generic path);
//   * generic contacts (robot involved, two objects, object-static beyond os_cap): SLOT LAYOUT.  Every scalar velocity
//     variable of the env has a fixed (lane, slot):
//         slot A: lanes 0..10 joint velocities dq (the same register as the motor rows'), lanes 11..15 object 2 (v.xyz, w.xy)
//         slot B: lanes 0..5 object 0 (v.xyz, w.xyz), lanes 6..11 object 1, lane 12 object 2 (w.z)
//     and a row is one float4 per lane {J_A, (M^-1 J^T)_A, J_B, (M^-1 J^T)_B} (zeros where the row does not act): a row
//     step is one 16-byte load, two multiply-adds, a four-step DPP sum, the clamp, one DPP broadcast and two
//     multiply-adds -- no role logic, no per-row scalars in memory: rows are swept in blocks of 16, lane k of the group
//     holds {rhs, 1/diag, lambda, bounds} of the block's row k in registers, computes the clamp of "its" row from the
//     common J.v, and the impulse change of row k is lane k's value (DPP row_newbcast k).  The row data (256 B per row,
//     up to 6 rows per contact) does not fit LDS for an env with dozens of contacts; it lives in global memory
//     (D.grows, L2 resident), written once by the row builder and streamed through a register queue eight rows ahead.
//     Object velocities are moved between the object lanes and the slots around each generic sweep, only for the objects
//     that some generic contact of the wave touches.
//   Rows of contacts without normal impulse whose friction impulses are zero have the bounds [-0, 0] and cannot move
//   anything: the friction and torsional sweeps run over compacted lists of the other rows, rebuilt after every normal
//   sweep (94 % of the robot contacts of a pushing gripper are speculative: inside the margin, not touching).
// LDS per env (LF_TOTAL floats): Minv (121), motor rows (11 x {rhs, dinv, lambda}), joint-limit rows (22 x {rhs, lambda}),
// contact meta (48 ints), friction / spinning / rolling coefficients of the object-lane contacts (3 x 12), the objects' data (3 x 20),
// a staging area for 16 contact records, object-lane rows (12 x (3 x 12 linear + 3 x 8 torsional)), generic row scalars (288 x {rhs, dinv, bound coefficient, lambda}), the two row lists.
#define SGRP 4           // envs per workgroup (64 threads)
#define OS_CAP 12        // object-vs-static contacts per env on the object lanes: KOS per object, rows staged in LDS
#define GROWS (6 * MAXC) // generic row ids: 6 j + k for generic contact j; k = 0 normal, 1 2 lateral, 3 spinning, 4 5 rolling
// LF_ZPAD: the scalars of the DUMMY generic contacts MAXC .. MAXC + 3 (all zero: a block step on them is a no-op) -- what a group
// sweeps when another env of its wave has more blocks.  LF_LISTA / LF_LISTT: the active contacts of the friction / torsional
// passes, one byte each, padded with MAXC.
#define LIST_CAP (MAXC + 4)
enum { LF_MINV = 0, LF_MOT = LF_MINV + 124, LF_LIM = LF_MOT + 36, LF_META = LF_LIM + 44, LF_MU = LF_META + MAXC, LF_SPIN = LF_MU + OS_CAP,
       LF_ROLL = LF_SPIN + OS_CAP, LF_OBJ = LF_ROLL + OS_CAP, LF_CST = LF_OBJ + NOBJ * 20, LF_OSL = LF_CST + 16 * 12, LF_OST = LF_OSL + OS_CAP * 36,
       LF_GSC = LF_OST + OS_CAP * 24, LF_ZPAD = LF_GSC + 4 * GROWS, LF_LISTA = LF_ZPAD + 4 * 24, LF_LISTT = LF_LISTA + 16, LF_ENVW = LF_LISTT + 16, LF_TOTAL = LF_ENVW + 4 };
static_assert(LIST_CAP <= 64, "a list of LIST_CAP bytes must fit its 16 floats");
// Global store of the generic rows (D.grows), per env GP_RECS records of 16 lanes x float4:
//   GP_C + j       the normal row of generic contact j in the canonical layout {J_A, MJ_A, J_B, MJ_B} (block repack, warm start)
//   GP_N + 5 b     block of the normal rows of contacts 4 b .. 4 b + 3  {J pair, J pair, MJ pair, MJ pair, cross terms}
//   GP_T + 5 j     block of the torsional rows of contact j (spinning, rolling, rolling, -)
//   GP_F + 3 j     block of the lateral friction rows of contact j {J pair, MJ pair, cross term}
// Block index NBLK4 / contact index MAXC are the dummies: all-zero records nobody writes.
#define NBLK4 (MAXC / 4)
enum { GP_C = 0, GP_N = GP_C + MAXC, GP_T = GP_N + 5 * (NBLK4 + 1), GP_F = GP_T + 5 * (MAXC + 1), GP_RECS = GP_F + 3 * (MAXC + 1) };
#define GP_ENV_BYTES (GP_RECS * 256)
#define SLDS_FLOATS (SGRP * LF_TOTAL)
static_assert(SLDS_FLOATS * 4 * 4 <= 163840, "sixteen envs (four 64-thread workgroups or one 256-thread workgroup) must fit the 160 KiB LDS of a CU");
static_assert(LF_TOTAL % 4 == 0 && LF_OSL % 4 == 0 && LF_OST % 4 == 0 && LF_GSC % 4 == 0 && LF_OBJ % 4 == 0 && LF_CST % 4 == 0, "row parts must be 16-byte aligned");
extern __shared__ __attribute__((aligned(16))) float g_slds[];      // (blockDim.x / 16) x LF_TOTAL floats
#define LD(slot) g_slds[(slot)]

// meta word: bodyA (8) | bodyB (8) | linkA (8) | swept by the object lane (1) | object-lane slot or generic contact index (6)
__device__ __forceinline__ int meta_bodyA(int m) { return (signed char)(m & 255); }
__device__ __forceinline__ int meta_bodyB(int m) { return (signed char)((m >> 8) & 255); }
__device__ __forceinline__ int meta_link(int m) { return (signed char)((m >> 16) & 255); }
__device__ __forceinline__ bool meta_fast(int m) { return (m >> 24) & 1; }
__device__ __forceinline__ int meta_slot(int m) { return (m >> 25) & 63; }
__device__ __forceinline__ bool meta_near(int m) { return m < 0; }     // |distance| < 0.1 (robot.py:136)

// Sum over the 16 lanes of a group (= one DPP row), result in every lane: four rotate-and-add steps on the VALU
// (v_add_f32 with row_ror:8/4/2/1), no LDS crossbar traffic. Every lane performs the same commutative pairings, so
// all 16 lanes hold bitwise the same sum.
template <int ROR>
__device__ __forceinline__ float dpp_ror(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + ROR, 0xf, 0xf, false));
}
// value of lane J of each 16-lane row, in every lane of that row (gfx90a+ DPP row_newbcast)
template <int J> __device__ __forceinline__ float row_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x150 + J, 0xf, 0xf, false));
}
// (the same with a zero `old` operand and bound_ctrl: a form the compiler's DPP combiner can fold into the instruction that uses it)
template <int J> __device__ __forceinline__ float row_bcast_z(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + J, 0xf, 0xf, true));
}
template <int J> __device__ __forceinline__ int row_bcast_i(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x150 + J, 0xf, 0xf, false); }
// value of an arbitrary lane of the wavefront (ds_bpermute; the source lane must be active)
__device__ __forceinline__ float lane_gather(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}
__device__ __forceinline__ int lane_gather_i(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_ror<8>(v);
    v += dpp_ror<4>(v);
    v += dpp_ror<2>(v);
    v += dpp_ror<1>(v);
    return v;
}

// ancestors-or-self of body b as a bit mask over joints (kinematic tree PARENT)
__device__ constexpr unsigned ANC[NB] = {0x001, 0x003, 0x007, 0x00f, 0x01f, 0x03f, 0x07f, 0x0ff, 0x1ff, 0x27f, 0x67f};

// Per-object data a contact row needs (pose, world inverse inertia, unconstrained velocities), fetched once per pair.
struct ObjData { v3 op, vs, ws; m3 Iinv; float imass; };

// What a lane owns in the slot layout: its object (or -1) and the unit vectors that pick its component out of a
// (linear, angular) pair -- J = lin . el + ang . ea.
struct SlotOwner { int objA, objB; v3 elA, eaA, elB, eaB; };
__device__ __forceinline__ v3 unit3(int c) { return mk(c == 0 ? 1.0f : 0.0f, c == 1 ? 1.0f : 0.0f, c == 2 ? 1.0f : 0.0f); }
__device__ __forceinline__ SlotOwner slot_owner(int l) {
    SlotOwner s;
    const int cA = l - NB;                                   // slot A, lanes 11..15: object 2, components 0..4
    s.objA = l >= NB ? 2 : -1;
    s.elA = unit3(cA < 3 ? cA : -1); s.eaA = unit3(cA >= 3 ? cA - 3 : -1);
    const int cB = l < 6 ? l : (l < 12 ? l - 6 : 5);         // slot B: object 0 | object 1 | object 2 component 5
    s.objB = l < 6 ? 0 : (l < 12 ? 1 : (l == 12 ? 2 : -1));
    s.elB = unit3(cB < 3 ? cB : -1); s.eaB = unit3(cB >= 3 ? cB - 3 : -1);
    return s;
}

// Generic rows in the slot layout, built per contact in two stages so that a row costs a handful of dot products:
//   stage 1 (once per contact): for this lane's slot-A and slot-B variable the vectors g, h with
//       J = dir . g,   (M^-1 J^T) = dir . h        for a linear row along `dir` at the contact point
//     and gt, ht likewise for a torsional row about `dir`.  Joint lane l (slot A): g = +-(a_l x (x - p_l)) for the ancestors
//     of the contact's robot body, gt = +-a_l, M^-1 J^T by the row of Minv; an object component lane: with e the unit vector
//     of its component, r = x - object position, s = +1 (body A) / -1 (body B):
//       linear component    g = s e,            h = s e / m
//       angular component   g = s (e x r),      h = s ((I^-1 e) x r)      [(r x d) . e = d . (e x r), I^-1 symmetric]
//     torsional row:        gt = s e (angular components only), ht = s I^-1 e
//   stage 2 (per row): four dot products, the 11-step Minv product for the joint lanes, two group sums, one store.
// Branch-free: the four envs of a wave have different body types.
struct GrowCtx { v3 gA, hA, gtA, htA, gB, hB, gtB, htB; };
__device__ __forceinline__ void grow_slot(int myobj, v3 el, v3 ea, int bodyA, int bodyB, v3 x, const ObjData &oA, const ObjData &oB,
                                          v3 &g, v3 &h, v3 &gt, v3 &ht) {
    const bool isA = myobj >= 0 && bodyA == 16 + myobj, isB = myobj >= 0 && bodyB == 16 + myobj;
    const float s = isA ? 1.0f : (isB ? -1.0f : 0.0f);
    const v3 op = isA ? oA.op : oB.op;
    const float im = isA ? oA.imass : oB.imass;
    m3 Ii;
#pragma unroll
    for (int k = 0; k < 9; k++) Ii.m[k] = isA ? oA.Iinv.m[k] : oB.Iinv.m[k];
    const v3 r = x - op;
    const v3 Iea = mulv(Ii, ea);
    g = (el + cross(ea, r)) * s;
    h = (el * im + cross(Iea, r)) * s;
    gt = ea * s;
    ht = Iea * s;
}

// Row step of an object-vs-static contact row held in registers, executed by the lane that owns the object only:
// b0,b1,b2 = the row (dir.xy dir.z ang.x | ang.yz dir.z mang.x | mang.yz rhs dinv), lambda in `lam`, bounds [lo, hi]; the
// object's velocity change lives in three register pairs V01 = (v.x v.y), V23 = (v.z w.x), V45 = (w.y w.z): J.v is three
// packed multiply-adds and one add, the update three packed FMAs (v_pk_fma_f32: two lanes' worth of fp32 per issue slot).
// An all-zero row with lam = 0 is a
// no-op (dl = 0), which is how absent rows are represented -- no predicates, no scalar mask registers.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
#define P2(a, b) (v2f{(a), (b)})
#define REG_ROW_STEP(b0, b1, b2, lam, lo, hi)                                                                     \
    do {                                                                                                          \
        v2f p_ = P2((b0).x, (b0).y) * V01;                                                                        \
        p_ = pk_fma(P2((b0).z, (b0).w), V23, p_);                                                                 \
        p_ = pk_fma(P2((b1).x, (b1).y), V45, p_);                                                                 \
        const float jv_ = p_.x + p_.y;                                                                            \
        const float s0_ = fmaf(-jv_, (b2).w, (lam) + (b2).z);       /* (lambda + rhs) - dinv * J.v */             \
        const float sum_ = __builtin_amdgcn_fmed3f(s0_, (lo), (hi));                                              \
        const float dl_ = sum_ - (lam);                                                                           \
        (lam) = sum_;                                                                                             \
        const float sm_ = dl_ * inv_mass;                                                                         \
        V01 = pk_fma(P2((b0).x, (b0).y), P2(sm_, sm_), V01);                                                      \
        V23 = pk_fma(P2((b1).z, (b1).w), P2(sm_, dl_), V23);                                                      \
        V45 = pk_fma(P2((b2).x, (b2).y), P2(dl_, dl_), V45);                                                      \
    } while (0)
// (the components of the pairs by name)
#define DVX V01.x
#define DVY V01.y
#define DVZ V23.x
#define DWX V23.y
#define DWY V45.x
#define DWZ V45.y
#define KLIM 2           // joint-limit rows kept in registers (usually two: the finger lower limits)
#define KOS 4            // object-vs-static contacts per object kept in registers (a resting object has <= 4)

__device__ __forceinline__ float4 sel4(bool has, float4 v) {
    return make_float4(has ? v.x : 0.0f, has ? v.y : 0.0f, has ? v.z : 0.0f, has ? v.w : 0.0f);
}

// sel 0: wave b handles the envs 4 b .. 4 b + 3; 1: the same, but heavy envs are left out (their 16 lanes run along as no-ops);
// 2: wave w of the launch handles the heavy envs 4 w .. 4 w + 3 of D.hlist -- packed four to a wave whichever groups they
// come from (256-thread workgroups: sixteen heavy envs fill a CU's LDS and leave the other CUs to the render of the light
// envs).  No result depends on which envs share a wave: only trip counts and the choice between equivalent code paths do.
// One object-vs-static contact row pair along / about `dir` (k = 0: the normal, 1 2: the tangents): the linear row
// {dir, ang, I^-1 ang, rhs, 1/diag} and the torsional row about the same axis {I^-1 dir, rhs, 1/diag}, written to the LDS
// row areas of slot `slot`.  Used by the sequential row builder (lanes 0..2 of a group take k = lane) and by the
// lane-per-contact builder of the light form (one lane, k = 0..2): the same expressions, hence the same bits.
__device__ __forceinline__ void os_row_pair(int k, v3 dir, v3 x, const ObjData &oA, float dist, float rest, float spin, float roll, float lam0,
                                            float dt, float erp, float rest_thresh, int row_osl, int row_ost) {
    const v3 ang = cross(x - oA.op, dir);
    const v3 mang = mulv(oA.Iinv, ang);
    const float diag = dot(dir, dir) * oA.imass + dot(ang, mang);
    const float rel = dot(dir, oA.vs) + dot(ang, oA.ws);
    const float dinv = diag > 0 ? 1.0f / diag : 0.0f;
    float rr = 0;
    if (fabsf(rel) >= rest_thresh) { rr = rest * -rel; if (rr < 0) rr = 0; }
    float verr = rr - rel, perr = 0;
    if (dist > 0) verr -= dist / dt;
    else perr = -dist * erp / dt;
    const float rhs = k == 0 ? (perr + verr) * dinv : -rel * dinv;
    // torsional: pure rotation about dir; absent (coefficient 0) rows are all-zero
    const float coef = k == 0 ? spin : roll;
    const v3 tm = mulv(oA.Iinv, dir);
    const float tdiag = dot(dir, tm);
    const float tdinv = (coef > 0 && tdiag > 0) ? 1.0f / tdiag : 0.0f;
    const float trhs = -dot(dir, oA.ws) * tdinv;
    // (layout: REG_ROW_STEP / REG_TORS_STEP take the row in aligned pairs -- packed fp32 operations on (v.x v.y) (v.z w.x) (w.y w.z))
    float4 *bp4 = (float4 *)&LD(row_osl);
    bp4[0] = make_float4(dir.x, dir.y, dir.z, ang.x);
    bp4[1] = make_float4(ang.y, ang.z, dir.z, mang.x);
    bp4[2] = make_float4(mang.y, mang.z, rhs, dinv);
    float4 *tp4 = (float4 *)&LD(row_ost);
    tp4[0] = make_float4(tm.x, trhs, tm.y, tm.z);
    tp4[1] = make_float4(tdinv, k == 0 ? lam0 : 0.0f, 0.0f, 0.0f);      // (.y of the normal row: warm-start impulse)
}

// ---------------------------------------------------------------------------------------------- render setup
// mvp = VP [R p; 0 1] of one render instance: the one 4x4 product of the camera with a model matrix (instance_setup_core)
__device__ __forceinline__ void instance_mvp(const float *VP, const m3 &R, const v3 &p, float (&mvp)[16]) {
#pragma clang fp contract(off)
    const float xf[12] = {R.m[0], R.m[1], R.m[2], R.m[3], R.m[4], R.m[5], R.m[6], R.m[7], R.m[8], p.x, p.y, p.z};
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int r = e >> 2, c = e & 3;
        float a = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) a += VP[4 * r + k] * (c < 3 ? xf[3 * k + c] : xf[9 + k]);
        a += VP[4 * r + 3] * (c == 3 ? 1.0f : 0.0f);
        mvp[e] = a;
    }
}
// Instance transforms for the rasteriser, one thread per (env, instance): a robot-link thread composes the joint
// transforms of its body's ancestors only (same operations, in the same order, as fk_all() for that chain), an object
// thread converts the object's quaternion; the 12 floats of an instance are stored as three 16-byte words, so a wave
// writes a contiguous span.  (One thread per env needed 264 stores with a 1.5 KB stride between lanes.)
// instance i of env: FK of its owner's ancestor chain -> model-view-projection matrix and shading constants (D.inst_xf).
// qj: the robot's joint angles; op7: pose {x y z, quaternion} of the instance's object (read for an object instance only).
// Two callers: k_render_setup (values from the state) and the light solve, which runs it on the values it has just
// integrated (registers / LDS) -- the same operations on the same floats, hence the same bits.
__device__ __forceinline__ void instance_setup_core(const BodyParams &B, const RenderModel &RM, const DevPtrs &D, int env, int i, int ot, int oi,
                                                    const float (&qj)[NB], const float (&op7)[7]) {
    m3 R = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    v3 p = mk(0, 0, 0);
    if (ot == 1) {
        unsigned anc = 0;
#pragma unroll
        for (int b = 0; b < NB; b++) if (oi == b) anc = ANC[b];
        p = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            if (!((anc >> b) & 1u)) continue;
            m3 jr;
#pragma unroll
            for (int k = 0; k < 9; k++) jr.m[k] = B.jrot[b][k];
            const m3 Rj = nc::mul(R, jr);
            const v3 ax = mk(B.axis[b][0], B.axis[b][1], B.axis[b][2]);
            p = nc::add(p, nc::mulv(R, mk(B.jpos[b][0], B.jpos[b][1], B.jpos[b][2])));
            R = nc::mul(Rj, nc::axis_angle(ax, qj[b]));
        }
    } else if (ot == 2) {
        R = nc::quat_to_m3(op7[3], op7[4], op7[5], op7[6]);
        p = mk(op7[0], op7[1], op7[2]);
    }
    // mvp = VP * [R p; 0 1] (same summation order as the oracle's 4x4 product, no FMA contraction), then the shading
    // constants: the raster and shading workgroups just copy these 128 bytes per instance into LDS.  VP is the env's own
    // camera with per-env cameras (several envs per wave here: vector loads), else the handle's (scalar loads, as before).
    float mvp[16];
    if (D.env_cam) instance_mvp(D.env_cam + (size_t)env * cam_floats(RM.ntiles) + CAM_VP, R, p, mvp);
    else instance_mvp(RM.VP, R, p, mvp);
    const int tidx = RM.in_tex[i];
    float4 *o = (float4 *)(D.inst_xf + ((size_t)env * MAXINST + i) * 32);
    o[0] = make_float4(mvp[0], mvp[1], mvp[2], mvp[3]);
    o[1] = make_float4(mvp[4], mvp[5], mvp[6], mvp[7]);
    o[2] = make_float4(mvp[8], mvp[9], mvp[10], mvp[11]);
    o[3] = make_float4(mvp[12], mvp[13], mvp[14], mvp[15]);
    o[4] = make_float4(R.m[0], R.m[1], R.m[2], R.m[3]);
    o[5] = make_float4(R.m[4], R.m[5], R.m[6], R.m[7]);
    // the instance's colour: the model's, or this env's own (rr_set_env_appearance)
    const float *col = D.env_colour ? D.env_colour + ((size_t)env * MAXINST + i) * 3 : RM.in_color[i];
    o[6] = make_float4(R.m[8], col[0], col[1], col[2]);
    o[7] = make_float4(__int_as_float(tidx >= 0 ? RM.tex_off[tidx] : 0), __int_as_float(tidx >= 0 ? RM.tex_w[tidx] : 0),
                       __int_as_float(tidx >= 0 ? RM.tex_h[tidx] : 0), __int_as_float(RM.in_uid[i]));
}
__device__ __forceinline__ void instance_setup(const BodyParams &B, const SimParams &P, const RenderModel &RM, const DevPtrs &D, int env, int i) {
    const int N = P.N;
    const float *state = D.state;
    const int ot = RM.in_otype[i], oi = RM.in_oidx[i];
    float qj[NB] = {0}, op7[7] = {0};
    if (ot == 1) {                 // all joint angles requested up front: one round trip instead of one per ancestor
#pragma unroll
        for (int b = 0; b < NB; b++) qj[b] = STT(ST_Q + b);
    } else if (ot == 2) {
#pragma unroll
        for (int k = 0; k < 3; k++) op7[k] = STT(ST_OPOS + 3 * oi + k);
#pragma unroll
        for (int k = 0; k < 4; k++) op7[3 + k] = STT(ST_OQUAT + 4 * oi + k);
    }
    instance_setup_core(B, RM, D, env, i, ot, oi, qj, op7);
}

// GEN = false is the form for the light envs (sel 1): no generic contact row can occur there (k_collide classifies by the
// very rule the row builder uses), so everything of the generic path -- the row builder, the streamed sweeps, their register
// queue -- folds away at compile time and the sweep of motors, limits and object-lane rows runs without the register
// spills (v_accvgpr_read: a third of the torsional steps' instructions) the full kernel needs.  Same source, same
// arithmetic: results do not depend on which form solved an env (split-equivalence tests, bitwise).
// The light form runs with an object wave: workgroups of five waves solve sixteen envs -- waves 0..3 are the envs' 16-lane groups
// (command part, row build, the robot's rows, joint integration), wave 4 runs the object chains of all sixteen envs, one LANE per
// (env, object) (light_object_wave below).  In a light env the robot's rows and each object's rows are separate problems;
// with the object rows on lanes 11..13 of every group 62 % of a sweep's instructions ran with 3 of 16 lanes live.
__device__ void light_object_wave(const BodyParams &B, const SimParams &P, const DevPtrs &D, const RenderModel *RMp);
#ifndef LIGHT_OW_THREADS
#define LIGHT_OW_THREADS 384
#endif
#define OW_FLAGS 0       // L_GSC words of an env that its group publishes for the object wave: flags (1 light env of this launch, 2 does not step)
#define OW_MASK 1        // .. +3: the contacts (bit = list index) of object 0 / 1 / 2
#define OW_QUAT 4        // .. +12: the objects' orientations at the start of the step (after the out-of-bounds rule)
// RSETUP: the kernel also sets up the render instances of its envs (RMp).  A template parameter, not just a null pointer: with the
// set-up code in its tail the generic kernel's sweep loop comes out 3 % slower (register allocation), which a step without camera --
// config 2 -- must not pay.
template <bool GEN, bool RSETUP = !GEN>
__device__ __forceinline__ void solve_body(const BodyParams &B, const SimParams &P, const DevPtrs &D, int sel, int coop_launch, const RenderModel *RMp = nullptr) {
    const int N = P.N;
    if (sel <= 1 && blockIdx.x == 0 && threadIdx.x == 0) {
        // (once per step, by the launch every step has: the bookkeeping of the contact frame this step's look-ahead will fill;
        // the number of heavy / very heavy envs of this step goes to pinned host memory on the way -- a posted write)
        if (D.hcount_host) { D.hcount_host[0] = D.hcount[0]; D.hcount_host[1] = D.hcount2[0]; }
        D.hcount_next[0] = 0; D.hcount_next[1] = 0; D.hcount2_next[0] = 0; D.hcount2_next[1] = 0;
    }
#if LIGHT_OW_THREADS == 384
    // wave roles O J J J - J: waves w and w + 4 of a workgroup land on the same SIMD (tools/ubench/simd_map.hip), so the object
    // wave has its SIMD to itself -- wave 4 only keeps the workgroup's barrier company and ends -- and two of the four group
    // waves share one (together as many issue slots as the object wave).  Object wave 53 -> 37 us (scratch/sprof_light.py), the
    // kernel 56.7 -> 54.3 us, the step 0.691 -> 0.685 ms.  (LIGHT_OW_THREADS 320: J J J J O, the object wave shares with a group wave.)
    int jwave = 0;
    if (!GEN) {
        const int wv = threadIdx.x >> 6;
        if (wv == 0) { light_object_wave(B, P, D, RMp); return; }
        if (wv == 4) { __syncthreads(); return; }
        jwave = wv < 4 ? wv - 1 : 3;
    }
    const int grp = !GEN ? 4 * jwave + ((threadIdx.x >> 4) & 3) : threadIdx.x >> 4, l = threadIdx.x & 15;
#else
    if (!GEN && (threadIdx.x >> 6) == 4) { light_object_wave(B, P, D, RMp); return; }
    const int grp = threadIdx.x >> 4, l = threadIdx.x & 15;
#endif
    const int unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // the wave's index in the launch
    // coop (a heavy / very heavy list of at most COOP_MAX envs -- the host's lagged count decides, any actual count is handled):
    // ONE env per wave -- its four 16-lane groups build the rows of four contacts at a time (the row build of an env at the
    // contact cap is a fifth of its chain with 16 lanes); group 0 then sweeps, groups 1..3 run along as no-ops.  The wave has
    // one LDS region (the launch asks for a quarter of the LDS of the packed form: the same sixteen envs per CU).  Same
    // arithmetic per row whichever group builds it: results do not depend on the mode (tested bitwise).
    const bool coop = GEN && coop_launch && (sel >= 2 || sel == 0);    // (sel 0: every env its own wave -- batches of at most one wave per SIMD, rr_step)
    const int cg = coop ? (grp & 3) : 0;                              // this group's place among the builders of its env
    int env_raw = !GEN ? 16 * (int)blockIdx.x + grp : (coop ? unit : 4 * unit + (grp & 3));
    bool mine = true;                                                 // this 16-lane group has an env to solve in this launch
    if (sel == 2) { mine = env_raw < *D.hcount; env_raw = mine ? D.hlist[env_raw] : N; }
    else if (sel == 3) { mine = env_raw < *D.hcount2; env_raw = mine ? D.hlist2[env_raw] : N; }
    else if (sel == 1) mine = env_raw < N && D.hgflag[env_raw] == 0;
    if (GEN && __ballot(mine) == 0ull) return;                        // (wave-uniform; the light form: every wave goes to the workgroup's barrier)
    int env = env_raw < N ? env_raw : N - 1;                          // groups without an env run along as no-ops
    float *state = D.state, *scratch = D.scratch;
    const int lj = l < NB ? l : 0;               // joint owned by this lane (lanes >= 11 alias joint 0, masked)
    const int lo_ = (l >= NB && l < NB + NOBJ) ? l - NB : -1;   // object owned by this lane
    const ShapeData *S = D.shapes;
    const int fix = (coop ? (grp >> 2) : grp) * LF_TOTAL;            // (coop: the four groups of a wave share its one LDS region)
    const int L_MINV = fix + LF_MINV, L_MOT = fix + LF_MOT, L_LIM = fix + LF_LIM, L_META = fix + LF_META, L_MU = fix + LF_MU,
              L_SPIN = fix + LF_SPIN, L_ROLL = fix + LF_ROLL, L_OSL = fix + LF_OSL, L_OST = fix + LF_OST, L_GSC = fix + LF_GSC,
              L_OBJ = fix + LF_OBJ, L_CST = fix + LF_CST;
    unsigned char *listA = (unsigned char *)&LD(fix + LF_LISTA), *listT = (unsigned char *)&LD(fix + LF_LISTT);
    const float dt = P.dt, inv_dt = 1.0f / P.dt;
    SPROF_INIT
    SBLK_BEGIN
    // ---- stage-in: EVERY global load of the env's inputs is issued here, before anything is computed from them or stored (a
    // global round trip costs ~7000 cycles at one wave per SIMD, and a store in between would hold the later loads back):
    // error flags, command, the lane's joint state and frame, M^-1 (staged in LDS below), the contact count, the first 16
    // contact records with their inherited impulses, the object lanes' data.
    const unsigned ef0 = (mine && env_raw < N) ? D.errflags[env] : 1u;
    const int lc = l < 9 ? l : 0;
    const float cmd_v = D.cmd_in[(size_t)env * 9 + lc];
    const float act_md = B.act_maxdiff[lc], act_lo = B.act_min[lc], act_hi = B.act_max[lc];
    const float q_l = STT(ST_Q + lj), qds_l = SCR(S_QDS + lj);
    float minv_stage[8];
#pragma unroll
    for (int i = 0; i < 8; i++) minv_stage[i] = SCR(S_MINV + min(l + 16 * i, NB * NB - 1));
    const v3 pk_l = mk(SCR(S_BP + 3 * lj), SCR(S_BP + 3 * lj + 1), SCR(S_BP + 3 * lj + 2));
    const v3 ak_l = mk(SCR(S_BAX + 3 * lj), SCR(S_BAX + 3 * lj + 1), SCR(S_BAX + 3 * lj + 2));
    const int ccount_in = D.ccount[env];
    const int cls_in = sel == 0 ? D.hgflag[env] : sel - 1;           // (sel 1 / 2 / 3: the launch's class)
    float cw0, cw1, cw2;              // warm-start impulses of contacts l, 16 + l, 32 + l
    float4 cr0, cr1, cr2, cr3, cr4, cr5, cr6, cr7, cr8;   // lane l's float4 #(l + 16 i) of the list: cr0..2 = the first 16 records
    {
        const float4 *cl = D.clist + (size_t)env * MAXC * 3;
        cr0 = cl[l]; cr1 = cl[16 + l]; cr2 = cl[32 + l];
        cr3 = cr4 = cr5 = cr6 = cr7 = cr8 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (GEN && __ballot(ccount_in > 16) != 0ull) {  // (a light env has at most 12 contacts, all on the object lanes; a heavy one
            cr3 = cl[48 + l]; cr4 = cl[64 + l]; cr5 = cl[80 + l];     //  with more than 16 pays a second round trip for the other 32 records)
            cr6 = cl[96 + l]; cr7 = cl[112 + l]; cr8 = cl[128 + l];
        }
        const float *cwp = D.cwarm + (size_t)env * MAXC;
        cw0 = cwp[l]; cw1 = cwp[16 + l]; cw2 = cwp[32 + l];       // (unconditional: selected by the count below)
    }
    // the object lanes: the pose that counts (k_prep: the home pose when the out-of-bounds rule fires), inverse inertia,
    // unconstrained velocities; the raw position decides whether the rule fires (then this kernel writes the home pose into the state)
    ObjData myobj;
    const int ob_l = (l >= NB && l < NB + NOBJ && l - NB < P.nobj) ? l - NB : 0;
    const float raw_x = STT(ST_OPOS + 3 * ob_l), raw_z = STT(ST_OPOS + 3 * ob_l + 2);
    float oquat[4];                   // orientation at the start of the step (replaced by the home orientation below if the rule fires)
#pragma unroll
    for (int k = 0; k < 4; k++) oquat[k] = STT(ST_OQUAT + 4 * ob_l + k);
    myobj.op = mk(SCR(S_OP + 3 * ob_l), SCR(S_OP + 3 * ob_l + 1), SCR(S_OP + 3 * ob_l + 2));
#pragma unroll
    for (int kk = 0; kk < 9; kk++) myobj.Iinv.m[kk] = SCR(S_OIINV + 9 * ob_l + kk);
    myobj.vs = mk(SCR(S_OVS + 3 * ob_l), SCR(S_OVS + 3 * ob_l + 1), SCR(S_OVS + 3 * ob_l + 2));
    myobj.ws = mk(SCR(S_OWS + 3 * ob_l), SCR(S_OWS + 3 * ob_l + 1), SCR(S_OWS + 3 * ob_l + 2));
    myobj.imass = 1.0f / D.obj_dyn[(size_t)(4 * ob_l) * N + env];          // (the env's own mass: rr_set_object_dynamics)
    // the lane's actuator: gains and impulse bound of its joint's motor (the env's own: rr_set_env_actuators)
    const float *ea_l = D.env_act + ((size_t)lj * N + env);
    const float act_kp = ea_l[0], act_kd = ea_l[(size_t)NB * N], act_imp = ea_l[(size_t)(2 * NB) * N];
    // ---- the command part of the step -- everything that needs the action: limitActionByJoint (env.py:314-321), the clipping
    // and gripper coupling of Kuka.apply_action (robot.py:188-201) -> the motor target of this lane's joint; a non-finite
    // command flags the env (robot.py:189 asserts) and the env does not step.  It also APPLIES the out-of-bounds rule
    // (env.py:257-264) to the state: the state part of the preparation only derived the collision inputs from the re-posed object.
    float tgt_l = 0.0f;
    bool rejected = false;
    {
        const float cur = l == 8 ? -q_l : q_l;                           // robot.py:203-211 (lanes 0..8: q_l is joint l)
        float d = cmd_v - cur;                                           // env.py:314-321
        d = fminf(d, act_md);
        d = fmaxf(d, -act_md);
        float a = cur + d;
        a = fmaxf(act_lo, fminf(a, act_hi));                             // robot.py:192
        const float a7 = row_bcast<7>(a);
        if (l == 8) a = fmaxf(0.0f, fminf(2.0f * a7, a));                // robot.py:193
        const float a8 = row_bcast<8>(a);
        tgt_l = l < 7 ? a : ((l == 7 || l == 9) ? a7 : -a8);             // robot.py:195-201 (lanes 8, 10: -a8)
        rejected = ((unsigned)(__ballot(l < 9 && !isfinite(cmd_v)) >> (16 * (grp & 3))) & 0xffffu) != 0u;
    }
    const bool frozen = (ef0 & 1u) != 0u;
    bool dead = frozen || (ef0 & ~11u) != 0u || rejected;      // (bit 8 is a render status: it never stops the physics)
    const int nct = dead ? 0 : min(ccount_in, MAXC);
    cw0 = l < nct ? cw0 : 0.0f; cw1 = 16 + l < nct ? cw1 : 0.0f; cw2 = 32 + l < nct ? cw2 : 0.0f;
    // ---- and only now the stores of the command part
    if (!frozen && l == 0) D.errflags[env] = rejected ? ((ef0 & ~2u) | 2u) : (ef0 & ~2u);
    // an env whose command was rejected does not step; the list the look-ahead made for this step is dropped with it, so that
    // the normal forces of the last solved step (cforce) are never matched against a list they do not belong to
    if (!frozen && rejected && l == 0) D.ccount[env] = 0;
    if (l == 0 && mine && env_raw < N) { D.ccount_pub[env] = (!frozen && rejected) ? 0 : ccount_in; D.class_pub[env] = cls_in; }
    if (!dead) {
        if (l < NB) STT(ST_TGT + l) = tgt_l;
        if (lo_ >= 0 && lo_ < P.nobj && object_out_of_bounds(raw_x, raw_z, B.table_z)) {       // env.py:257-264
            const int i = lo_;
            for (int k = 0; k < 3; k++) { STT(ST_OPOS + 3 * i + k) = D.obj_home[(size_t)(7 * i + k) * N + env]; STT(ST_OVEL + 3 * i + k) = 0; STT(ST_OANG + 3 * i + k) = 0; }
#pragma unroll
            for (int k = 0; k < 4; k++) { oquat[k] = D.obj_home[(size_t)(7 * i + 3 + k) * N + env]; STT(ST_OQUAT + 4 * i + k) = oquat[k]; }
        }
    }
    // M^-1 goes to LDS (row builders, limit rows)
#pragma unroll
    for (int i = 0; i < 8; i++) if (l + 16 * i < NB * NB) LD(L_MINV + l + 16 * i) = minv_stage[i];
    // the lane's actuator waits in the three words of its motor row (three registers less over the row build; a coop env's four
    // groups hold the same values and store them in the same instruction)
    if (l < NB) { LD(L_MOT + 3 * l) = act_kp; LD(L_MOT + 3 * l + 1) = act_kd; LD(L_MOT + 3 * l + 2) = act_imp; }
    float wsA = 0.0f, wsB = 0.0f;     // slot-layout velocity change of the warm-start impulses of the generic normal rows
    // lanes 11..13 publish "their" object's data in LDS: the row builder reads the data of a contact's objects from there
    // (20 floats per object: position, 1/mass, I^-1, v*, w*)
    if (lo_ >= 0) {
        float4 *od = (float4 *)&LD(L_OBJ + 20 * lo_);
        od[0] = make_float4(myobj.op.x, myobj.op.y, myobj.op.z, myobj.imass);
        od[1] = make_float4(myobj.Iinv.m[0], myobj.Iinv.m[1], myobj.Iinv.m[2], myobj.Iinv.m[3]);
        od[2] = make_float4(myobj.Iinv.m[4], myobj.Iinv.m[5], myobj.Iinv.m[6], myobj.Iinv.m[7]);
        od[3] = make_float4(myobj.Iinv.m[8], myobj.vs.x, myobj.vs.y, myobj.vs.z);
        od[4] = make_float4(myobj.ws.x, myobj.ws.y, myobj.ws.z, 0.0f);
    }
    // row l of Minv in registers (motor rows, and M^-1 J^T of the generic rows)
    float minv_l[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) minv_l[j] = l < NB ? LD(L_MINV + lj * NB + j) : 0.0f;
    // the unconstrained velocities in the slot layout (relative velocity of a generic row = sum over lanes of J . u)
    const SlotOwner so = slot_owner(l);
    float ua = l < NB ? qds_l : 0.0f, ub = 0.0f;
    {
#define U_FROM(O)                                                                                                  \
        {                                                                                                          \
            const v3 vs_ = mk(row_bcast<NB + (O)>(myobj.vs.x), row_bcast<NB + (O)>(myobj.vs.y), row_bcast<NB + (O)>(myobj.vs.z));     \
            const v3 ws_ = mk(row_bcast<NB + (O)>(myobj.ws.x), row_bcast<NB + (O)>(myobj.ws.y), row_bcast<NB + (O)>(myobj.ws.z));     \
            ua = so.objA == (O) ? dot(vs_, so.elA) + dot(ws_, so.eaA) : ua;                                        \
            ub = so.objB == (O) ? dot(vs_, so.elB) + dot(ws_, so.eaB) : ub;                                        \
        }
        U_FROM(0) U_FROM(1) U_FROM(2)
#undef U_FROM
    }
    SPROF(0);
    // ---- walk the contact list in order, build rows (all lanes of the group run the control flow redundantly): 16 records at
    // a time go through the LDS staging area, from where every lane reads the record of the contact at hand
    int n_os = 0;                     // object-vs-static contacts swept by the object lanes (slots 0 .. n_os-1 of the LDS staging area)
    unsigned own_os = 0;              // this lane's share of them (bit = slot)
    unsigned fcnt = 0;                // ... per object, 4 bits each
    unsigned gobj = 0;                // objects touched by generic contacts of this env (bit o)
    int nc = 0, ng = 0;               // contacts; generic contacts
    bool class_mismatch = false;      // GEN = false only: a contact that needs generic rows
    const int nct_max = max(max(__builtin_amdgcn_readlane(nct, 0), __builtin_amdgcn_readlane(nct, 16)),
                            max(__builtin_amdgcn_readlane(nct, 32), __builtin_amdgcn_readlane(nct, 48)));
    if (!GEN) {
        // ---- light form: every contact is an object-vs-static one on the object lanes (<= 12 of them), so there is no slot
        // to hand out in list order -- contact c is slot c -- and LANE c builds all six rows of contact c: one trip instead of
        // one per contact (each a chain of LDS round trips at one wave per SIMD).  Same expressions as the walk below
        // (os_row_pair), same bits.
        {
            float4 *st = (float4 *)&LD(L_CST);
            st[l] = cr0; st[16 + l] = cr1; st[32 + l] = cr2;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const bool have = l < nct;
        const int ci = l;
        const float4 ra = *(const float4 *)&LD(L_CST + 12 * ci), rb_ = *(const float4 *)&LD(L_CST + 12 * ci + 4), rc = *(const float4 *)&LD(L_CST + 12 * ci + 8);
        const v3 x = mk(ra.x, ra.y, ra.z), n = mk(ra.w, rb_.x, rb_.y);
        const float dist = rb_.z;
        const int cm = __float_as_int(rb_.w);
        const int bodyA = (signed char)(cm & 255), bodyB = (signed char)((cm >> 8) & 255), linkA = (signed char)((cm >> 16) & 255);
        const float mu = rc.x, rest = rc.y, roll = rc.z, spin = rc.w;
        const bool ospair = bodyA >= 16 && bodyB < 0;
        const int obA = bodyA >= 16 ? min(bodyA - 16, NOBJ - 1) : 0;
        ObjData oA;
        {
            const float4 *od = (const float4 *)&LD(L_OBJ + 20 * obA);
            const float4 d0 = od[0], d1 = od[1], d2 = od[2], d3 = od[3], d4 = od[4];
            oA.op = mk(d0.x, d0.y, d0.z); oA.imass = d0.w;
            oA.Iinv.m[0] = d1.x; oA.Iinv.m[1] = d1.y; oA.Iinv.m[2] = d1.z; oA.Iinv.m[3] = d1.w;
            oA.Iinv.m[4] = d2.x; oA.Iinv.m[5] = d2.y; oA.Iinv.m[6] = d2.z; oA.Iinv.m[7] = d2.w;
            oA.Iinv.m[8] = d3.x; oA.vs = mk(d3.y, d3.z, d3.w); oA.ws = mk(d4.x, d4.y, d4.z);
        }
        // which contacts belong to which object: the masks the object lanes own, and this contact's place among its object's
        const int gsh = 16 * (grp & 3);
        const unsigned m0 = (unsigned)(__ballot(have && ospair && obA == 0) >> gsh) & 0xffffu, m1 = (unsigned)(__ballot(have && ospair && obA == 1) >> gsh) & 0xffffu,
                       m2 = (unsigned)(__ballot(have && ospair && obA == 2) >> gsh) & 0xffffu;
        const unsigned mine_m = obA == 0 ? m0 : (obA == 1 ? m1 : m2);
        const int before = __popc(mine_m & ((1u << l) - 1u));
        // (the row builder's rule: an object-vs-static pair, among the first KOS of its object and the first P.os_cap in all)
        class_mismatch = have && !(ospair && before < KOS && l < P.os_cap);
        own_os = lo_ == 0 ? m0 : (lo_ == 1 ? m1 : (lo_ == 2 ? m2 : 0u));
        n_os = nct; nc = nct;
        if (have) {
            const int meta = (bodyA & 255) | ((bodyB & 255) << 8) | ((linkA & 255) << 16) | (1 << 24) | (ci << 25) |
                             (fabsf(dist) < 0.1f ? (int)0x80000000u : 0);        // robot.py:136 contact_threshold
            *(int *)&LD(L_META + ci) = meta;
            LD(L_MU + ci) = mu; LD(L_SPIN + ci) = spin; LD(L_ROLL + ci) = roll;
            v3 t1, t2;
            plane_space(n, t1, t2);
            const float lam0 = cw0;           // (this lane holds the warm-start impulse of contact l)
#pragma unroll
            for (int k = 0; k < 3; k++)
                os_row_pair(k, k == 0 ? n : (k == 1 ? t1 : t2), x, oA, dist, rest, spin, roll, lam0, dt, P.erp, P.rest_thresh,
                            L_OSL + (3 * ci + k) * 12, L_OST + (3 * ci + k) * 8);
        }
        if (!GEN) {
            // what the object wave needs besides the rows and the objects' data (L_OBJ): who steps, whose contacts, orientations
            if (l == 0) {
                *(int *)&LD(L_GSC + OW_FLAGS) = ((mine && env_raw < N) ? 1 : 0) | (dead ? 2 : 0);
                *(unsigned *)&LD(L_GSC + OW_MASK) = m0; *(unsigned *)&LD(L_GSC + OW_MASK + 1) = m1; *(unsigned *)&LD(L_GSC + OW_MASK + 2) = m2;
            }
            if (lo_ >= 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) LD(L_GSC + OW_QUAT + 4 * lo_ + k) = oquat[k];
            }
            own_os = 0;
            __syncthreads();
        } else {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        }
    } else
#pragma unroll 1        // one copy of the (large) row-building body: the kernel must stay inside the instruction cache
    for (int bt = 0; 16 * bt < nct_max; bt++) {
        {   // batch bt = records 16 bt .. 16 bt + 15 = float4 48 bt .. 48 bt + 47 of the list = cr(3 bt) .. cr(3 bt + 2) of the lanes
            float4 *st = (float4 *)&LD(L_CST);
#define STAGE_REC(I, A_, B_, C_)                                                                                        \
            st[16 * (I) + l] = make_float4(bt == 0 ? A_.x : (bt == 1 ? B_.x : C_.x), bt == 0 ? A_.y : (bt == 1 ? B_.y : C_.y), \
                                           bt == 0 ? A_.z : (bt == 1 ? B_.z : C_.z), bt == 0 ? A_.w : (bt == 1 ? B_.w : C_.w));
            STAGE_REC(0, cr0, cr3, cr6) STAGE_REC(1, cr1, cr4, cr7) STAGE_REC(2, cr2, cr5, cr8)
#undef STAGE_REC
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // (coop: group cg takes contact ci0 + cg of every quadruple; otherwise one contact per trip)
        for (int ci0 = 0; ci0 < 16 && 16 * bt + ci0 < nct; ci0 += coop ? 4 : 1) {
            const int ci = min(ci0 + cg, 15);
            const bool have = 16 * bt + ci0 + cg < nct;             // (coop: the last quadruple may be short -- the group runs along, stores nothing)
            const float4 ra = *(const float4 *)&LD(L_CST + 12 * ci), rb_ = *(const float4 *)&LD(L_CST + 12 * ci + 4), rc = *(const float4 *)&LD(L_CST + 12 * ci + 8);
            const v3 x = mk(ra.x, ra.y, ra.z), n = mk(ra.w, rb_.x, rb_.y);
            const float dist = rb_.z;
            const int cm = __float_as_int(rb_.w);
            const int bodyA = (signed char)(cm & 255), bodyB = (signed char)((cm >> 8) & 255), linkA = (signed char)((cm >> 16) & 255);
            const float mu = rc.x, rest = rc.y, roll = rc.z, spin = rc.w;
            // warm start: this contact's initial normal impulse is held by lane ci of the group
            const float lam0 = lane_gather(bt == 0 ? cw0 : (bt == 1 ? cw1 : cw2), (threadIdx.x & 48) + ci);
            const bool ospair = bodyA >= 16 && bodyB < 0;
            ObjData oA, oB;
#pragma unroll
            for (int side = 0; side < 2; side++) {
                ObjData &o = side == 0 ? oA : oB;
                const int body = side == 0 ? bodyA : bodyB;
                const float4 *od = (const float4 *)&LD(L_OBJ + 20 * (body >= 16 ? body - 16 : 0));
                const float4 d0 = od[0], d1 = od[1], d2 = od[2], d3 = od[3], d4 = od[4];
                o.op = mk(d0.x, d0.y, d0.z); o.imass = d0.w;
                o.Iinv.m[0] = d1.x; o.Iinv.m[1] = d1.y; o.Iinv.m[2] = d1.z; o.Iinv.m[3] = d1.w;
                o.Iinv.m[4] = d2.x; o.Iinv.m[5] = d2.y; o.Iinv.m[6] = d2.z; o.Iinv.m[7] = d2.w;
                o.Iinv.m[8] = d3.x; o.vs = mk(d3.y, d3.z, d3.w); o.ws = mk(d4.x, d4.y, d4.z);
            }
            // the first KOS object-vs-static contacts of an object are swept by the object's lane, any further ones take the
            // generic path (rows of different objects commute, and an object's own rows keep their order: its pairs with
            // the statics precede every other pair).  The slots are handed out in list order: with four builders each group
            // replays the decisions of the quadruple's contacts (codes exchanged with v_readlane) and keeps the one of its own.
            const int obA = bodyA >= 16 ? bodyA - 16 : 0;
            const int code = have ? (1 | (ospair ? 2 : 0) | (obA << 2)) : 0;
            bool fast = false;
            int slot = 0, mync = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j > 0 && !coop) break;
                const int cj = coop ? __builtin_amdgcn_readlane(code, 16 * j) : code;
                if (!(cj & 1)) continue;
                const int ob_j = (cj >> 2) & 3;
                const bool fast_j = (cj & 2) && ((fcnt >> (4 * ob_j)) & 15u) < KOS && n_os < P.os_cap;
                const int slot_j = fast_j ? n_os : ng;
                if (j == cg) { fast = fast_j; slot = slot_j; mync = nc; }
                if (fast_j) {
                    n_os++;
                    fcnt += 1u << (4 * ob_j);
                    if (lo_ >= 0 && ob_j == lo_) own_os |= 1u << slot_j;
                } else if (GEN) ng++;
                else class_mismatch = true;       // (cannot happen: k_collide counts generic contacts by this very rule)
                nc++;
            }
            const int meta = (bodyA & 255) | ((bodyB & 255) << 8) | ((linkA & 255) << 16) | ((fast ? 1 : 0) << 24) | (slot << 25) |
                             (fabsf(dist) < 0.1f ? (int)0x80000000u : 0);        // robot.py:136 contact_threshold
            if (l == 0 && have) {
                *(int *)&LD(L_META + mync) = meta;
                if (fast) { LD(L_MU + slot) = mu; LD(L_SPIN + slot) = spin; LD(L_ROLL + slot) = roll; }      // (generic rows carry their coefficient)
            }
            v3 t1, t2;
            plane_space(n, t1, t2);
            if (fast) {
                // the three linear rows (n, t1, t2) and the three torsional rows about the same axes are built by lanes 0, 1, 2
                if (l < 3 && have)
                    os_row_pair(l, l == 0 ? n : (l == 1 ? t1 : t2), x, oA, dist, rest, spin, roll, lam0, dt, P.erp, P.rest_thresh,
                                L_OSL + (3 * slot + l) * 12, L_OST + (3 * slot + l) * 8);
                continue;
            }
            if (!GEN || !have) continue;
            // generic contact j = slot: six rows in the slot layout
            const int r0 = 6 * slot;
            if (bodyA >= 16) gobj |= 1u << (bodyA - 16);
            if (bodyB >= 16) gobj |= 1u << (bodyB - 16);
            GrowCtx gc;
            {
                const int rb = bodyA >= 0 && bodyA < 16 ? bodyA : (bodyB >= 0 && bodyB < 16 ? bodyB : -1);
                const float sgr = rb < 0 ? 0.0f : (rb == bodyA ? 1.0f : -1.0f);
                const float jm = (l < NB && rb >= 0 && ((ANC[rb >= 0 ? rb : 0] >> l) & 1u)) ? sgr : 0.0f;     // joint lanes: sign x ancestor mask
                v3 gA, hA, gtA, htA;
                grow_slot(so.objA, so.elA, so.eaA, bodyA, bodyB, x, oA, oB, gA, hA, gtA, htA);
                grow_slot(so.objB, so.elB, so.eaB, bodyA, bodyB, x, oA, oB, gc.gB, gc.hB, gc.gtB, gc.htB);
                const v3 cj = cross(ak_l, x - pk_l) * jm, aj = ak_l * jm;
                gc.gA = l < NB ? cj : gA; gc.gtA = l < NB ? aj : gtA; gc.hA = hA; gc.htA = htA;
            }
            // the three linear rows (n, t1, t2), then the three torsional rows about the same axes: the rows of a triple are
            // independent, so their chains (the 11-step M^-1 product, the group sums) are evaluated side by side
#pragma unroll 1
            for (int tq = 0; tq < 2; tq++) {
                const bool tors = tq == 1;
                // torsional rows without a coefficient (robot link against table / shelf: most contacts of a crushed arm) are
                // never swept: only their (zero) scalars are read, when the sweep lists are built
                if (tors && __ballot(spin > 0 || roll > 0) == 0ull) {
                    if (l == 0) {
                        *(float4 *)&LD(L_GSC + 4 * (r0 + 3)) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        *(float4 *)&LD(L_GSC + 4 * (r0 + 4)) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        *(float4 *)&LD(L_GSC + 4 * (r0 + 5)) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
                    continue;
                }
                const v3 gA_ = tors ? gc.gtA : gc.gA, gB_ = tors ? gc.gtB : gc.gB, hA_ = tors ? gc.htA : gc.hA, hB_ = tors ? gc.htB : gc.hB;
                float ja3[3], jb3[3], mja3[3], mjb3[3];
#pragma unroll
                for (int ka = 0; ka < 3; ka++) {
                    const v3 d = ka == 0 ? n : (ka == 1 ? t1 : t2);
                    ja3[ka] = dot(d, gA_); jb3[ka] = dot(d, gB_); mjb3[ka] = dot(d, hB_);
                    mja3[ka] = 0.0f;
                }
#define MJA_STEP(J) { mja3[0] += minv_l[J] * row_bcast<J>(ja3[0]); mja3[1] += minv_l[J] * row_bcast<J>(ja3[1]); mja3[2] += minv_l[J] * row_bcast<J>(ja3[2]); }
                MJA_STEP(0) MJA_STEP(1) MJA_STEP(2) MJA_STEP(3) MJA_STEP(4) MJA_STEP(5) MJA_STEP(6) MJA_STEP(7) MJA_STEP(8) MJA_STEP(9) MJA_STEP(10)
#undef MJA_STEP
                float mjf3[3], dinv3[3];          // M^-1 J^T of this lane's slot-A variable; 1 / diagonal (0: row absent)
#pragma unroll
                for (int ka = 0; ka < 3; ka++) {
                    const int kr = 3 * tq + ka;
                    const v3 d = ka == 0 ? n : (ka == 1 ? t1 : t2);
                    const bool present = !tors || (ka == 0 ? spin > 0 : roll > 0);
                    const float ja = ja3[ka], jb = jb3[ka], mjb = mjb3[ka];
                    const float mja = l < NB ? mja3[ka] : dot(d, hA_);
                    mjf3[ka] = mja;
                    const float diag = group_sum(ja * mja + jb * mjb);
                    const float rel = group_sum(ja * ua + jb * ub);
                    // (the normal row in the canonical layout: the block repack below and the coop warm start read it back)
                    if (kr == 0) D.grows[((size_t)env * GP_RECS + GP_C + slot) * 16 + l] = make_float4(ja, mja, jb, mjb);
                    if (kr == 0 && !coop) { wsA = fmaf(mja, lam0, wsA); wsB = fmaf(mjb, lam0, wsB); }      // (coop: replayed in list order below)
                    float rhsn;
                    if (kr == 0) {
                        float r = 0;
                        if (fabsf(rel) >= P.rest_thresh) { r = rest * -rel; if (r < 0) r = 0; }
                        float verr = r - rel, perr = 0;
                        if (dist > 0) verr -= dist * inv_dt;
                        else perr = -dist * P.erp * inv_dt;
                        rhsn = perr + verr;
                    } else rhsn = -rel;
                    const float dinv = (present && diag > 0) ? 1.0f / diag : 0.0f;
                    dinv3[ka] = dinv;
                    if (l == 0)
                        *(float4 *)&LD(L_GSC + 4 * (r0 + kr)) = make_float4(rhsn * dinv, dinv, kr == 0 ? 0.0f : (kr < 3 ? mu : (kr == 3 ? spin : roll)), kr == 0 ? lam0 : 0.0f);
                }
                // ---- the rows as the sweeps stream them (block Gauss-Seidel, see the sweep): lane (h, g) = (bit 3, bit 2) of the group
                const bool hh_ = (l & 8) != 0, gg_ = (l & 4) != 0;
                if (!tors) {
                    // lateral friction pair (t1, t2): J pair in the lane's order (its own row first), M^-1 J^T pair, cross term of row t2
                    const float c21 = group_sum(ja3[2] * mjf3[1] + jb3[2] * mjb3[1]);
                    float4 *fp = D.grows + ((size_t)env * GP_RECS + GP_F + 3 * slot) * 16 + l;
                    fp[0] = make_float4(hh_ ? ja3[2] : ja3[1], hh_ ? ja3[1] : ja3[2], hh_ ? jb3[2] : jb3[1], hh_ ? jb3[1] : jb3[2]);
                    fp[16] = make_float4(mjf3[1], mjb3[1], mjf3[2], mjb3[2]);
                    fp[32] = make_float4(hh_ ? -(dinv3[2] * c21) : 0.0f, 0.0f, 0.0f, 0.0f);
                } else {
                    // torsional triple (spinning about n, rolling about t1, t2) + an absent fourth row; absent rows are all zero
                    const bool ps = spin > 0, pr = roll > 0;
                    const float a0 = ps ? ja3[0] : 0.0f, b0 = ps ? jb3[0] : 0.0f, ma0 = ps ? mjf3[0] : 0.0f, mb0 = ps ? mjb3[0] : 0.0f;
                    const float a1 = pr ? ja3[1] : 0.0f, b1 = pr ? jb3[1] : 0.0f, ma1 = pr ? mjf3[1] : 0.0f, mb1 = pr ? mjb3[1] : 0.0f;
                    const float a2 = pr ? ja3[2] : 0.0f, b2 = pr ? jb3[2] : 0.0f, ma2 = pr ? mjf3[2] : 0.0f, mb2 = pr ? mjb3[2] : 0.0f;
                    const float c10 = group_sum(a1 * ma0 + b1 * mb0), c20 = group_sum(a2 * ma0 + b2 * mb0), c21 = group_sum(a2 * ma1 + b2 * mb1);
                    const float4 pa = make_float4(hh_ ? a1 : a0, hh_ ? a0 : a1, hh_ ? b1 : b0, hh_ ? b0 : b1);      // pair (row 0, row 1)
                    const float4 pb = make_float4(hh_ ? 0.0f : a2, hh_ ? a2 : 0.0f, hh_ ? 0.0f : b2, hh_ ? b2 : 0.0f);  // pair (row 2, -)
                    float4 *tp = D.grows + ((size_t)env * GP_RECS + GP_T + 5 * slot) * 16 + l;
                    tp[0] = make_float4(gg_ ? pb.x : pa.x, gg_ ? pb.y : pa.y, gg_ ? pb.z : pa.z, gg_ ? pb.w : pa.w);     // (component selects: a
                    tp[16] = make_float4(gg_ ? pa.x : pb.x, gg_ ? pa.y : pb.y, gg_ ? pa.z : pb.z, gg_ ? pa.w : pb.w);    //  select of structs goes through scratch)
                    tp[32] = make_float4(ma0, mb0, ma1, mb1);
                    tp[48] = make_float4(ma2, mb2, 0.0f, 0.0f);
                    // (the lane's row: 2 g + h -- cross terms with the rows in front of it, times -1/diag)
                    const float x0 = gg_ ? (hh_ ? 0.0f : -(dinv3[2] * c20)) : (hh_ ? -(dinv3[1] * c10) : 0.0f);
                    const float x1 = (gg_ && !hh_) ? -(dinv3[2] * c21) : 0.0f;
                    tp[64] = make_float4(x0, x1, 0.0f, 0.0f);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");        // the staging area is rewritten by the next batch
        __builtin_amdgcn_wave_barrier();
    }
    if (!GEN) {
        const unsigned mm = (unsigned)(__ballot(class_mismatch) >> (16 * (grp & 3))) & 0xffffu;
        if (mm != 0u && l == 0 && !dead) atomicOr(&D.errflags[env], 4u);      // (internal consistency: never seen)
    }
    if (GEN) {
        // ---- block repack of the generic NORMAL rows: contacts 4 b .. 4 b + 3 as one block {J pair, J pair, M^-1 J^T pair, M^-1 J^T
        // pair, cross terms} in the lanes' order (see the sweep), from the canonical rows the builders have just stored.  coop:
        // group cg takes the blocks cg, cg + 4, ..  Also: the scalars of the dummy contacts and of the last block's absent rows.
        const int ngw = max(max(__builtin_amdgcn_readlane(ng, 0), __builtin_amdgcn_readlane(ng, 16)),
                            max(__builtin_amdgcn_readlane(ng, 32), __builtin_amdgcn_readlane(ng, 48)));
        if (ngw > 0) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            {
                float4 *zp = (float4 *)&LD(fix + LF_ZPAD);
                zp[l] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (l < 8) zp[16 + l] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            const bool hh_ = (l & 8) != 0, gg_ = (l & 4) != 0;
            const int nbw = (ngw + 3) >> 2;
#pragma unroll 1
            for (int b = cg; b < nbw; b += coop ? 4 : 1) {
                const int c0 = 4 * b;
                const float4 *cp = D.grows + ((size_t)env * GP_RECS + GP_C) * 16 + l;
                // (unconditional loads from always-valid addresses, values selected: DESIGN.md 7)
                const float4 r0_ = sel4(c0 < ng, cp[16 * (c0 < ng ? c0 : 0)]), r1_ = sel4(c0 + 1 < ng, cp[16 * (c0 + 1 < ng ? c0 + 1 : 0)]),
                             r2_ = sel4(c0 + 2 < ng, cp[16 * (c0 + 2 < ng ? c0 + 2 : 0)]), r3_ = sel4(c0 + 3 < ng, cp[16 * (c0 + 3 < ng ? c0 + 3 : 0)]);
                const float d1 = c0 + 1 < ng ? LD(L_GSC + 24 * (c0 + 1 < ng ? c0 + 1 : 0) + 1) : 0.0f, d2 = c0 + 2 < ng ? LD(L_GSC + 24 * (c0 + 2 < ng ? c0 + 2 : 0) + 1) : 0.0f,
                            d3 = c0 + 3 < ng ? LD(L_GSC + 24 * (c0 + 3 < ng ? c0 + 3 : 0) + 1) : 0.0f;
                // cross terms J_k . M^-1 J_i^T (i < k): what row i's impulse change adds to row k's J . v
                const float c10 = group_sum(r1_.x * r0_.y + r1_.z * r0_.w);
                const float c20 = group_sum(r2_.x * r0_.y + r2_.z * r0_.w), c21 = group_sum(r2_.x * r1_.y + r2_.z * r1_.w);
                const float c30 = group_sum(r3_.x * r0_.y + r3_.z * r0_.w), c31 = group_sum(r3_.x * r1_.y + r3_.z * r1_.w), c32 = group_sum(r3_.x * r2_.y + r3_.z * r2_.w);
                const float4 pa = make_float4(hh_ ? r1_.x : r0_.x, hh_ ? r0_.x : r1_.x, hh_ ? r1_.z : r0_.z, hh_ ? r0_.z : r1_.z);
                const float4 pb = make_float4(hh_ ? r3_.x : r2_.x, hh_ ? r2_.x : r3_.x, hh_ ? r3_.z : r2_.z, hh_ ? r2_.z : r3_.z);
                const float dk = gg_ ? (hh_ ? d3 : d2) : d1;          // (the lane's row 2 g + h; row 0 has no cross term)
                const float x0 = gg_ ? (hh_ ? c30 : c20) : (hh_ ? c10 : 0.0f), x1 = gg_ ? (hh_ ? c31 : c21) : 0.0f, x2 = (gg_ && hh_) ? c32 : 0.0f;
                if (c0 < ng) {
                    float4 *np = D.grows + ((size_t)env * GP_RECS + GP_N + 5 * b) * 16 + l;
                    np[0] = make_float4(gg_ ? pb.x : pa.x, gg_ ? pb.y : pa.y, gg_ ? pb.z : pa.z, gg_ ? pb.w : pa.w);
                    np[16] = make_float4(gg_ ? pa.x : pb.x, gg_ ? pa.y : pb.y, gg_ ? pa.z : pb.z, gg_ ? pa.w : pb.w);
                    np[32] = make_float4(r0_.y, r0_.w, r1_.y, r1_.w);
                    np[48] = make_float4(r2_.y, r2_.w, r3_.y, r3_.w);
                    np[64] = make_float4(-(dk * x0), -(dk * x1), -(dk * x2), 0.0f);
                    if (l >= 1 && l <= 3 && c0 + l >= ng) *(float4 *)&LD(L_GSC + 24 * (c0 + l)) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                } else if (!coop) {
                    // (four envs to a wave: this env has fewer blocks than another one of its wave -- it sweeps all-zero blocks meanwhile)
                    float4 *np = D.grows + ((size_t)env * GP_RECS + GP_N + 5 * b) * 16 + l;
                    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    np[0] = z4; np[16] = z4; np[32] = z4; np[48] = z4; np[64] = z4;
                    if (l < 4) *(float4 *)&LD(L_GSC + 24 * (c0 + l)) = z4;
                }
            }
        }
    }
    if (coop) {
        // the warm-start velocity change of the generic normal rows, in list order, from the stored rows: the very fma sequence
        // a single builder runs in line (each of the four builders holds only its own contacts' share)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        for (int j = 0; j < ng; j++) {
            const float4 rw = D.grows[((size_t)env * GP_RECS + GP_C + j) * 16 + l];
            const float l0 = LD(L_GSC + 24 * j + 3);
            wsA = fmaf(rw.y, l0, wsA); wsB = fmaf(rw.w, l0, wsB);
        }
        // groups 1..3 have done their part: from here on they run along without rows of their own and store nothing
        if (cg != 0) { ng = 0; own_os = 0; n_os = 0; wsA = 0.0f; wsB = 0.0f; dead = true; }
    }
    SPROF(1);
    // ---- motor + limit rows: lane j < 11 builds the rows of joint j
    if (l < NB) {
        float dinv = 1.0f / LD(L_MINV + l * NB + l);
        const float kp_l = LD(L_MOT + 3 * l), kd_l = LD(L_MOT + 3 * l + 1);      // (the lane's own words; + 2, the impulse bound, stays for the sweeps)
        float vt = kp_l * (tgt_l - q_l) / dt + qds_l + kd_l * (0.0f - qds_l);
        LD(L_MOT + 3 * l) = (vt - qds_l) * dinv;
        LD(L_MOT + 3 * l + 1) = dinv;
        float lo = B.limits[l][0], hi = B.limits[l][1];
#pragma unroll
        for (int side = 0; side < 2; side++) {
            float dist = side == 0 ? q_l - lo : hi - q_l;
            bool on = (lo < hi) && (dist < 0.5f);
            float sg = side == 0 ? 1.0f : -1.0f;
            float rel = sg * qds_l;
            float verr = -rel, perr = 0;
            if (dist > 0) verr -= dist / dt;
            else perr = -dist * P.erp / dt;
            LD(L_LIM + 2 * (2 * l + side)) = on ? (perr + verr) * dinv : -1e30f;   // -1e30: row absent
            LD(L_LIM + 2 * (2 * l + side) + 1) = 0.0f;
        }
    }
    SPROF(2);
    // compact list of the limit rows that exist (usually the two finger lower limits), in row order
    unsigned limmask = 0;
#pragma unroll
    for (int js = 0; js < 2 * NB; js++) if (LD(L_LIM + 2 * js) > -1e29f) limmask |= 1u << js;    // 22 independent LDS reads
    if (coop && cg != 0) limmask = 0;            // (the limit rows live in the LDS region group 0 sweeps)
    // ---- PGS.  Lane state: dq (slot A: lanes 0..10 joints, lanes 11..15 object 2 during generic sweeps), vb (slot B), and
    // (dv, dw) of object lane-11 on lanes 11..13
    float dq = wsA, vb = wsB;          // (warm start: the inherited impulses of the generic normal rows are already applied)
    v2f V01 = P2(0.0f, 0.0f), V23 = P2(0.0f, 0.0f), V45 = P2(0.0f, 0.0f);      // (dv.xy) (dv.z dw.x) (dw.yz), REG_ROW_STEP
    // (1 / mass of the lane's object as its L_OBJ record holds it -- the word the light object wave reads too; an LDS read
    // instead of a register held from the stage-in.  Lanes of objects the handle does not simulate have no rows to step.)
    const float inv_mass = lo_ >= 0 ? LD(L_OBJ + 20 * (lo_ >= 0 ? lo_ : 0) + 3) : 0.0f;
    const float m_rhs = l < NB ? LD(L_MOT + 3 * lj) : 0.0f, m_dinv = l < NB ? LD(L_MOT + 3 * lj + 1) : 0.0f;
    const float max_imp = l < NB ? LD(L_MOT + 3 * lj + 2) : 0.0f;       // (per lane: the clamp of the lane's own motor row, the only one whose step is kept)
    float m_lam = 0.0f, m_c = m_rhs, m_keep = 0.0f;      // m_c = lambda + rhs of this lane's motor row (brought up to date once per sweep, SWEEP_MOTORS)
#define LDB4(r, off) (*(const float4 *)&LD(L_OSL + (r) * 12 + (off)))
#define LDT4(r, off) (*(const float4 *)&LD(L_OST + (r) * 8 + (off)))
#define LDZ4(has, r, off) sel4((has), LDB4((r), (off)))
    int lim_j[KLIM]; float lim_sg[KLIM], lim_rhs[KLIM], lim_dinv[KLIM], lim_col[KLIM], lim_lam[KLIM];
    {
        unsigned rem = limmask;
#pragma unroll
        for (int k = 0; k < KLIM; k++) {
            const bool has = rem != 0;
            const int js = has ? __ffs(rem) - 1 : 0;
            rem &= rem - 1;
            lim_j[k] = js >> 1; lim_sg[k] = (js & 1) == 0 ? 1.0f : -1.0f;
            lim_rhs[k] = has ? LD(L_LIM + 2 * js) : 0.0f; lim_dinv[k] = has ? LD(L_MOT + 3 * (js >> 1) + 1) : 0.0f;
            lim_col[k] = (has && l < NB) ? LD(L_MINV + lj * NB + (js >> 1)) : 0.0f;
            lim_lam[k] = 0.0f;
        }
        limmask = rem;                                   // rows left for the LDS loop
    }
    unsigned os_cs = 0;                                  // contact indices of the register rows, one byte each
    float os_mu[KOS], os_ln[KOS], os_l1[KOS], os_l2[KOS], os_l0[KOS];      // (os_l0: the inherited normal impulses)
    float4 os_n0[KOS], os_n1[KOS], os_n2[KOS], os_a0[KOS], os_a1[KOS], os_a2[KOS], os_b0[KOS], os_b1[KOS], os_b2[KOS];
    {
        unsigned rem = own_os;
#pragma unroll
        for (int i = 0; i < KOS; i++) {
            const bool has = rem != 0;
            const int c = has ? __ffs(rem) - 1 : 0;
            rem &= rem - 1;
            os_cs |= (has ? (unsigned)c : 255u) << (8 * i);
            os_mu[i] = has ? LD(L_MU + c) : 0.0f; os_ln[i] = 0.0f; os_l1[i] = 0.0f; os_l2[i] = 0.0f;
            os_l0[i] = has ? LD(L_OST + (3 * c) * 8 + 5) : 0.0f;
            os_n0[i] = LDZ4(has, 3 * c, 0); os_n1[i] = LDZ4(has, 3 * c, 4); os_n2[i] = LDZ4(has, 3 * c, 8);
            os_a0[i] = LDZ4(has, 3 * c + 1, 0); os_a1[i] = LDZ4(has, 3 * c + 1, 4); os_a2[i] = LDZ4(has, 3 * c + 1, 8);
            os_b0[i] = LDZ4(has, 3 * c + 2, 0); os_b1[i] = LDZ4(has, 3 * c + 2, 4); os_b2[i] = LDZ4(has, 3 * c + 2, 8);
        }
    }
    // torsional rows of the same contacts: rotation about the axis of linear row k (its dir), {m.x, rhs, m.y, m.z} (m = M^-1 J^T), 1/diag, lambda
    float4 ot_m[KOS][3]; float ot_d[KOS][3], ot_l[KOS][3], os_sp[KOS], os_ro[KOS];
#pragma unroll
    for (int i = 0; i < KOS; i++) {
        const int c = (os_cs >> (8 * i)) & 255;
        const bool has = c != 255;
        const int cc = has ? c : 0;
        os_sp[i] = has ? LD(L_SPIN + cc) : 0.0f; os_ro[i] = has ? LD(L_ROLL + cc) : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            ot_m[i][k] = sel4(has, LDT4(3 * cc + k, 0));
            ot_d[i][k] = has ? LD(L_OST + (3 * cc + k) * 8 + 4) : 0.0f;
            ot_l[i][k] = 0.0f;
        }
    }
    // motors: every lane evaluates the step of "its" row from its own dq; row J's impulse change is lane J's value,
    // broadcast to the 16 lanes of the env with one DPP row_newbcast (branch-free clamp, same values as if/else).
    // A lane's own lambda and lambda + rhs are read by ITS row only, once per sweep: the row's new impulse is set aside (one select
    // per step) and both are brought up to date behind the eleven steps -- six issue slots per row instead of nine, the same values
    // (what the other ten steps compute from a lane's stale pair is never used: only lane J's change is broadcast).
    // The inline asm's `s_nop 1` covers the VGPR-write -> DPP-read hazard (2 wait states) by hand; the 5-wait-state hazard behind a
    // VALU write of EXEC, which the compiler cannot see inside the asm, is excluded by a build gate: tools/check_dpp_hazard.py
    // (make check-no-scratch, run by __graft_entry__.build) fails the build if any kernel writes EXEC from the VALU at all.
#define MOTOR_STEP(J)                                                                     \
        {                                                                                 \
            const float s0_ = fmaf(-dq, m_dinv, m_c);          /* (lambda + rhs) - dinv * dq */ \
            const float sum_ = __builtin_amdgcn_fmed3f(s0_, -max_imp, max_imp);           \
            const float dl_ = sum_ - m_lam;                                               \
            m_keep = (l == (J)) ? sum_ : m_keep;                                          \
            asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "+v"(dq) : "v"(dl_), "v"(minv_l[J]));   /* dq += lane J's dl * minv[J]: broadcast and multiply-add in ONE instruction (the compiler does not fold row_newbcast; the two wait states a DPP read needs behind the VALU write of its source are in the string) */ \
        }
#define SWEEP_MOTORS                                                                                  \
        MOTOR_STEP(0) MOTOR_STEP(1) MOTOR_STEP(2) MOTOR_STEP(3) MOTOR_STEP(4) MOTOR_STEP(5)           \
        MOTOR_STEP(6) MOTOR_STEP(7) MOTOR_STEP(8) MOTOR_STEP(9) MOTOR_STEP(10)                        \
        m_lam = m_keep; m_c = m_keep + m_rhs;
#define LIMIT_STEP(k)   /* joint limit held in registers; absent rows are all-zero: dl = 0 */        \
        {                                                                                             \
            const float dqj_ = group_sum(l == lim_j[k] ? dq : 0.0f);                                  \
            const float s0_ = fmaf(-(lim_sg[k] * dqj_), lim_dinv[k], lim_lam[k] + lim_rhs[k]);         \
            const float sum_ = __builtin_amdgcn_fmed3f(s0_, 0.0f, 100.0f);                                       \
            const float dl_ = sum_ - lim_lam[k];                                                      \
            lim_lam[k] = sum_;                                                                        \
            dq += lim_col[k] * (lim_sg[k] * dl_);                                                     \
        }
#define OSN_STEP(i) REG_ROW_STEP(os_n0[i], os_n1[i], os_n2[i], os_ln[i], 0.0f, 1e10f);
#define OSF_STEP(i)                                                                                   \
        {                                                                                             \
            const float hi_ = os_mu[i] * os_ln[i];                                                    \
            REG_ROW_STEP(os_a0[i], os_a1[i], os_a2[i], os_l1[i], -hi_, hi_);                          \
            REG_ROW_STEP(os_b0[i], os_b1[i], os_b2[i], os_l2[i], -hi_, hi_);                          \
        }
#define REG_TORS_STEP(AX, i, k, HI)                                                                  \
        {                                                                                             \
            const float jv_ = fmaf((AX).x, DWX, fmaf((AX).y, DWY, (AX).z * DWZ));                     \
            const float s0_ = fmaf(-jv_, ot_d[i][k], ot_l[i][k] + ot_m[i][k].y);                      \
            const float sum_ = __builtin_amdgcn_fmed3f(s0_, -(HI), (HI));                             \
            const float dl_ = sum_ - ot_l[i][k];                                                      \
            ot_l[i][k] = sum_;                                                                        \
            DWX = fmaf(ot_m[i][k].x, dl_, DWX);                                                       \
            V45 = pk_fma(P2(ot_m[i][k].z, ot_m[i][k].w), P2(dl_, dl_), V45);                          \
        }
#define OST_STEP(i)                                                                                   \
        {                                                                                             \
            const float hs_ = os_sp[i] * os_ln[i], hr_ = os_ro[i] * os_ln[i];                         \
            REG_TORS_STEP(os_n0[i], i, 0, hs_) REG_TORS_STEP(os_a0[i], i, 1, hr_) REG_TORS_STEP(os_b0[i], i, 2, hr_) \
        }
    // joint limits beyond the register rows (GEN: all of them), existing rows only; the expressions of LIMIT_STEP
#define LIMIT_LOOP                                                                                    \
        _Pragma("unroll 1")                                                                           \
        for (unsigned rem = limmask; rem; rem &= rem - 1) {                                           \
            const int js = __ffs(rem) - 1;                                                            \
            const int j = js >> 1;                                                                    \
            const float lr = LD(L_LIM + 2 * js), ll = LD(L_LIM + 2 * js + 1), di = LD(L_MOT + 3 * j + 1); \
            const float col = l < NB ? LD(L_MINV + lj * NB + j) : 0.0f;                               \
            const float sg = (js & 1) == 0 ? 1.0f : -1.0f;                                            \
            const float dqj_ = group_sum(l == j ? dq : 0.0f);                                         \
            const float s0_ = fmaf(-(sg * dqj_), di, ll + lr);                                        \
            const float sum_ = __builtin_amdgcn_fmed3f(s0_, 0.0f, 100.0f);                                       \
            const float dl_ = sum_ - ll;                                                              \
            LD(L_LIM + 2 * js + 1) = sum_;                                                            \
            dq += col * (sg * dl_);                                                                   \
        }
    SPROF(3);
    SBLK_MARK(sb_t1)
    static_assert(KLIM == 2 && KOS == 4, "the sweeps below are written out for KLIM = 2, KOS = 4");
    // When no env of this wave has a row outside the registers (no generic contact, no further limit rows), an iteration is one straight-line block: the robot chain (motors, limits) and the object chain
    // (normals, frictions, torsional) are independent and the scheduler overlaps them.
    const bool simple = __ballot(!(ng == 0 && limmask == 0)) == 0ull;
    // generic sweeps: trip counts and the objects to move between the object lanes and the slots, over the whole wave
    const int ng_max = max(max(__builtin_amdgcn_readlane(ng, 0), __builtin_amdgcn_readlane(ng, 16)),
                           max(__builtin_amdgcn_readlane(ng, 32), __builtin_amdgcn_readlane(ng, 48)));
    const unsigned gobj_w = (unsigned)__builtin_amdgcn_readlane((int)gobj, 0) | (unsigned)__builtin_amdgcn_readlane((int)gobj, 16) |
                            (unsigned)__builtin_amdgcn_readlane((int)gobj, 32) | (unsigned)__builtin_amdgcn_readlane((int)gobj, 48);
    // the generic rows written to global memory by the builder are read back by this same wave: its stores must have
    // completed (workgroup scope: the CU's vector L1 is write-through and shared by the workgroup -- no cache maintenance;
    // an agent-scope fence would write back the XCD's L2)
    if (ng_max > 0) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // ---- generic rows: BLOCK Gauss-Seidel.  Rows are swept in blocks -- the normal rows of four consecutive contacts, the two
    // lateral rows of a contact, its (up to) three torsional rows -- whose J . v are formed SIDE BY SIDE from the velocities in
    // front of the block; row k's value then takes the impulse changes of the block's rows i < k through the cross terms
    // J_k . M^-1 J_i^T (stored with the block, times -1/diag_k).  Algebraically the very Gauss-Seidel sequence (same order, same
    // clamps); at one wave per SIMD a kernel lasts as long as its instruction count, and a block of four costs 29 VALU
    // instructions instead of 4 x 14 (two rows: 18 instead of 28):
    //   * lane (h, g) = (bit 3, bit 2) of the group ends up with the sum of row 2 g + h (two-row block: row h).  The J pairs are
    //     STORED in the order each lane needs ({own row, partner's row} x {slot A, slot B}, builder / repack above), so that the
    //     products are two packed multiply-adds per pair and the 16-lane sums of all four rows take five DPP adds: across the
    //     halves (row_ror 8: my second value is my partner's first), across the quads (row_half_mirror), inside the quad;
    //   * the clamp of row k is evaluated by the lanes of row k (their scalars rhs, 1/diag, bound, lambda come from LDS), its impulse
    //     change goes to all lanes with one DPP row_newbcast and updates the running sums s (one FMA) and the velocities
    //     (dq, vb) (one packed FMA with the row's (M^-1 J^T)_A, (M^-1 J^T)_B pair);
    //   * a lane's s stops changing once its own row is done (its later cross terms are zero): `sum` after the last step is the
    //     row's new lambda in every lane of the row.
    // The blocks are streamed from global memory (L2 / L1 resident: the wave wrote them) through ONE register set: every part of
    // the next block is requested as soon as the registers it lands in are free (BLK4_STEP), its scalars from LDS behind the
    // step.  Measured (profiles/r05_*): two sets (a block further ahead) were slower everywhere -- the 24 registers they take
    // push the object lanes' rows into AGPR traffic (+17 % on a sweep without generic rows) -- and three sets spilled.  A normal
    // block takes ~210 shader cycles (52 per row; the row-by-row step of round 4: 82), a lateral pair ~140.  Dummy blocks (contact
    // MAXC: all-zero records and scalars; all-zero normal blocks behind an env's own) are what a group sweeps while another env of
    // its wave has blocks left.  Byte offsets are 32 bits (rr_create checks N).
    const unsigned gp_l = (unsigned)env * (unsigned)GP_ENV_BYTES + ((unsigned)l << 4);
    // (LDS is addressed through 32-bit address-space-3 pointers made from byte addresses: the generic-pointer form costs an add per access)
    typedef float v4f_ __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const v4f_ lds_cf4;
    typedef __attribute__((address_space(3))) float lds_f;
    typedef __attribute__((address_space(3))) const unsigned char lds_cu8;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float *)g_slds;
#define LDS_F4(BYTE) (*(lds_cf4 *)(size_t)(unsigned)(BYTE))
#define LDS_F(BYTE) (*(lds_f *)(size_t)(unsigned)(BYTE))
    const bool hh = (l & 8) != 0, gg = (l & 4) != 0;
    const int rho = (gg ? 2 : 0) + (hh ? 1 : 0);
    const unsigned gsc_b = lds0 + 4u * (unsigned)L_GSC;             // byte address of the generic row scalars in LDS
    const int nb_g = (ng + 3) >> 2;                                 // normal blocks of this group's env
    const int nb_max = (ng_max + 3) >> 2;
    const unsigned list_b = lds0 + 4u * (unsigned)(fix + LF_LISTA); // byte address of listA (listT: + 64)
    // object lane (11 + O) -> slots, and back; comps 0..5 = dv.xyz, dw.xyz
    // (row_bcast_z: the broadcast reads the register where it is -- the tied form copies it first and then waits out the DPP hazard
    // behind its own copy: four issue slots per component instead of two, 108 components per sweep of an env with three pushed objects)
#define TO_SLOT(O, C, REG, SLOTREG, LANE) { const float t_ = row_bcast_z<NB + (O)>(REG); SLOTREG = (l == (LANE)) ? t_ : SLOTREG; }
#define FROM_SLOT(O, C, REG, SLOTREG, LANE) { const float t_ = row_bcast_z<LANE>(SLOTREG); REG = (l == NB + (O)) ? t_ : REG; }
#define OBJ_SLOTS(OP)                                                                                                  \
    if (gobj_w & 1u) { OP(0, 0, DVX, vb, 0) OP(0, 1, DVY, vb, 1) OP(0, 2, DVZ, vb, 2) OP(0, 3, DWX, vb, 3) OP(0, 4, DWY, vb, 4) OP(0, 5, DWZ, vb, 5) } \
    if (gobj_w & 2u) { OP(1, 0, DVX, vb, 6) OP(1, 1, DVY, vb, 7) OP(1, 2, DVZ, vb, 8) OP(1, 3, DWX, vb, 9) OP(1, 4, DWY, vb, 10) OP(1, 5, DWZ, vb, 11) } \
    if (gobj_w & 4u) { OP(2, 0, DVX, dq, 11) OP(2, 1, DVY, dq, 12) OP(2, 2, DVZ, dq, 13) OP(2, 3, DWX, dq, 14) OP(2, 4, DWY, dq, 15) OP(2, 5, DWZ, vb, 12) }
    // warm start: the object components of the generic rows' initial velocity change go from the slots to the object lanes,
    // then the register rows add theirs (b2.w of a normal row = its inherited impulse; absent rows are all-zero)
    if (ng_max > 0) { OBJ_SLOTS(FROM_SLOT) }
#pragma unroll
    for (int i = 0; i < (GEN ? KOS : 0); i++) {
        const float l0_ = os_l0[i], sm_ = l0_ * inv_mass;
        os_ln[i] = l0_;
        V01 = pk_fma(P2(os_n0[i].x, os_n0[i].y), P2(sm_, sm_), V01);
        V23 = pk_fma(P2(os_n1[i].z, os_n1[i].w), P2(sm_, l0_), V23);
        V45 = pk_fma(P2(os_n2[i].x, os_n2[i].y), P2(l0_, l0_), V45);
    }
    int nA = 0, nT = 0;                                   // entries of this env's lists of active contacts (lateral / torsional pass)
    if (ng_max > 0) {                                     // (both lists start as all dummies)
#pragma unroll
        for (int k = 0; k < 64; k += 16) { listA[k + l] = (unsigned char)MAXC; listT[k + l] = (unsigned char)MAXC; }
    }
    // lane l's generic contacts l, 16 + l, 32 + l: which of them have torsional rows (bit c), and which had a positive normal impulse
    // after the previous sweep's normal pass (the list rebuild below)
    unsigned tors_bits = 0u, act_prev = 0u;
    if (GEN && ng_max > 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int j = 16 * c + l;
            if (j < ng && ((LD(L_GSC + 24 * j + 14) > 0.0f) | (LD(L_GSC + 24 * j + 18) > 0.0f))) tors_bits |= 1u << c;
        }
    }
    // the register set of the block in flight: records {j0, j1, m0, m1, x}, scalars {rhs, 1/diag, lambda, upper bound}, the LDS
    // byte address of the scalars (lambda goes back there)
#define BLK_DECL(R) float4 R##j0 = make_float4(0, 0, 0, 0), R##j1 = R##j0, R##m0 = R##j0, R##m1 = R##j0; float R##x0 = 0.0f, R##x1 = 0.0f, R##x2 = 0.0f, R##rhs = 0.0f, R##di = 0.0f, R##lam = 0.0f, R##hi = 0.0f; int R##a = 0;
    BLK_DECL(A)
    // where block I of the pass lives: N pass: block I itself (a group whose env has fewer blocks than its wave sweeps the all-zero
    // blocks the repack left behind its own); F / T pass: the contact in entry I of the pass' list (dummy MAXC: all-zero records)
#define BLK_ENTRY(I) ((int)*(lds_cu8 *)(size_t)(lst_b + (unsigned)(I)))
#define GP_PTR(OFF) ((const char *)D.grows + (unsigned)(OFF))
#define BLK4_FETCH(R, OFF) { const char *bp__ = GP_PTR(OFF); R##j0 = *(const float4 *)bp__; R##j1 = *(const float4 *)(bp__ + 256); R##m0 = *(const float4 *)(bp__ + 512);   \
                             R##m1 = *(const float4 *)(bp__ + 768); R##x0 = *(const float *)(bp__ + 1024); R##x1 = *(const float *)(bp__ + 1028); R##x2 = *(const float *)(bp__ + 1032); }
#define BLK2_FETCH(R, OFF) { const char *bp__ = GP_PTR(OFF); R##j0 = *(const float4 *)bp__; R##m0 = *(const float4 *)(bp__ + 256); R##x0 = *(const float *)(bp__ + 512); }
#define SC_SET(R, HIEXPR) { const v4f_ sc__ = LDS_F4(R##a); R##rhs = sc__.x; R##di = sc__.y; R##lam = sc__.w; R##hi = (HIEXPR); }
    // N pass: the lane's row is the normal row of contact 4 b + rho
    const unsigned gpn_l = gp_l + GP_N * 256, nsc_l = gsc_b + (unsigned)rho * 96u;
#define N_OFF(I) (gpn_l + (unsigned)(I) * 1280u)
    typedef __attribute__((address_space(3))) const v2f lds_cf2;
    // (the bound coefficient of a normal row is not read: a 16-byte read whose third word is dead makes the next writer of that register wait for the LDS)
#define N_SC(R, I) { R##a = (int)(nsc_l + (unsigned)(I) * 384u); const v2f rd__ = *(lds_cf2 *)(size_t)(unsigned)R##a; R##rhs = rd__.x; R##di = rd__.y; R##lam = LDS_F(R##a + 12); R##hi = 1e10f; }
    // F pass: the lateral rows 6 j + 1 + h of contact j; T pass: the torsional rows 6 j + 3 + rho (rho 3: absent -> dummy contact)
    const unsigned gpf_l = gp_l + GP_F * 256, fsc_l = gsc_b + (hh ? 32u : 16u), gpt_l = gp_l + GP_T * 256, tsc_l = gsc_b + (rho == 3 ? MAXC * 96u : 48u + 16u * (unsigned)rho);
#define F_OFF(J) (gpf_l + (unsigned)(J) * 768u)
#define F_SC(R, J) { const unsigned t__ = (unsigned)(J) * 96u; R##a = (int)(fsc_l + t__); const float ln__ = LDS_F(gsc_b + t__ + 12u); SC_SET(R, sc__.z * ln__) }
#define T_OFF(J) (gpt_l + (unsigned)(J) * 1280u)
#define T_SC(R, J) { const unsigned t__ = (unsigned)(J) * 96u; R##a = (int)(tsc_l + (rho == 3 ? 0u : t__)); const float ln__ = LDS_F(gsc_b + t__ + 12u); SC_SET(R, sc__.z * ln__) }
#define DPPF(CTRL, V) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(V), (CTRL), 0xf, 0xf, false))
#define BLK_ROW(R, LANE, X, M0, M1)                                                                                    \
                {                                                                                                      \
                    sum_ = __builtin_amdgcn_fmed3f(s_, lo_, hi_);                                                      \
                    const float b_ = row_bcast<LANE>(sum_ - lam_);                                                     \
                    s_ = fmaf((X), b_, s_);                                                                            \
                    V_ = pk_fma(P2((M0), (M1)), P2(b_, b_), V_);                                                       \
                }
#define BLK_LAST(R, LANE, M0, M1)                                                                                      \
                {                                                                                                      \
                    sum_ = __builtin_amdgcn_fmed3f(s_, lo_, hi_);                                                      \
                    const float b_ = row_bcast<LANE>(sum_ - lam_);                                                     \
                    V_ = pk_fma(P2((M0), (M1)), P2(b_, b_), V_);                                                       \
                }
    // one block of four rows (HI: upper bound of the lane's row; lower bound LO).  NEXT: byte offset of the block the register
    // set sweeps next: each part of it is requested as soon as the registers it lands in are free -- the J pairs right behind
    // the products, the first M^-1 J^T pair behind row 1, the rest behind the last row
#define SCHED_FENCE __builtin_amdgcn_sched_barrier(0);
#define BLK4_STEP(R, LO, HI, NEXT)                                                                                     \
                {                                                                                                      \
                    const char *bp__ = GP_PTR(NEXT);                                                                   \
                    v2f p01_ = P2(R##j0.x, R##j0.y) * P2(dq, dq);                                                      \
                    v2f p23_ = P2(R##j1.x, R##j1.y) * P2(dq, dq);                                                      \
                    p01_ = pk_fma(P2(R##j0.z, R##j0.w), P2(vb, vb), p01_);                                             \
                    p23_ = pk_fma(P2(R##j1.z, R##j1.w), P2(vb, vb), p23_);                                             \
                    SCHED_FENCE                                                                                        \
                    R##j0 = *(const float4 *)bp__; R##j1 = *(const float4 *)(bp__ + 256);                             \
                    SCHED_FENCE                                                                                        \
                    const float s0_ = p01_.x + dpp_ror<8>(p01_.y);                                                     \
                    const float s1_ = p23_.x + dpp_ror<8>(p23_.y);                                                     \
                    float u_ = s0_ + DPPF(0x141, s1_);                                                                 \
                    u_ += DPPF(0xB1, u_);                                                                              \
                    u_ += DPPF(0x4E, u_);                                                                              \
                    const float lam_ = R##lam, lo_ = (LO), hi_ = (HI);                                                 \
                    float s_ = fmaf(-u_, R##di, lam_ + R##rhs), sum_;                                                  \
                    v2f V_ = P2(dq, vb);                                                                               \
                    BLK_ROW(R, 0, R##x0, R##m0.x, R##m0.y)                                                             \
                    BLK_ROW(R, 8, R##x1, R##m0.z, R##m0.w)                                                             \
                    SCHED_FENCE                                                                                        \
                    R##m0 = *(const float4 *)(bp__ + 512);                                                             \
                    SCHED_FENCE                                                                                        \
                    BLK_ROW(R, 4, R##x2, R##m1.x, R##m1.y)                                                             \
                    BLK_LAST(R, 12, R##m1.z, R##m1.w)                                                                  \
                    dq = V_.x; vb = V_.y;                                                                              \
                    LDS_F(R##a + 12) = sum_;                                                                           \
                    R##m1 = *(const float4 *)(bp__ + 768); R##x0 = *(const float *)(bp__ + 1024); R##x1 = *(const float *)(bp__ + 1028); R##x2 = *(const float *)(bp__ + 1032); \
                }
    // one block of two rows (lanes 0..7: the first row, 8..15: the second)
#define BLK2_STEP(R, LO, HI, NEXT)                                                                                     \
                {                                                                                                      \
                    const char *bp__ = GP_PTR(NEXT);                                                                   \
                    v2f p_ = P2(R##j0.x, R##j0.y) * P2(dq, dq);                                                        \
                    p_ = pk_fma(P2(R##j0.z, R##j0.w), P2(vb, vb), p_);                                                 \
                    SCHED_FENCE                                                                                        \
                    R##j0 = *(const float4 *)bp__;                                                                     \
                    SCHED_FENCE                                                                                        \
                    float u_ = p_.x + dpp_ror<8>(p_.y);                                                                \
                    u_ += DPPF(0x141, u_);                                                                             \
                    u_ += DPPF(0xB1, u_);                                                                              \
                    u_ += DPPF(0x4E, u_);                                                                              \
                    const float lam_ = R##lam, lo_ = (LO), hi_ = (HI);                                                 \
                    float s_ = fmaf(-u_, R##di, lam_ + R##rhs), sum_;                                                  \
                    v2f V_ = P2(dq, vb);                                                                               \
                    BLK_ROW(R, 0, R##x0, R##m0.x, R##m0.y)                                                             \
                    BLK_LAST(R, 8, R##m0.z, R##m0.w)                                                                   \
                    dq = V_.x; vb = V_.y;                                                                              \
                    LDS_F(R##a + 12) = sum_;                                                                           \
                    R##m0 = *(const float4 *)(bp__ + 256); R##x0 = *(const float *)(bp__ + 512);                       \
                }
    if (GEN) *(volatile int *)&LD(fix + LF_ENVW) = env;
    // (coop: groups 1..3 of the wave have no rows of their own -- their lanes are switched off for the sweeps)
    if (!(coop && cg != 0))
    for (int it = 0; it < P.iters; it++) {
        // compiler barrier: the row data in LDS / global memory is loop invariant, but hoisting hundreds of such loads out
        // of the sweep loop exhausts the register file (everything that should live in registers is held explicitly)
        asm volatile("" ::: "memory");
        if (simple) {
            SWEEP_MOTORS
            LIMIT_STEP(0) LIMIT_STEP(1)
            if (GEN) {
                OSN_STEP(0) OSN_STEP(1) OSN_STEP(2) OSN_STEP(3)
                OSF_STEP(0) OSF_STEP(1) OSF_STEP(2) OSF_STEP(3)
                OST_STEP(0) OST_STEP(1) OST_STEP(2) OST_STEP(3)
            }
            continue;
        }
        SPROF(4);
        SWEEP_MOTORS
        LIMIT_STEP(0) LIMIT_STEP(1)
        LIMIT_LOOP
        SPROF(7);
        if (!GEN) continue;                         // (the object chains are the object wave's)
#pragma unroll 1
        for (int pass = 0; pass < 3; pass++) {    // all normals, then all lateral frictions, then all torsional frictions
            // ---- the generic sweep of this pass: its first blocks are requested before the object lanes' own work
            const int cnt = pass == 0 ? nb_g : (pass == 1 ? nA : nT);
#define WAVE_MAX4(V) (coop ? __builtin_amdgcn_readlane((V), 0) : max(max(__builtin_amdgcn_readlane((V), 0), __builtin_amdgcn_readlane((V), 16)), max(__builtin_amdgcn_readlane((V), 32), __builtin_amdgcn_readlane((V), 48))))
            const int cmax = pass == 0 ? nb_max : WAVE_MAX4(cnt);
            const unsigned lst_b = list_b + (pass == 2 ? 64u : 0u);
            int jn_ = MAXC;                                   // (F / T pass: the contact of the block after the next one)
            if (cmax > 0) {
                if (pass == 0) {
                    BLK4_FETCH(A, N_OFF(0))
                } else if (pass == 1) {
                    BLK2_FETCH(A, F_OFF(BLK_ENTRY(0)))
                } else {
                    BLK4_FETCH(A, T_OFF(BLK_ENTRY(0)))
                }
            }
            // ---- object-vs-static rows of this pass (object lanes, side by side; all register resident)
            if (pass == 0) { OSN_STEP(0) OSN_STEP(1) OSN_STEP(2) OSN_STEP(3) }
            else if (pass == 1) { OSF_STEP(0) OSF_STEP(1) OSF_STEP(2) OSF_STEP(3) }
            else { OST_STEP(0) OST_STEP(1) OST_STEP(2) OST_STEP(3) }
            SPROF(8);
            if (cmax == 0) continue;
            OBJ_SLOTS(TO_SLOT)
            SPROF(9);
            // (one block per trip: the records of block i + 1 are requested inside the step of block i, its scalars behind it)
            // (the scalars of the pass' first block: requested only now -- the object lanes' rows need the registers)
            if (pass == 0) { N_SC(A, 0) }
            else if (pass == 1) { const int ja_ = BLK_ENTRY(0); jn_ = BLK_ENTRY(1); F_SC(A, ja_) }
            else { const int ja_ = BLK_ENTRY(0); jn_ = BLK_ENTRY(1); T_SC(A, ja_) }
            if (pass == 0) {
#define N_ITER(R, R2, I)                                                                                               \
                {                                                                                                      \
                    BLK4_STEP(R, 0.0f, R##hi, N_OFF((I) + 1))                                                          \
                    N_SC(R2, (I) + 1)                                                                                  \
                }
                for (int i0 = 0; i0 < cmax; i0++) N_ITER(A, A, i0)
#undef N_ITER
            } else if (pass == 1) {
#define F_ITER(R, R2, I)                                                                                               \
                {                                                                                                      \
                    const int j1_ = jn_;                                                                               \
                    jn_ = BLK_ENTRY((I) + 2);                                                                          \
                    BLK2_STEP(R, -R##hi, R##hi, F_OFF(j1_))                                                            \
                    F_SC(R2, j1_)                                                                                      \
                }
                for (int i0 = 0; i0 < cmax; i0++) F_ITER(A, A, i0)
#undef F_ITER
            } else {
#define T_ITER(R, R2, I)                                                                                               \
                {                                                                                                      \
                    const int j1_ = jn_;                                                                               \
                    jn_ = BLK_ENTRY((I) + 2);                                                                          \
                    BLK4_STEP(R, -R##hi, R##hi, T_OFF(j1_))                                                            \
                    T_SC(R2, j1_)                                                                                      \
                }
                for (int i0 = 0; i0 < cmax; i0++) T_ITER(A, A, i0)
#undef T_ITER
            }
            if (pass == 0) SPROF(10); else if (pass == 1) SPROF(5); else SPROF(6);      // (generic blocks: normal / lateral / torsional pass)
            OBJ_SLOTS(FROM_SLOT)
            if (pass == 0) {
                // ---- the contacts whose lateral and torsional rows can move something: those with a normal impulse, or with a
                //      lateral / torsional impulse left from the previous sweep.  The lists keep their dummy padding.
                const int nA_old = nA, nT_old = nT;
                nA = 0; nT = 0;
                // (one LDS read per contact: a lateral / torsional impulse can only be non-zero where the normal impulse was positive
                // a sweep earlier -- its bound is mu x that impulse --, so "positive now or a sweep ago" covers every row that can move
                // anything; a contact listed beyond that is an exact no-op.  Which contacts have torsional rows is known from the build.)
                unsigned pos_now = 0u;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int j = 16 * c + l;
                    if (16 * c >= ng_max) break;                 // (wave-uniform)
                    const bool pos = j < ng && LD(L_GSC + 24 * (j < ng ? j : 0) + 3) > 0.0f;
                    const bool act = pos | (((act_prev >> c) & 1u) != 0u);
                    const bool ht = act & (((tors_bits >> c) & 1u) != 0u);
                    pos_now |= (pos ? 1u : 0u) << c;
                    const unsigned lt = (1u << l) - 1u;
                    const unsigned ma = (unsigned)(__ballot(act) >> (16 * (grp & 3))) & 0xffffu, mt = (unsigned)(__ballot(ht) >> (16 * (grp & 3))) & 0xffffu;
                    if (act) listA[nA + __popc(ma & lt)] = (unsigned char)j;
                    if (ht) listT[nT + __popc(mt & lt)] = (unsigned char)j;
                    nA += __popc(ma); nT += __popc(mt);
                }
                act_prev = pos_now;
                // (entries a shrinking list leaves behind become dummies again: sixteen behind the new end at once, more only
                // when a list lost more than that in one sweep)
                listA[nA + l] = (unsigned char)MAXC; listT[nT + l] = (unsigned char)MAXC;
                if (__ballot((nA_old - nA > 16) | (nT_old - nT > 16)) != 0ull) {
                    for (int k = 16 + l; nA + k < nA_old; k += 16) listA[nA + k] = (unsigned char)MAXC;
                    for (int k = 16 + l; nT + k < nT_old; k += 16) listT[nT + k] = (unsigned char)MAXC;
                }
            }
            SPROF(11);
            SPROF(3);           // (calibration: two stamps back to back -- the cost of a stamp, once per pass)
        }
    }
    SPROF(4);
    // (GEN: the env index is parked in LDS over the sweeps -- the kernel with the generic rows has no register to spare there)
    if (GEN) env = *(volatile int *)&LD(fix + LF_ENVW);
    SBLK_MARK(sb_t2)
    SBLK_END(nc, ng, n_os, nA);
    SPROF_FLUSH;
    // normal impulses of the register-resident contact rows go back to their LDS slots (contact forces below)
#pragma unroll
    for (int i = 0; i < (GEN ? KOS : 0); i++) {
        const int c = (os_cs >> (8 * i)) & 255;
        if (c != 255) LD(L_OSL + (3 * c) * 12 + 11) = os_ln[i];
    }
    // (the light solve of a step with camera also sets up the render instances of its envs -- below; an env that does not
    // step is drawn as it stands)
    const bool setup = RSETUP && RMp != nullptr && mine && env_raw < N && !(GEN && coop && cg != 0);      // (coop: group 0 of the wave has the env)
    if (dead && !setup) return;
    // (the lane predicates of the tail are taken from a copy of the lane index the compiler cannot see through: lane masks of
    // the stage-in kept alive over the sweeps cost scalar registers the solver does not have)
    int lt = l;
    asm volatile("" : "+v"(lt));
    float q_fin = q_l;                 // joint angle / object pose after this step: what the render instances are set up from
    float o_fin[7] = {0, 0, 0, 0, 0, 0, 1};
    if (dead) {
        if (GEN && lt >= NB && lt - NB < P.nobj) {
#pragma unroll
            for (int k = 0; k < 3; k++) o_fin[k] = STT(ST_OPOS + 3 * (lt - NB) + k);
#pragma unroll
            for (int k = 0; k < 4; k++) o_fin[3 + k] = STT(ST_OQUAT + 4 * (lt - NB) + k);
        }
    } else {
    // ---- integrate: lanes 0..10 joints, lanes 11..13 objects
    bool finite = true;
    if (lt < NB) {
        // (GEN: the kernel with the generic rows reads the two values again instead of holding them over the sweeps, like the objects' below)
        const float qds_t = GEN ? SCR(S_QDS + (lt < NB ? lt : 0)) : qds_l, q_t = GEN ? STT(ST_Q + (lt < NB ? lt : 0)) : q_l;
        float v = qds_t + dq;
        float qn = fmaf(dt, v, q_t);            // (the integration is written out in fused operations: both forms of the kernel must round alike)
        finite = isfinite(qn);
        q_fin = qn;
        STT(ST_QD + lt) = v;
        STT(ST_Q + lt) = qn;
        if (lt < 7) D.joints[(size_t)env * 9 + lt] = qn;               // robot.py:203-211
        else if (lt == 7) D.joints[(size_t)env * 9 + 7] = qn;
        else if (lt == 8) D.joints[(size_t)env * 9 + 8] = -qn;
    }
    if (GEN && lt >= NB && lt - NB < P.nobj) {
        // (position, orientation and unconstrained velocities are the registers of the stage-in: no load at the tail of the chain)
        const int i = lt - NB;
        float v[3], w[3], pn[3];
        const float dvi[3] = {DVX, DVY, DVZ}, dwi[3] = {DWX, DWY, DWZ};
        // (GEN: the solver with the generic rows has no 13 registers to spare over the sweeps -- it reads them again)
        float vs3[3] = {myobj.vs.x, myobj.vs.y, myobj.vs.z}, ws3[3] = {myobj.ws.x, myobj.ws.y, myobj.ws.z};
        float op3[3] = {myobj.op.x, myobj.op.y, myobj.op.z};
        if (GEN) {
#pragma unroll
            for (int k = 0; k < 3; k++) { vs3[k] = SCR(S_OVS + 3 * i + k); ws3[k] = SCR(S_OWS + 3 * i + k); op3[k] = SCR(S_OP + 3 * i + k); }
#pragma unroll
            for (int k = 0; k < 4; k++) oquat[k] = STT(ST_OQUAT + 4 * i + k);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = vs3[k] + dvi[k];
            w[k] = ws3[k] + dwi[k];
            pn[k] = fmaf(dt, v[k], op3[k]);
            finite = finite && isfinite(pn[k]);
            STT(ST_OVEL + 3 * i + k) = v[k];
            STT(ST_OANG + 3 * i + k) = w[k];
            STT(ST_OPOS + 3 * i + k) = pn[k];
        }
        float wn = sqrtf(fmaf(w[0], w[0], fmaf(w[1], w[1], w[2] * w[2])));
        float ang = wn * dt, d0, d1, d2, d3;
        if (ang > 1e-12f) {
            float sn, cs;
            sincosf(ang * 0.5f, &sn, &cs);
            float s = sn / wn;
            d0 = w[0] * s; d1 = w[1] * s; d2 = w[2] * s; d3 = cs;
        } else {
            d0 = w[0] * dt * 0.5f; d1 = w[1] * dt * 0.5f; d2 = w[2] * dt * 0.5f; d3 = 1.0f;
        }
        float q0 = oquat[0], q1 = oquat[1], q2 = oquat[2], q3 = oquat[3];
        float r0 = fmaf(d3, q0, fmaf(d0, q3, fmaf(d1, q2, -(d2 * q1))));
        float r1 = fmaf(d3, q1, fmaf(-d0, q2, fmaf(d1, q3, d2 * q0)));
        float r2 = fmaf(d3, q2, fmaf(d0, q1, fmaf(-d1, q0, d2 * q3)));
        float r3 = fmaf(d3, q3, fmaf(-d0, q0, fmaf(-d1, q1, -(d2 * q2))));
        float inv = 1.0f / sqrtf(fmaf(r0, r0, fmaf(r1, r1, fmaf(r2, r2, r3 * r3))));
        STT(ST_OQUAT + 4 * i) = r0 * inv; STT(ST_OQUAT + 4 * i + 1) = r1 * inv;
        STT(ST_OQUAT + 4 * i + 2) = r2 * inv; STT(ST_OQUAT + 4 * i + 3) = r3 * inv;
        float *op = D.objpose + ((size_t)env * P.nobj + i) * 7;
        for (int k = 0; k < 3; k++) op[k] = pn[k];
        op[3] = r0 * inv; op[4] = r1 * inv; op[5] = r2 * inv; op[6] = r3 * inv;
        o_fin[0] = pn[0]; o_fin[1] = pn[1]; o_fin[2] = pn[2];
        o_fin[3] = r0 * inv; o_fin[4] = r1 * inv; o_fin[5] = r2 * inv; o_fin[6] = r3 * inv;
    }
    SPROF(5);
    if (!finite) atomicOr(&D.errflags[env], 1u);
    // ---- touch sensors (robot.py:152-163) + contact forces: lane c takes contacts c, c + 16, c + 32; the four maxima go round
    // the group (a maximum does not depend on the order it is taken in)
    if (!GEN) {
        // (a light env has no contact of the robot: the touch sensors read zero; the contact forces are the object wave's)
        if (l < 4) D.touch[(size_t)env * 4 + l] = 0.0f;
        if (l == 0) D.timestep[env] += 1;
    } else {
        float touch[4] = {0, 0, 0, 0};
        for (int c0 = 0; c0 < nc; c0 += 16) {
            const int c = c0 + l;
            if (c < nc) {
                const int meta = *(const int *)&LD(L_META + c);
                const int bodyA = meta_bodyA(meta), link = meta_link(meta);
                const float lam = meta_fast(meta) ? LD(L_OSL + (3 * meta_slot(meta)) * 12 + 11) : LD(L_GSC + 24 * meta_slot(meta) + 3);
                const float f = lam / dt;
                D.cforce[(size_t)env * MAXC + c] = f;
                if (bodyA >= 0 && bodyA < 16 && meta_near(meta)) {
#pragma unroll
                    for (int k = 0; k < 4; k++) if (link == B.touch_links[k]) touch[k] = fmaxf(touch[k], f);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float m = touch[k];
            m = fmaxf(m, dpp_ror<8>(m)); m = fmaxf(m, dpp_ror<4>(m)); m = fmaxf(m, dpp_ror<2>(m)); m = fmaxf(m, dpp_ror<1>(m));
            touch[k] = m;
        }
        if (l == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) D.touch[(size_t)env * 4 + k] = touch[k];
            D.timestep[env] += 1;
        }
    }
    }       // (!dead)
    SPROF(6);
    // ---- render set-up of this env's instances (k_render_setup's work, from the values just integrated: the joint angles
    // go round the group by DPP, the object poses through LDS; lane l takes instances l and 16 + l).  The kernel with the generic rows
    // does the same for the heavy classes when the step draws (RMp): their render then starts without a set-up launch / pass of its own.
    if (RSETUP) {
        if (!setup) return;
        const RenderModel &RM = *RMp;
        if (GEN && lt >= NB && lt < NB + NOBJ) {
#pragma unroll
            for (int k = 0; k < 7; k++) LD(L_OBJ + 20 * (lt - NB) + k) = o_fin[k];
        }
        float qj[NB];
        static_assert(NB == 11, "joint angles round the group");
        qj[0] = row_bcast<0>(q_fin); qj[1] = row_bcast<1>(q_fin); qj[2] = row_bcast<2>(q_fin); qj[3] = row_bcast<3>(q_fin);
        qj[4] = row_bcast<4>(q_fin); qj[5] = row_bcast<5>(q_fin); qj[6] = row_bcast<6>(q_fin); qj[7] = row_bcast<7>(q_fin);
        qj[8] = row_bcast<8>(q_fin); qj[9] = row_bcast<9>(q_fin); qj[10] = row_bcast<10>(q_fin);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int i = lt; i < RM.ni; i += 16) {
            const int ot = RM.in_otype[i], oi = RM.in_oidx[i];
            if (!GEN && ot == 2) continue;          // (an object's instances are set up by the object wave, from what it integrated)
            float op7[7];
            const int ob = ot == 2 ? min(max(oi, 0), NOBJ - 1) : 0;
#pragma unroll
            for (int k = 0; k < 7; k++) op7[k] = LD(L_OBJ + 20 * ob + k);
            instance_setup_core(B, RM, D, env, i, ot, oi, qj, op7);
        }
    }
}
// The object wave of a k_solve_light_ow workgroup (solve_body<false>): the object chains of the workgroup's sixteen envs, lane 3 e + o =
// object o of env e.  Everything it needs was staged in LDS by the env's group before the workgroup's barrier: the objects'
// data (L_OBJ), the rows of the contacts (L_OSL / L_OST, coefficients), flags, contact masks and orientations (OW_*).  Same
// row steps, same order within a chain, same integration as the object lanes of the one-kernel form: same bits.
__device__ __forceinline__ void light_object_wave(const BodyParams &B, const SimParams &P, const DevPtrs &D, const RenderModel *RMp) {
    const int N = P.N;
    const int t = threadIdx.x & 63;
    const int e = min(t / 3, 15), o = t - 3 * (t / 3);
    const int env_raw = 16 * (int)blockIdx.x + e;
    const bool lane_on = t < 48 && o < P.nobj && env_raw < N;
    const int env = env_raw < N ? env_raw : N - 1;
    const int fix = e * LF_TOTAL;
    const int L_MU = fix + LF_MU, L_SPIN = fix + LF_SPIN, L_ROLL = fix + LF_ROLL, L_OSL = fix + LF_OSL, L_OST = fix + LF_OST,
              L_GSC = fix + LF_GSC, L_OBJ = fix + LF_OBJ;
    float *state = D.state;
    const float dt = P.dt;
#ifdef RR_RASTER_STATS
    unsigned long long ow_t0 = __builtin_amdgcn_s_memrealtime();      // (100 MHz: the shader clock counter runs with the DVFS state)
#define OWPROF(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); if (t == 0 && (!(P.ablate & 0x4000) || (int)blockIdx.x == (P.ablate >> 16))) atomicAdd(&g_sprof[i], now_ - ow_t0); ow_t0 = now_; } while (0)
#else
#define OWPROF(i)
#endif
    // (while the env groups stage in and build rows: which render instance is this object's -- uniform loads, one round trip)
    int my_inst = -1, my_inst2 = -1;
    if (RMp) {
        const RenderModel &RM = *RMp;
        const int ni = RM.ni;
#pragma unroll
        for (int i = 0; i < MAXINST; i++) {
            const bool m_ = i < ni && RM.in_otype[i] == 2 && RM.in_oidx[i] == o;
            my_inst2 = (m_ && my_inst >= 0 && my_inst2 < 0) ? i : my_inst2;
            my_inst = (m_ && my_inst < 0) ? i : my_inst;
        }
    }
#ifdef RR_RASTER_STATS
    if (t == 0 && blockIdx.x < 4096) g_sblk[(2048 + blockIdx.x) * 8] = (unsigned)ow_t0;       // (scratch/ow_blocks.py: when did this workgroup start / end?)
#endif
    __syncthreads();
    OWPROF(8);           // waiting for the env groups (stage-in, command part, row build)
    const int flags = *(const int *)&LD(L_GSC + OW_FLAGS);
    if (!lane_on || !(flags & 1)) return;          // (per lane: nothing below crosses lanes)
    const bool dead = (flags & 2) != 0;
    const unsigned own_os = dead ? 0u : *(const unsigned *)&LD(L_GSC + OW_MASK + o);
    const float inv_mass = LD(L_OBJ + 20 * o + 3);
    float o_fin[7] = {0, 0, 0, 0, 0, 0, 1};
    if (dead) {
        if (!RMp) return;
#pragma unroll
        for (int k = 0; k < 3; k++) o_fin[k] = STT(ST_OPOS + 3 * o + k);
#pragma unroll
        for (int k = 0; k < 4; k++) o_fin[3 + k] = STT(ST_OQUAT + 4 * o + k);
    } else {
    // ---- this object's contacts: all six rows of each in registers (as the object lanes of solve_body hold them)
    unsigned os_cs = 0;
    float os_mu[KOS], os_ln[KOS], os_l1[KOS], os_l2[KOS], os_l0[KOS];
    float4 os_n0[KOS], os_n1[KOS], os_n2[KOS], os_a0[KOS], os_a1[KOS], os_a2[KOS], os_b0[KOS], os_b1[KOS], os_b2[KOS];
    {
        unsigned rem = own_os;
#pragma unroll
        for (int i = 0; i < KOS; i++) {
            const bool has = rem != 0;
            const int c = has ? __ffs(rem) - 1 : 0;
            rem &= rem - 1;
            os_cs |= (has ? (unsigned)c : 255u) << (8 * i);
            os_mu[i] = has ? LD(L_MU + c) : 0.0f; os_ln[i] = 0.0f; os_l1[i] = 0.0f; os_l2[i] = 0.0f;
            os_l0[i] = has ? LD(L_OST + (3 * c) * 8 + 5) : 0.0f;
            os_n0[i] = LDZ4(has, 3 * c, 0); os_n1[i] = LDZ4(has, 3 * c, 4); os_n2[i] = LDZ4(has, 3 * c, 8);
            os_a0[i] = LDZ4(has, 3 * c + 1, 0); os_a1[i] = LDZ4(has, 3 * c + 1, 4); os_a2[i] = LDZ4(has, 3 * c + 1, 8);
            os_b0[i] = LDZ4(has, 3 * c + 2, 0); os_b1[i] = LDZ4(has, 3 * c + 2, 4); os_b2[i] = LDZ4(has, 3 * c + 2, 8);
        }
    }
    float4 ot_m[KOS][3]; float ot_d[KOS][3], ot_l[KOS][3], os_sp[KOS], os_ro[KOS];
#pragma unroll
    for (int i = 0; i < KOS; i++) {
        const int c = (os_cs >> (8 * i)) & 255;
        const bool has = c != 255;
        const int cc = has ? c : 0;
        os_sp[i] = has ? LD(L_SPIN + cc) : 0.0f; os_ro[i] = has ? LD(L_ROLL + cc) : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            ot_m[i][k] = sel4(has, LDT4(3 * cc + k, 0));
            ot_d[i][k] = has ? LD(L_OST + (3 * cc + k) * 8 + 4) : 0.0f;
            ot_l[i][k] = 0.0f;
        }
    }
    OWPROF(9);           // rows from LDS to registers
    v2f V01 = P2(0.0f, 0.0f), V23 = P2(0.0f, 0.0f), V45 = P2(0.0f, 0.0f);
    // warm start: the inherited normal impulses
#pragma unroll
    for (int i = 0; i < KOS; i++) {
        const float l0_ = os_l0[i], sm_ = l0_ * inv_mass;
        os_ln[i] = l0_;
        V01 = pk_fma(P2(os_n0[i].x, os_n0[i].y), P2(sm_, sm_), V01);
        V23.x = fmaf(os_n0[i].z, sm_, V23.x); V23.y = fmaf(os_n1[i].w, l0_, V23.y);
        V45 = pk_fma(P2(os_n2[i].x, os_n2[i].y), P2(l0_, l0_), V45);
    }
    // (the middle pair's update as two scalar FMAs on dir.z of the first pair: the same two operations as the packed one, and the
    // twelve registers of the rows' second copy of dir.z go to row data the wave would otherwise spill -- it shares its SIMD)
#pragma push_macro("REG_ROW_STEP")
#undef REG_ROW_STEP
#define REG_ROW_STEP(b0, b1, b2, lam, lo, hi)                                                                     \
    do {                                                                                                          \
        v2f p_ = P2((b0).x, (b0).y) * V01;                                                                        \
        p_ = pk_fma(P2((b0).z, (b0).w), V23, p_);                                                                 \
        p_ = pk_fma(P2((b1).x, (b1).y), V45, p_);                                                                 \
        const float jv_ = p_.x + p_.y;                                                                            \
        const float s0_ = fmaf(-jv_, (b2).w, (lam) + (b2).z);                                                     \
        const float sum_ = __builtin_amdgcn_fmed3f(s0_, (lo), (hi));                                              \
        const float dl_ = sum_ - (lam);                                                                           \
        (lam) = sum_;                                                                                             \
        const float sm_ = dl_ * inv_mass;                                                                         \
        V01 = pk_fma(P2((b0).x, (b0).y), P2(sm_, sm_), V01);                                                      \
        V23.x = fmaf((b0).z, sm_, V23.x); V23.y = fmaf((b1).w, dl_, V23.y);                                       \
        V45 = pk_fma(P2((b2).x, (b2).y), P2(dl_, dl_), V45);                                                      \
    } while (0)
    for (int it = 0; it < P.iters; it++) {
        asm volatile("" ::: "memory");
        OSN_STEP(0) OSN_STEP(1) OSN_STEP(2) OSN_STEP(3)
        OSF_STEP(0) OSF_STEP(1) OSF_STEP(2) OSF_STEP(3)
        OST_STEP(0) OST_STEP(1) OST_STEP(2) OST_STEP(3)
    }
#pragma pop_macro("REG_ROW_STEP")
    OWPROF(10);          // sweeps
    // ---- contact forces of this object's contacts (robot.py:131-150 reads them)
#pragma unroll
    for (int i = 0; i < KOS; i++) {
        const int c = (os_cs >> (8 * i)) & 255;
        if (c != 255) D.cforce[(size_t)env * MAXC + c] = os_ln[i] / dt;
    }
    // ---- integrate (the object lanes' code of solve_body, same operations); the object's pose and unconstrained velocities are
    // fetched from LDS only now: thirteen registers the sweeps need for row data
    bool finite = true;
    {
        const int i = o;
        float op3[3], vs3[3], ws3[3], oquat[4];
        {
            asm volatile("" ::: "memory");
            const float4 *od = (const float4 *)&LD(L_OBJ + 20 * o);
            const float4 d0 = od[0], d3 = od[3], d4 = od[4];
            op3[0] = d0.x; op3[1] = d0.y; op3[2] = d0.z;
            vs3[0] = d3.y; vs3[1] = d3.z; vs3[2] = d3.w; ws3[0] = d4.x; ws3[1] = d4.y; ws3[2] = d4.z;
#pragma unroll
            for (int k = 0; k < 4; k++) oquat[k] = LD(L_GSC + OW_QUAT + 4 * o + k);
        }
        float v[3], w[3], pn[3];
        const float dvi[3] = {DVX, DVY, DVZ}, dwi[3] = {DWX, DWY, DWZ};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = vs3[k] + dvi[k];
            w[k] = ws3[k] + dwi[k];
            pn[k] = fmaf(dt, v[k], op3[k]);
            finite = finite && isfinite(pn[k]);
            STT(ST_OVEL + 3 * i + k) = v[k];
            STT(ST_OANG + 3 * i + k) = w[k];
            STT(ST_OPOS + 3 * i + k) = pn[k];
        }
        float wn = sqrtf(fmaf(w[0], w[0], fmaf(w[1], w[1], w[2] * w[2])));
        float ang = wn * dt, d0, d1, d2, d3;
        if (ang > 1e-12f) {
            float sn, cs;
            sincosf(ang * 0.5f, &sn, &cs);
            float s_ = sn / wn;
            d0 = w[0] * s_; d1 = w[1] * s_; d2 = w[2] * s_; d3 = cs;
        } else {
            d0 = w[0] * dt * 0.5f; d1 = w[1] * dt * 0.5f; d2 = w[2] * dt * 0.5f; d3 = 1.0f;
        }
        float q0 = oquat[0], q1 = oquat[1], q2 = oquat[2], q3 = oquat[3];
        float r0 = fmaf(d3, q0, fmaf(d0, q3, fmaf(d1, q2, -(d2 * q1))));
        float r1 = fmaf(d3, q1, fmaf(-d0, q2, fmaf(d1, q3, d2 * q0)));
        float r2 = fmaf(d3, q2, fmaf(d0, q1, fmaf(-d1, q0, d2 * q3)));
        float r3 = fmaf(d3, q3, fmaf(-d0, q0, fmaf(-d1, q1, -(d2 * q2))));
        float inv = 1.0f / sqrtf(fmaf(r0, r0, fmaf(r1, r1, fmaf(r2, r2, r3 * r3))));
        STT(ST_OQUAT + 4 * i) = r0 * inv; STT(ST_OQUAT + 4 * i + 1) = r1 * inv;
        STT(ST_OQUAT + 4 * i + 2) = r2 * inv; STT(ST_OQUAT + 4 * i + 3) = r3 * inv;
        float *op = D.objpose + ((size_t)env * P.nobj + i) * 7;
        for (int k = 0; k < 3; k++) op[k] = pn[k];
        op[3] = r0 * inv; op[4] = r1 * inv; op[5] = r2 * inv; op[6] = r3 * inv;
        o_fin[0] = pn[0]; o_fin[1] = pn[1]; o_fin[2] = pn[2];
        o_fin[3] = r0 * inv; o_fin[4] = r1 * inv; o_fin[5] = r2 * inv; o_fin[6] = r3 * inv;
    }
    if (!finite) atomicOr(&D.errflags[env], 1u);
    OWPROF(11);          // forces, integration
    }       // (!dead)
    // ---- the render instances of this object
    if (RMp) {
        const RenderModel &RM = *RMp;
        const float qj[NB] = {0};
        if (my_inst >= 0) instance_setup_core(B, RM, D, env, my_inst, 2, o, qj, o_fin);
        if (my_inst2 >= 0) {          // (an object drawn as more than two instances: the rest in a loop)
            instance_setup_core(B, RM, D, env, my_inst2, 2, o, qj, o_fin);
#pragma unroll 1
            for (int i = my_inst2 + 1; i < RM.ni; i++)
                if (RM.in_otype[i] == 2 && RM.in_oidx[i] == o) instance_setup_core(B, RM, D, env, i, 2, o, qj, o_fin);
        }
    }
    OWPROF(12);          // render instances
#ifdef RR_RASTER_STATS
    if (t == 0 && blockIdx.x < 4096) g_sblk[(2048 + blockIdx.x) * 8 + 1] = (unsigned)__builtin_amdgcn_s_memrealtime();
#endif
}
__global__ void __launch_bounds__(256) k_solve(BodyParams B, SimParams P, DevPtrs D, int sel, int coop_launch) { solve_body<true>(B, P, D, sel, coop_launch); }
// ... and with the render set-up of its envs in its tail (the heavy classes of a step that draws)
__global__ void __launch_bounds__(256) k_solve_rs(BodyParams B, SimParams P, DevPtrs D, int sel, int coop_launch, const RenderModel *RMp) { solve_body<true, true>(B, P, D, sel, coop_launch, RMp); }
// the light envs of a split step (sel 1), in workgroups for sixteen envs with one wave running the object chains; the bookkeeping
// of solve_body's first lines is thread 0's whatever its wave's role
// (RMp: the render model when the step draws -- the kernel then sets up the render instances of its envs; else nullptr)
__global__ void __launch_bounds__(LIGHT_OW_THREADS) k_solve_light_ow(BodyParams B, SimParams P, DevPtrs D, const RenderModel *RMp) { solve_body<false>(B, P, D, 1, 0, RMp); }

// obs pack without stepping (after reset / set_state)
__global__ void k_obs(SimParams P, DevPtrs D) {
    const int N = P.N;
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const float *state = D.state;
    for (int i = 0; i < 7; i++) D.joints[(size_t)env * 9 + i] = STT(ST_Q + i);
    D.joints[(size_t)env * 9 + 7] = STT(ST_Q + 7);
    D.joints[(size_t)env * 9 + 8] = -STT(ST_Q + 8);
    for (int i = 0; i < P.nobj; i++) {
        float *op = D.objpose + ((size_t)env * P.nobj + i) * 7;
        for (int k = 0; k < 3; k++) op[k] = STT(ST_OPOS + 3 * i + k);
        for (int k = 0; k < 4; k++) op[3 + k] = STT(ST_OQUAT + 4 * i + k);
    }
}

// Host mirror of the low-dimensional observations (rr_map_observations): device-mapped pinned host memory that a step's last
// launch on the main stream fills -- the single-env facade then needs ONE wait per step and no device-to-host copy calls.
struct ObsMirror { float *joints, *touch, *objpose; int *timestep; unsigned *errflags; };
__global__ void k_obs_mirror(SimParams P, DevPtrs D, ObsMirror M) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= P.N) return;
    for (int i = 0; i < 9; i++) M.joints[(size_t)env * 9 + i] = D.joints[(size_t)env * 9 + i];
    for (int i = 0; i < 4; i++) M.touch[(size_t)env * 4 + i] = D.touch[(size_t)env * 4 + i];
    for (int i = 0; i < P.nobj * 7; i++) M.objpose[(size_t)env * P.nobj * 7 + i] = D.objpose[(size_t)env * P.nobj * 7 + i];
    M.timestep[env] = D.timestep[env];
    M.errflags[env] = D.errflags[env];
}
