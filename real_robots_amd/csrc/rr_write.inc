// rr_write.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_state_rw: the state of the whole batch between the AoS tensor f32 [N][61] of RR_F_STATE and the SoA slab [slot][N], in either
// direction, on the device (rr_write_state, rr_read_state; realrobot.h).  The write is masked and takes the columns by groups -- joint
// positions, joint velocities, object poses, object twists --, optionally behind a reset of the env and in front of the fresh-start
// clean-up of rr_set_state: a device program decides which envs restart and where.  Launched by those two calls alone, never by a
// step.
//
// A transpose, bound by memory traffic.  A thread per env walking its 244-byte row would touch 64 cache lines with every wave-wide
// access, so a 256-thread workgroup owns SW_ENVS = 64 consecutive envs, as k_fork does, and goes through LDS, as k_kinematics does:
//   tensor side  the rows of the workgroup's envs are ONE contiguous span of 64 x 244 = 15 616 bytes, a multiple of 16, so with a
//                16-byte aligned tensor every workgroup's span is aligned and moves as float4, lane i at base + 16 i (a tensor that
//                is only 4-byte aligned -- a view into a larger allocation -- moves float by float; the ragged end of the last
//                workgroup's span too);
//   slab side    (slot, env) pairs, the slot uniform in a wave and lane l on env 64 g + l: every access is one 256-byte line of the
//                slab, and the LDS image [env][61] has an odd row stride, so the 64 lanes hit distinct banks.
// One barrier between the two sides; every thread reaches it (no early return: an env behind the end of the batch has a clear mask
// byte in LDS and stores nothing).
//
// Write (to_aos == 0).  Every (slot, env) pair of the slab has exactly ONE writer that stores at most once, so the order "reset,
// then the columns, then the clean-up" of realrobot.h needs no ordering between threads -- the value a pair ends with is decided in
// one place:
//   the tensor's column            if the slot's group is selected (object slots: and the object is one the handle has),
//   0                              else if the slot is a twist slot of such an object and RR_W_OBJ_POSE is given without
//                                  RR_W_OBJ_VEL (set_object_pose_env: a teleported object is at rest),
//   the reset value                else if RR_W_RESET is given: the home pose in the pose slots of all NOBJ objects, 0 elsewhere --
//                                  motor targets included (reset_env),
//   no store                       otherwise.
// The per-env words behind the slab go to the lane of the env in wave 0: clock 0 with RR_W_RESET; error flags, touch sensors,
// contact count, published count and class 0 with RR_W_RESET or RR_W_FRESH (reset_env; the tail of k_state_io's upload).  The values
// are placed, never computed: the results are those of k_reset / k_set_object_poses / k_state_io bit for bit (tested per pair).
// Neither a tensor value nor a mask byte ever forms an address; values are not looked at (a NaN in a selected column reaches the
// state and the next step's guard, as with rr_set_state), and LDS words of columns that are not selected, of rows whose mask byte
// is clear and of objects the handle does not have are never read back.
// Read (to_aos != 0): all 61 columns of every env -- what k_state_io gathers for rr_copy_to_host --, the mask and the parts ignored.
#define SW_ENVS 64
#define SW_THREADS 256

// Row j of the walk over an env's slab slots: j < 61 is column j of the 61-float row -- q[11] qd[11], per object pos3 quat4 lin3
// ang3 --, the others are the motor targets.  Returns the slab slot; *group: the RR_W_* bit that selects the column (0: a motor
// target), *obj: its object (-1: a joint column), *k: its place in the object's 13 floats.
__device__ __forceinline__ int sw_slot(int j, unsigned *group, int *obj, int *k) {
    static_assert(ST_Q == 0 && ST_QD == NB && ST_OPOS == 2 * NB && ST_TGT == NSTATE && NSTATE == 2 * NB + 13 * NOBJ, "the slab's slots against the 61-float row");
    *obj = -1; *k = 0; *group = 0;
    if (j >= NSTATE) return j;
    if (j < 2 * NB) { *group = j < NB ? RR_W_JOINT_POS : RR_W_JOINT_VEL; return j; }
    const int o = (j - 2 * NB) / 13, r = (j - 2 * NB) % 13;
    *obj = o; *k = r;
    *group = r < 7 ? RR_W_OBJ_POSE : RR_W_OBJ_VEL;
    return r < 3 ? ST_OPOS + 3 * o + r : (r < 7 ? ST_OQUAT + 4 * o + r - 3 : (r < 10 ? ST_OVEL + 3 * o + r - 7 : ST_OANG + 3 * o + r - 10));
}

__global__ void __launch_bounds__(SW_THREADS) k_state_rw(SimParams P, DevPtrs D, float *__restrict__ aos /*[N][61], nullptr: a write without columns*/,
                                                        const unsigned char *__restrict__ mask /*[N] or nullptr: all*/, unsigned parts, int to_aos) {
    static_assert((SW_ENVS * NSTATE * 4) % 16 == 0, "every workgroup's span of the tensor starts on a 16-byte boundary");
    static_assert(SW_THREADS % 64 == 0 && SW_ENVS == 64, "slab side: the row of the walk is uniform in a wave, the lane is the env");
    __shared__ __attribute__((aligned(16))) float s_row[SW_ENVS * NSTATE];
    __shared__ unsigned char s_on[SW_ENVS];
    const int N = P.N, tid = threadIdx.x;
    const int env0 = blockIdx.x * SW_ENVS;
    const int ne = min(SW_ENVS, N - env0);                 // live envs of this workgroup (>= 1 by the grid)
    const int n = ne * NSTATE;                             // floats of its span
    const int n4 = (((size_t)aos & 15) == 0) ? n >> 2 : 0; // float4 of the span that move as such
    float *span = aos ? aos + (size_t)env0 * NSTATE : nullptr;
    float *state = D.state;
    const int lane = tid & 63, env = env0 + lane;
    unsigned g; int o, k;
    if (to_aos) {
        // (an env behind the batch's end reads the last env's state into an LDS row that is not stored)
        for (int i = tid; i < NSTATE * SW_ENVS; i += SW_THREADS) {
            const int j = i >> 6;
            s_row[lane * NSTATE + j] = state[(size_t)sw_slot(j, &g, &o, &k) * N + min(env, N - 1)];
        }
        __syncthreads();
        for (int i = tid; i < n4; i += SW_THREADS) ((float4 *)span)[i] = ((const float4 *)s_row)[i];
        for (int i = 4 * n4 + tid; i < n; i += SW_THREADS) span[i] = s_row[i];
        return;
    }
    if (span) {
        for (int i = tid; i < n4; i += SW_THREADS) ((float4 *)s_row)[i] = ((const float4 *)span)[i];
        for (int i = 4 * n4 + tid; i < n; i += SW_THREADS) s_row[i] = span[i];
    }
    if (tid < SW_ENVS) s_on[tid] = tid < ne && (!mask || mask[env0 + tid]) ? 1 : 0;
    __syncthreads();
    const bool on = s_on[lane] != 0;
    const bool rest = (parts & RR_W_OBJ_POSE) && !(parts & RR_W_OBJ_VEL);
    for (int i = tid; i < ST_TOTAL * SW_ENVS; i += SW_THREADS) {
        const int j = i >> 6;                              // uniform in the wave
        const int s = sw_slot(j, &g, &o, &k);
        const bool have = o < P.nobj;                      // (a joint column: o == -1)
        if (!on) continue;
        if (span && (parts & g) && have) STT(s) = s_row[lane * NSTATE + j];
        else if (rest && g == RR_W_OBJ_VEL && have) STT(s) = 0.0f;
        else if (parts & RR_W_RESET) STT(s) = g == RR_W_OBJ_POSE ? D.obj_home[(size_t)(7 * o + k) * N + env] : 0.0f;
    }
    if (tid < SW_ENVS && on) {
        if (parts & RR_W_RESET) D.timestep[env] = 0;
        if (parts & (RR_W_RESET | RR_W_FRESH)) {
            D.errflags[env] = 0;
            ((float4 *)D.touch)[env] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            D.ccount[env] = 0;
            D.ccount_pub[env] = 0; D.class_pub[env] = 0;
        }
    }
}
