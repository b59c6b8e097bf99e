// rr_cart.inc -- part of realrobot.hip (included there, behind rr_macro.inc; not a stand-alone translation unit).
// Device-resident cartesian actions (rr_step_cartesian, realrobot.h): REALRobotEnv.step_cartesian (env.py:358-386) for the whole batch.
// The handle holds a request record f32 [N][7] (xyz + xyzw quaternion; all NaN on creation: nothing equals it), the solution f32 [N][7]
// of that request (the reference's last_ik), its residual [N], the `solved` bytes of the last call and a list of the envs that need a solve.
//
// k_cart_decide.  k_macro_decide's scheme on seven floats: one workgroup of MD_THREADS walks the envs in strides of MD_THREADS, MD_ROUND
// strides between two barriers.  Per env: idle -> nothing; otherwise same = the seven request floats == the record (IEEE ==: -0.0
// equals 0.0, a NaN equals nothing), need = !same; a needing env gets the request into its record.  The needing envs go into the list in
// ASCENDING env index: a wave's ballot gives a lane its place among its wave's needing lanes, the waves' counts go through LDS, and a
// running offset carries from stride to stride.  No atomics; the order places work and decides no result (every listed env's solution
// is a function of its own joints and request alone).
//
// k_cart_solve.  Solves the listed envs: k_ik's joints and residual, bit for bit, from the same ik_fk / ik_dls and ik_solve's
// selection rule with no predecessor.  The grid is sized from N -- min(N, max(CS_WAVES, ceil(N / CS_SLOTS))) workgroups, all the list
// can need under the slot rule below -- because the list's length stays on the device; a workgroup beyond the list leaves at once.
//   Seeds across lanes.  A workgroup is one wave; a listed env owns a SLOT of two neighbouring lanes, lane s of the slot runs seed s
//   of ik_solve (present joints, elbow-up): ik_solve's loop body, one iteration per lane.  Each leaves {converged, key, residual,
//   q[7]} in LDS and lane 0 of the slot then applies ik_solve's `better` rule to them in seed order: the first seed stands, a
//   converged second seed beats an unconverged first, equal convergence is decided by a strictly greater elbow height.  The winner's
//   joints and residual are stored.  Under ik_single_seed only lane 0 of a slot works.
//   The chain is latency-bound and a wave runs as long as its slowest lane: two seeds side by side halve the per-lane chain, where
//   4096 envs one per lane would fill a fraction of the device with waves twice as long.
//   Slots per wave.  E = min(32, ceil(count / CS_WAVES)) listed envs share a wave: up to CS_WAVES needing envs every env has a wave
//   of its own (no env waits for another env's longer solve), beyond that the waves fill up instead of queueing (beyond CS_WAVES *
//   CS_SLOTS all 32 slots are in use and the grid grows).  E is read from the list's length by every wave alike and changes no result.
// The one barrier stands behind the solves, where every lane of the wave arrives.
//
// k_cart_fetch.  Over all N: the command row [solution[0..6], gripper[0], gripper[1]] into D.cmd, zeros(9) for an idle env.
// k_cart_invalidate.  NaN into the masked record rows.
#define CS_SLOTS 32          // slots of two lanes in a wave
#define CS_WAVES 1024        // the needing envs up to which every env gets a wave of its own (the SIMDs of an MI355X)

__global__ void __launch_bounds__(MD_THREADS) k_cart_decide(int N, const float *__restrict__ cart /*[N][7]*/, const unsigned char *__restrict__ idle /*[N] or nullptr*/,
                                                            float *__restrict__ req /*[N][7]*/, unsigned char *__restrict__ solved /*[N]*/,
                                                            int *__restrict__ list /*[N + 1]: the envs, ascending; [N] their number*/) {
    __shared__ int wcount[MD_ROUND][MD_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0;
    for (int base = 0; base < N; base += MD_ROUND * MD_THREADS) {
        // the round's loads first (scalar loads: a caller's tensor need not be 16-byte aligned), then the decisions and their stores
        float c[MD_ROUND][7], r[MD_ROUND][7];
        bool act[MD_ROUND], need[MD_ROUND];
        unsigned long long bal[MD_ROUND];
#pragma unroll
        for (int i = 0; i < MD_ROUND; i++) {
            const int env = base + i * MD_THREADS + tid;
            act[i] = env < N && !(idle && idle[env]);
            const size_t at = act[i] ? (size_t)env : 0;
#pragma unroll
            for (int k = 0; k < 7; k++) { c[i][k] = cart[at * 7 + k]; r[i][k] = req[at * 7 + k]; }
        }
#pragma unroll
        for (int i = 0; i < MD_ROUND; i++) {
            const int env = base + i * MD_THREADS + tid;
            bool same = true;
#pragma unroll
            for (int k = 0; k < 7; k++) same = same && c[i][k] == r[i][k];
            need[i] = act[i] && !same;
            if (need[i]) {
#pragma unroll
                for (int k = 0; k < 7; k++) req[(size_t)env * 7 + k] = c[i][k];
            }
            if (env < N) solved[env] = need[i] ? 1 : 0;
            bal[i] = __ballot(need[i]);
            if (lane == 0) wcount[i][wave] = __popcll(bal[i]);
        }
        __syncthreads();
        int before[MD_ROUND], acc = 0;
#pragma unroll
        for (int i = 0; i < MD_ROUND; i++) {
            before[i] = 0;
            for (int w = 0; w < MD_THREADS / 64; w++) { if (w == wave) before[i] = acc; acc += wcount[i][w]; }
        }
#pragma unroll
        for (int i = 0; i < MD_ROUND; i++)
            if (need[i]) list[running + before[i] + __popcll(bal[i] & ((1ull << lane) - 1ull))] = base + i * MD_THREADS + tid;
        running += acc;
        __syncthreads();
    }
    if (tid == 0) list[N] = running;
}

// NaN into the record rows of the masked envs (nullptr: all): nothing equals them, the next non-idle rr_step_cartesian solves those envs
__global__ void __launch_bounds__(256) k_cart_invalidate(int N, const unsigned char *__restrict__ mask, float *__restrict__ req /*[N][7]*/) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N * 7) return;
    if (mask && !mask[i / 7]) return;
    req[i] = __int_as_float(0x7fc00000);
}

__global__ void __launch_bounds__(64) k_cart_solve(IkModel M, SimParams P, DevPtrs D, const float *__restrict__ req /*[N][7]*/, const int *__restrict__ list /*[N + 1]*/,
                                                   float *__restrict__ sol /*[N][7]*/, float *__restrict__ res /*[N]*/) {
    const int N = P.N;
    const int count = min(list[N], N);           // (clamped, as the env index below: no value of the list forms an address unchecked)
    const int E = min(CS_SLOTS, max(1, (count + CS_WAVES - 1) / CS_WAVES));
    __shared__ float s_res[CS_SLOTS][2][10];     // per slot and seed: converged, key, residual, q[7]
    const int lane = threadIdx.x, slot = lane >> 1, seed = lane & 1;
    const int first = (int)blockIdx.x * E;
    if (first >= count) return;
    const bool live = slot < E && first + slot < count;
    const int env = live ? min(max(list[first + slot], 0), N - 1) : 0;
    const int nseeds = M.single_seed ? 1 : 2;
    if (live && seed < nseeds) {
        const float *state = D.state;
        const float *t = req + (size_t)env * 7;
        const m3 Rt = quat_target(t + 3);
        const float elbow_up[7] = {0.0f, 0.6f, 0.0f, -1.3f, 0.0f, 1.2f, 0.0f};
        // one iteration of ik_solve's loop: seed `seed`, no predecessor (the key is the elbow height)
        float q[7];
#pragma unroll
        for (int k = 0; k < 7; k++) q[k] = seed == 0 ? STT(ST_Q + k) : elbow_up[k];
        const float err = ik_dls(M, q, mk(t[0], t[1], t[2]), Rt, 1000);
        v3 p[7], ax[7], pe; m3 Re; float ez;
        ik_fk(M, q, p, ax, Re, pe, ez);
        s_res[slot][seed][0] = err < 1e-2f ? 1.0f : 0.0f;
        s_res[slot][seed][1] = ez;
        s_res[slot][seed][2] = err;
#pragma unroll
        for (int k = 0; k < 7; k++) s_res[slot][seed][3 + k] = q[k];
    }
    __syncthreads();
    if (live && seed == 0) {
        // ik_solve's `better`, applied in seed order
        int best = 0;
        if (nseeds > 1) {
            const bool conv0 = s_res[slot][0][0] != 0.0f, conv1 = s_res[slot][1][0] != 0.0f;
            const bool better = (conv1 && !conv0) || (conv1 == conv0 && s_res[slot][1][1] > s_res[slot][0][1]);
            if (better) best = 1;
        }
#pragma unroll
        for (int k = 0; k < 7; k++) sol[(size_t)env * 7 + k] = s_res[slot][best][3 + k];
        res[env] = s_res[slot][best][2];
    }
}

// command of this step = [solution[0..6], gripper[0], gripper[1]] (env.py:380-381); an idle env takes zeros(9) (env.py:359-361)
__global__ void __launch_bounds__(256) k_cart_fetch(SimParams P, DevPtrs D, const float *__restrict__ sol /*[N][7]*/, const float *__restrict__ gripper /*[N][2]*/,
                                                    const unsigned char *__restrict__ idle) {
    const int N = P.N;
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    float *c = D.cmd + (size_t)env * 9;
    if (idle && idle[env]) {
        for (int k = 0; k < 9; k++) c[k] = 0.0f;
        return;
    }
    for (int k = 0; k < 7; k++) c[k] = sol[(size_t)env * 7 + k];
    c[7] = gripper[(size_t)env * 2];
    c[8] = gripper[(size_t)env * 2 + 1];
}
