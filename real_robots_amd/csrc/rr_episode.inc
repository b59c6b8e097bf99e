// rr_episode.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// k_episode / k_env_goals / k_goal_image: the goal table and the per-env episode record on the device (rr_set_goals,
// rr_set_env_goals, rr_episode_update; realrobot.h).  What REALRobotEnv.set_goal, evaluateGoal and the end of step_joints do on the
// host for one env (env.py:151-166, 181-200, 345-352) for every env of the batch in one launch per step: score, reward, done bits
// and, on request, the reset of the finished envs into their next goal.
//
// The table and the record are kernel arguments of THESE kernels only (GoalTable, EpisodeRec): DevPtrs, SimParams and BodyParams are
// arguments of every kernel of the step, whose code must not depend on this part.  None of these kernels is launched by a step.
//
// k_episode, k_env_goals: one thread per env; the state slab is [slot][N], so consecutive lanes read consecutive words (as k_reset).
// k_goal_image: the only part with bandwidth -- up to H W 3 bytes per env whose goal changed.  RR_EP_GOAL_RGB is persistent: the
// producer kernel (k_episode or k_env_goals) writes one "goal changed" byte for EVERY env, and every workgroup of the (env, chunk)
// grid reads its env's byte first (a uniform load) and leaves when it is clear.  The copy moves 16 bytes per lane when H W 3 is a
// multiple of 16 (rows of the table and of the buffer are then 16-byte aligned), 4 bytes per lane otherwise (W is a multiple of 4,
// so H W 3 always is one of 4): lane i at base + i * width, four accesses in flight per lane.

struct GoalTable {
    const float *start;          // [G][nobj][7] start poses (read where flag bit 1 is set)
    const float *final_pos;      // [G][nobj][3] goal positions (read where flag bit 0 is set)
    const unsigned char *flags;  // [G][nobj] bit 0: the object counts in the score, bit 1: it has a start pose
    int G;
};
struct EpisodeRec {
    float *score, *reward, *prev;   // [N]; prev: the score the next reward is taken against
    unsigned *done;                 // [N] bit 0 truncated, bit 1 frozen
    int *goal_index, *episode;      // [N]
    float *final_obs;               // [N][9 + 4 + 7 nobj + 1]
    float *goal_pos;                // [N][nobj][3]
    unsigned char *changed;         // [N] the env's goal changed in the last k_episode / k_env_goals launch (k_goal_image reads it)
};

__device__ __forceinline__ float episode_score(const float *state, int N, int env, int nobj, const GoalTable &T, int gi) {
    if (gi < 0 || gi >= T.G) return 0.0f;
    return goal_score_env(state, N, env, nobj, T.final_pos + (size_t)gi * nobj * 3, T.flags + (size_t)gi * nobj, 1u);
}
// RR_EP_GOAL_POS of one env: the goal's position where the goal names the object, NaN elsewhere (and everywhere without a goal)
__device__ __forceinline__ void episode_goal_pos(const EpisodeRec &E, int env, int nobj, const GoalTable &T, int gi) {
    const float nan = __int_as_float(0x7fc00000);
    const bool has = gi >= 0 && gi < T.G;
    for (int i = 0; i < nobj; i++) {
        const bool named = has && (T.flags[(size_t)gi * nobj + i] & 1u);
        for (int k = 0; k < 3; k++) E.goal_pos[((size_t)env * nobj + i) * 3 + k] = named ? T.final_pos[((size_t)gi * nobj + i) * 3 + k] : nan;
    }
}

// rr_episode_update.  stride: the goal stride already reduced to [0, G).
__global__ void __launch_bounds__(256) k_episode(SimParams P, DevPtrs D, GoalTable T, EpisodeRec E, int horizon, int stride, int reset_done) {
    const int N = P.N;
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    float *state = D.state;
    int gi = E.goal_index[env];
    const float score = episode_score(state, N, env, P.nobj, T, gi);
    E.score[env] = score;
    E.reward[env] = score - E.prev[env];
    float prev = score;
    const unsigned done = ((horizon > 0 && D.timestep[env] >= horizon) ? 1u : 0u) | ((D.errflags[env] & 5u) ? 2u : 0u);
    E.done[env] = done;
    unsigned char changed = 0;
    if (reset_done && done) {
        // 1. the last observation of the finished episode, as the step left it
        const int F = 13 + 7 * P.nobj + 1;
        float *fo = E.final_obs + (size_t)env * F;
        for (int k = 0; k < 9; k++) fo[k] = D.joints[(size_t)env * 9 + k];
        for (int k = 0; k < 4; k++) fo[9 + k] = D.touch[(size_t)env * 4 + k];
        for (int k = 0; k < 7 * P.nobj; k++) fo[13 + k] = D.objpose[(size_t)env * P.nobj * 7 + k];
        fo[13 + 7 * P.nobj] = score;
        // 2. rr_reset of this env
        reset_env(D, N, env);
        // 3. the next goal (no goal stays no goal)
        if (gi >= 0 && gi < T.G) {
            const int old = gi;
            gi += stride;
            if (gi >= T.G) gi -= T.G;
            changed = gi != old;
            E.goal_index[env] = gi;
            // 4. its start poses (rr_set_object_poses); an object without one keeps its home pose
            for (int i = 0; i < P.nobj; i++)
                if (T.flags[(size_t)gi * P.nobj + i] & 2u) set_object_pose_env(state, N, env, i, T.start + ((size_t)gi * P.nobj + i) * 7);
            // 5. (the image follows in k_goal_image)
            if (changed) episode_goal_pos(E, env, P.nobj, T, gi);
        }
        // 6. the next reward is taken against the score of the start state
        prev = episode_score(state, N, env, P.nobj, T, gi);
        E.episode[env] += 1;
    }
    E.prev[env] = prev;
    E.changed[env] = changed;
}

// rr_set_env_goals: the masked envs (nullptr: all) take index[env]; their previous score becomes the score of the state as it is
__global__ void __launch_bounds__(256) k_env_goals(SimParams P, DevPtrs D, GoalTable T, EpisodeRec E, const int *index /*[N], nullptr: -1 for all*/, const unsigned char *mask) {
    const int N = P.N;
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    if (mask && !mask[env]) { E.changed[env] = 0; return; }
    const int gi = index ? index[env] : -1;
    E.goal_index[env] = gi;
    episode_goal_pos(E, env, P.nobj, T, gi);
    E.prev[env] = episode_score(D.state, N, env, P.nobj, T, gi);
    E.changed[env] = 1;
}

#define GI_THREADS 256
#define GI_PER_THREAD 4
#define GI_CHUNK (GI_THREADS * GI_PER_THREAD)      // units of U per workgroup
// units: U per env (H W 3 / sizeof(U)); chunks = ceil(units / GI_CHUNK); grid = N * chunks.  table: [G][units] or nullptr (G 0).
template <typename U>
__global__ void __launch_bounds__(GI_THREADS) k_goal_image(int N, int G, unsigned units, unsigned chunks, const int *__restrict__ goal_index,
                                                           const unsigned char *__restrict__ changed, const U *__restrict__ table, U *__restrict__ out) {
    const unsigned env = blockIdx.x / chunks, chunk = blockIdx.x - env * chunks;
    if (env >= (unsigned)N || !changed[env]) return;
    const int gi = goal_index[env];
    const bool has = gi >= 0 && gi < G;
    const U *src = table + (size_t)(has ? gi : 0) * units;
    U *dst = out + (size_t)env * units;
    const unsigned base = chunk * GI_CHUNK + threadIdx.x;
    U v[GI_PER_THREAD];
#pragma unroll
    for (int k = 0; k < GI_PER_THREAD; k++) {
        const unsigned u = base + k * GI_THREADS;
        v[k] = U{};
        if (has && u < units) v[k] = src[u];
    }
#pragma unroll
    for (int k = 0; k < GI_PER_THREAD; k++) {
        const unsigned u = base + k * GI_THREADS;
        if (u < units) dst[u] = v[k];
    }
}
