// rr_state.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// reset / state io / observation kernels, render set-up
// ---------------------------------------------------------------------------------------------- reset / state io
// what a reset does for one env (k_reset, and the auto-reset of k_episode in rr_episode.inc)
__device__ __forceinline__ void reset_env(const DevPtrs &D, int N, int env) {
    float *state = D.state;
    for (int i = 0; i < ST_TOTAL; i++) STT(i) = 0;
    for (int i = 0; i < NOBJ; i++) {
        for (int k = 0; k < 3; k++) STT(ST_OPOS + 3 * i + k) = D.obj_home[(size_t)(7 * i + k) * N + env];
        for (int k = 0; k < 4; k++) STT(ST_OQUAT + 4 * i + k) = D.obj_home[(size_t)(7 * i + 3 + k) * N + env];
    }
    D.timestep[env] = 0;
    D.errflags[env] = 0;
    for (int k = 0; k < 4; k++) D.touch[(size_t)env * 4 + k] = 0;
    D.ccount[env] = 0;
    D.ccount_pub[env] = 0; D.class_pub[env] = 0;
}

__global__ void k_reset(BodyParams B, SimParams P, DevPtrs D, const unsigned char *mask) {
    const int N = P.N;
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    if (mask && !mask[env]) return;
    reset_env(D, N, env);
}

__global__ void k_state_io(SimParams P, DevPtrs D, float *aos /*[N][61]*/, int to_aos) {
    const int N = P.N;
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    float *state = D.state;
    // AoS order (same as the oracle's 61-vector): q[11] qd[11] then per object pos3 quat4 lin3 ang3
    float *a = aos + (size_t)env * NSTATE;
    for (int i = 0; i < 22; i++) {
        if (to_aos) a[i] = STT(i); else STT(i) = a[i];
    }
    for (int o = 0; o < NOBJ; o++) {
        float *b = a + 22 + 13 * o;
        for (int k = 0; k < 3; k++) {
            if (to_aos) { b[k] = STT(ST_OPOS + 3 * o + k); b[7 + k] = STT(ST_OVEL + 3 * o + k); b[10 + k] = STT(ST_OANG + 3 * o + k); }
            else { STT(ST_OPOS + 3 * o + k) = b[k]; STT(ST_OVEL + 3 * o + k) = b[7 + k]; STT(ST_OANG + 3 * o + k) = b[10 + k]; }
        }
        for (int k = 0; k < 4; k++) {
            if (to_aos) b[3 + k] = STT(ST_OQUAT + 4 * o + k); else STT(ST_OQUAT + 4 * o + k) = b[3 + k];
        }
    }
    if (!to_aos) {
        // a restored state is a fresh start for everything derived from the previous step: the NaN guard's freeze bit, the
        // contact list behind rr_get_contacts and the touch sensors (as k_reset does)
        D.errflags[env] = 0;
        for (int k = 0; k < 4; k++) D.touch[(size_t)env * 4 + k] = 0;
        D.ccount[env] = 0;
        D.ccount_pub[env] = 0; D.class_pub[env] = 0;
    }
}

// object i of one env to the pose p7 (xyz + xyzw quaternion), at rest (k_set_object_poses, and the start poses of k_episode)
__device__ __forceinline__ void set_object_pose_env(float *state, int N, int env, int i, const float *p7) {
    for (int k = 0; k < 3; k++) { STT(ST_OPOS + 3 * i + k) = p7[k]; STT(ST_OVEL + 3 * i + k) = 0; STT(ST_OANG + 3 * i + k) = 0; }
    for (int k = 0; k < 4; k++) STT(ST_OQUAT + 4 * i + k) = p7[3 + k];
}

// rr_set_object_poses: poses [N][nobj][7] for the envs whose mask byte is set (nullptr: all); zeroes the velocities like
// BodyPart.reset_pose -> resetBasePositionAndOrientation (env.py:159-162)
__global__ void k_set_object_poses(SimParams P, DevPtrs D, const float *poses, const unsigned char *mask) {
    const int N = P.N;
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    if (mask && !mask[env]) return;
    for (int i = 0; i < P.nobj; i++) set_object_pose_env(D.state, N, env, i, poses + ((size_t)env * P.nobj + i) * 7);
}

// REALRobotEnv.evaluateGoal (env.py:181-200) for one env: sum over the goal's objects of exp(-(ln 4 / 0.10) |p_goal - p|).  The ONE
// place with the score's arithmetic: k_goal_score (rr_evaluate_goals) and k_episode (rr_episode_update) both call it, so the two
// agree bit for bit.  goal_pos: the env's rows [nobj][3]; object i counts when goal_mask is nullptr or goal_mask[i] & bits.
__device__ __forceinline__ float goal_score_env(const float *state, int N, int env, int nobj, const float *goal_pos, const unsigned char *goal_mask, unsigned bits) {
    const float pos_const = 13.862943611198906f;        // -log(0.25) / 0.10: the score falls to 0.25 within 10 cm
    float sc = 0.0f;
    for (int i = 0; i < nobj; i++) {
        if (goal_mask && !(goal_mask[i] & bits)) continue;
        const float *g = goal_pos + 3 * i;
        const float dx = g[0] - STT(ST_OPOS + 3 * i), dy = g[1] - STT(ST_OPOS + 3 * i + 1), dz = g[2] - STT(ST_OPOS + 3 * i + 2);
        sc += expf(-pos_const * sqrtf(dx * dx + dy * dy + dz * dz));
    }
    return sc;
}

__global__ void k_goal_score(SimParams P, DevPtrs D, const float *goal_pos /*[N][nobj][3]*/, const unsigned char *goal_mask /*[N][nobj] or nullptr*/, float *score) {
    const int N = P.N;
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    score[env] = goal_score_env(D.state, N, env, P.nobj, goal_pos + (size_t)env * P.nobj * 3, goal_mask ? goal_mask + (size_t)env * P.nobj : nullptr, 0xffu);
}

// ---------------------------------------------------------------------------------------------- render setup
__global__ void __launch_bounds__(64) k_render_setup(BodyParams B, SimParams P, const RenderModel *RMp, DevPtrs D, int sel) {
    const RenderModel &RM = *RMp;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int env = gid >> 5, i = gid & (MAXINST - 1);
    static_assert(MAXINST == 32, "thread -> (env, instance) mapping");
    if (env >= P.N || i >= RM.ni || !env_selected(D.hgflag, env, sel)) return;
    instance_setup(B, P, RM, D, env, i);
}

// link poses (COM frame) for rr_link_poses
__global__ void __launch_bounds__(64) k_link_poses(BodyParams B, SimParams P, const RenderModel *RMp, DevPtrs D, float *out /*[N][nl][7]*/) {
    const RenderModel &RM = *RMp;
    const int N = P.N;
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= N) return;
    const float *state = D.state;
    float q[NB];
#pragma unroll
    for (int i = 0; i < NB; i++) q[i] = STT(ST_Q + i);
    m3 bR[NB]; v3 bp[NB], bax[NB];
    fk_all(B, q, bR, bp, bax);
    for (int l = 0; l < RM.nl; l++) {
        int b = RM.link_body[l];
        m3 lr;
        for (int k = 0; k < 9; k++) lr.m[k] = RM.link_rot[l][k];
        v3 lp = mk(RM.link_pos[l][0], RM.link_pos[l][1], RM.link_pos[l][2]);
        m3 R = lr;
        v3 p = mk(B.robot_pos[0], B.robot_pos[1], B.robot_pos[2]) + lp;
        if (b >= 0) {
            m3 Rb = bR[0]; v3 pb = bp[0];
#pragma unroll
            for (int bb = 0; bb < NB; bb++) if (bb == b) { Rb = bR[bb]; pb = bp[bb]; }
            R = mul(Rb, lr);
            p = mulv(Rb, lp) + pb;
        }
        float qq[4];
        m3_to_quat(R, qq);
        float *o = out + ((size_t)env * RM.nl + l) * 7;
        o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = qq[0]; o[4] = qq[1]; o[5] = qq[2]; o[6] = qq[3];
    }
}
