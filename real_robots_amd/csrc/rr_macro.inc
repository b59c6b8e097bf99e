// rr_macro.inc -- part of realrobot.hip (included there, behind rr_ik.inc; not a stand-alone translation unit).
// Device-resident macro actions (rr_step_macro, realrobot.h): the deciding half of REALRobotEnv.step_macro (env.py:388-408) and a
// planner shaped for the list that decision produces.  The handle holds, next to the plan [N][1000][9] and the plan positions [N] of
// rr_plan_macro, a request record f32 [N][4] (all NaN on creation: nothing equals it), a list of the envs that need a plan and the
// `replanned` bytes of the last call.
//
// k_macro_decide.  One workgroup of MD_THREADS walks the envs in strides of MD_THREADS, MD_ROUND strides between two barriers.  Per env: idle -> nothing; otherwise
// same = the four request floats == the record (IEEE ==: -0.0 equals 0.0, a NaN equals nothing), need = !same || position >= 1000;
// a needing env gets the request into its record and position 0.  The needing envs go into the list in ASCENDING env index: a
// wave's ballot gives a lane its place among its wave's needing lanes, the waves' counts go through LDS, and a running offset carries
// from stride to stride.  No atomics; the order places work and decides no result (every listed env's plan is a function of its own
// joints and request alone).
//
// k_macro_replan.  Plans the listed envs: k_plan_macro's rows, bit for bit, from the same ik_fk / ik_dls and ik_solve's selection rule.
// The grid is sized from N -- min(N, max(MR_WAVES, ceil(N / MR_SLOTS))) workgroups, all the list can need under the slot rule below --
// because the list's length stays on the device; a workgroup beyond the list leaves at once.
//   Seeds across lanes.  A workgroup is one wave; a listed env owns a SLOT of four neighbouring lanes, lane s < 3 of the slot runs
//   seed s of ik_solve (present joints, elbow-up, previous way-point) of the env's current way-point, lane 3 only stores rows.  The
//   three runs are ik_solve's loop body, one iteration per lane; each leaves {converged, key, q[7]} in LDS and every lane of the slot
//   then applies ik_solve's `better` rule to them in seed order 0, 1, 2: the first seed always stands, a converged seed beats an
//   unconverged one, equal convergence is decided by a strictly greater key.  The first way-point has two seeds (no predecessor: the
//   key is the elbow height), ik_single_seed one.  The way-points stay sequential, each prefers its predecessor.
//   Slots per wave.  E = min(16, ceil(count / MR_WAVES)) listed envs share a wave: up to MR_WAVES needing envs every env has a wave
//   of its own (no env waits for another env's longer solve), beyond that the waves fill up instead of queueing (beyond MR_WAVES *
//   MR_SLOTS all sixteen slots are in use and the grid grows).  E is read from the list's length by every wave alike and changes no result.
//   Rows written once, by the wave.  A row's final value in k_plan_macro is the LAST way-point whose fill range covers it: sweep
//   piece i owns rows [250 + i chunk, 250 + (i + 1) chunk), the last piece up to 750.  After a way-point's winner is known, all 64
//   lanes store its rows -- (r1 - r0) * 9 consecutive floats per slot -- coalesced; nothing is stored twice.
// The way-point loop runs to the largest trip count among the wave's slots with the shorter slots masked, so that the barriers stand
// at wave-uniform points.
#define MD_THREADS 1024
#define MD_ROUND 4           // strides of MD_THREADS envs between two barriers: 4096 envs are one round
#define MR_SLOTS 16          // slots of four lanes in a wave
#define MR_WAVES 1024        // the needing envs up to which every env gets a wave of its own (the SIMDs of an MI355X)

__global__ void __launch_bounds__(MD_THREADS) k_macro_decide(int N, const float *__restrict__ macro /*[N][4]*/, const unsigned char *__restrict__ idle /*[N] or nullptr*/,
                                                             float *__restrict__ req /*[N][4]*/, int *__restrict__ plan_step /*[N]*/,
                                                             unsigned char *__restrict__ replanned /*[N]*/, int *__restrict__ list /*[N + 1]: the envs, ascending; [N] their number*/) {
    __shared__ int wcount[MD_ROUND][MD_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0;
    for (int base = 0; base < N; base += MD_ROUND * MD_THREADS) {
        // the round's loads first (scalar loads: a caller's tensor need not be 16-byte aligned), then the decisions and their stores
        float m[MD_ROUND][4], r[MD_ROUND][4];
        int pos[MD_ROUND];
        bool act[MD_ROUND], need[MD_ROUND];
        unsigned long long bal[MD_ROUND];
#pragma unroll
        for (int i = 0; i < MD_ROUND; i++) {
            const int env = base + i * MD_THREADS + tid;
            act[i] = env < N && !(idle && idle[env]);
            const size_t at = act[i] ? (size_t)env : 0;
#pragma unroll
            for (int k = 0; k < 4; k++) { m[i][k] = macro[at * 4 + k]; r[i][k] = req[at * 4 + k]; }
            pos[i] = plan_step[at];
        }
#pragma unroll
        for (int i = 0; i < MD_ROUND; i++) {
            const int env = base + i * MD_THREADS + tid;
            const bool same = m[i][0] == r[i][0] && m[i][1] == r[i][1] && m[i][2] == r[i][2] && m[i][3] == r[i][3];
            need[i] = act[i] && (!same || pos[i] >= PLAN_LEN);
            if (need[i]) {
#pragma unroll
                for (int k = 0; k < 4; k++) req[(size_t)env * 4 + k] = m[i][k];
                plan_step[env] = 0;
            }
            if (env < N) replanned[env] = need[i] ? 1 : 0;
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

// NaN into the record rows of the masked envs (nullptr: all): nothing equals them, the next non-idle rr_step_macro plans those envs
__global__ void __launch_bounds__(256) k_macro_invalidate(int N, const unsigned char *__restrict__ mask, float *__restrict__ req /*[N][4]*/) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N * 4) return;
    if (mask && !mask[i >> 2]) return;
    req[i] = __int_as_float(0x7fc00000);
}

__global__ void __launch_bounds__(64) k_macro_replan(IkModel M, SimParams P, DevPtrs D, const float *__restrict__ macro /*[N][4]*/, const int *__restrict__ list /*[N + 1]*/,
                                                     float *__restrict__ plan /*[N][1000][9]*/) {
    const int N = P.N;
    const int count = list[N];
    const int E = min(MR_SLOTS, max(1, (count + MR_WAVES - 1) / MR_WAVES));
    __shared__ float s_res[MR_SLOTS][3][9];      // per slot and seed: converged, key, q[7]
    __shared__ float s_row[MR_SLOTS][9];         // per slot: the row of the way-point just decided
    __shared__ int s_range[MR_SLOTS][3];         // per slot: its rows [r0, r1) and the env
    __shared__ int s_trips[MR_SLOTS];
    const int lane = threadIdx.x, slot = lane >> 2, seed = lane & 3;
    const int first = (int)blockIdx.x * E;
    if (first >= count) return;
    const bool live = slot < E && first + slot < count;
    const int env = live ? list[first + slot] : 0;
    const float *state = D.state;
    float qc[7], last[7];
#pragma unroll
    for (int k = 0; k < 7; k++) { qc[k] = STT(ST_Q + k); last[k] = 0.0f; }
    const float f7 = STT(ST_Q + 7), f8 = STT(ST_Q + 8);       // env.py:427: first 9 of the 11 dofs
    const float p1x = macro[(size_t)env * 4], p1y = macro[(size_t)env * 4 + 1], p2x = macro[(size_t)env * 4 + 2], p2y = macro[(size_t)env * 4 + 3];
    // getQuaternionFromEuler([0, 3.14, -1.57])  (env.py:422), as k_plan_macro
    float cr = 1.0f, sr = 0.0f, sp, cp, sy, cy;
    sincosf(3.14f * 0.5f, &sp, &cp);
    sincosf(-1.57f * 0.5f, &sy, &cy);
    float qt[4] = {sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy};
    m3 Rt = quat_target(qt);
    // interpolate3D(p1, p2, 500) (env.py:430-441), as k_plan_macro
    float dx = p2x - p1x, dy = p2y - p1y;
    float dist = sqrtf(dx * dx + dy * dy);
    int pieces = (int)(dist / 0.05f) + 1;
    if (pieces > 500) pieces = 500;
    const int npc = pieces > 0 ? pieces : 0;                  // (a request that is not finite can leave no piece: rows 250..749 keep their bytes, as in k_plan_macro)
    const int chunk = npc > 0 ? 500 / npc : 500;
    // way-point w of a slot: 0 above p1, 1 at p1, 2 + i sweep piece i, 2 + npc above p2
    if (seed == 0) { s_trips[slot] = live ? 3 + npc : 0; s_range[slot][2] = live ? env : -1; }
    __syncthreads();
    int trips = 0;
    for (int s = 0; s < E; s++) trips = max(trips, s_trips[s]);
    // the rows that hold no IK result: 0..99 and 800..899 home2, 900..999 home
    for (int s = 0; s < E; s++) {
        const int en = s_range[s][2];
        if (en < 0) continue;
        float *pl = plan + (size_t)en * PLAN_LEN * 9;
        for (int i = lane; i < 300 * 9; i += 64) {
            const int r = i / 9, k = i - r * 9;
            const int row = r < 100 ? r : 700 + r;
            pl[row * 9 + k] = (row < 900 && (k == 5 || k == 6)) ? 1.57079632679f : 0.0f;
        }
    }
    const float elbow_up[7] = {0.0f, 0.6f, 0.0f, -1.3f, 0.0f, 1.2f, 0.0f};
    const int nseeds = M.single_seed ? 1 : 3;
    for (int w = 0; w < trips; w++) {
        const bool on = live && w < 3 + npc;
        const bool prefer = w > 0;
        if (on && seed < (prefer ? nseeds : min(nseeds, 2))) {
            v3 tp;
            if (w == 0) tp = mk(p1x, p1y, 0.6f);
            else if (w == 1) tp = mk(p1x, p1y, 0.46f);
            else if (w < 2 + npc) { const float f = (float)(w - 1) / (float)pieces; tp = mk(p1x + dx * f, p1y + dy * f, 0.46f); }
            else tp = mk(p2x, p2y, 0.6f);
            // one iteration of ik_solve's loop: seed `seed`
            float q[7];
#pragma unroll
            for (int k = 0; k < 7; k++) q[k] = seed == 0 ? qc[k] : (seed == 1 ? elbow_up[k] : last[k]);
            float err = ik_dls(M, q, tp, Rt, 1000);
            bool conv = err < 1e-2f;
            float key;
            if (prefer) {
                float mxd = 0;
#pragma unroll
                for (int k = 0; k < 7; k++) mxd = fmaxf(mxd, fabsf(q[k] - last[k]));
                key = -mxd;
            } else {
                v3 p[7], ax[7], pe; m3 Re; float ez;
                ik_fk(M, q, p, ax, Re, pe, ez);
                key = ez;
            }
            s_res[slot][seed][0] = conv ? 1.0f : 0.0f;
            s_res[slot][seed][1] = key;
#pragma unroll
            for (int k = 0; k < 7; k++) s_res[slot][seed][2 + k] = q[k];
        }
        __syncthreads();
        if (on) {
            // ik_solve's `better`, applied in seed order
            const int ns = prefer ? nseeds : min(nseeds, 2);
            int best = 0;
            bool best_conv = s_res[slot][0][0] != 0.0f;
            float best_key = s_res[slot][0][1];
            for (int s = 1; s < ns; s++) {
                const bool conv = s_res[slot][s][0] != 0.0f;
                const float key = s_res[slot][s][1];
                const bool better = (conv && !best_conv) || (conv == best_conv && key > best_key);
                if (better) { best = s; best_conv = conv; best_key = key; }
            }
#pragma unroll
            for (int k = 0; k < 7; k++) last[k] = s_res[slot][best][2 + k];
        }
        if (seed == 0) {
            int r0 = 0, r1 = 0;
            if (on) {
                if (w == 0) { r0 = 100; r1 = 200; }
                else if (w == 1) { r0 = 200; r1 = 250; }
                else if (w < 2 + npc) { r0 = 250 + (w - 2) * chunk; r1 = w == 1 + npc ? 750 : r0 + chunk; }
                else { r0 = 750; r1 = 800; }
#pragma unroll
                for (int k = 0; k < 7; k++) s_row[slot][k] = last[k];
                s_row[slot][7] = f7; s_row[slot][8] = f8;
            }
            s_range[slot][0] = r0; s_range[slot][1] = r1;
        }
        __syncthreads();
        for (int s = 0; s < E; s++) {
            const int r0 = s_range[s][0], n = (s_range[s][1] - r0) * 9, en = s_range[s][2];
            if (n <= 0 || en < 0) continue;
            float *pl = plan + ((size_t)en * PLAN_LEN + r0) * 9;
            for (int i = lane; i < n; i += 64) pl[i] = s_row[s][i % 9];
        }
    }
}
