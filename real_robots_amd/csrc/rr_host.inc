// rr_host.inc -- part of realrobot.hip (included there, in this order; not a stand-alone translation unit).
// host side: model blob, rr_env, the C ABI
// ---------------------------------------------------------------------------------------------- host side
struct BlobEntry {
    char name[32];
    uint32_t dtype, ndim, shape[4];
    uint64_t offset, nbytes;
};

struct Blob {
    const char *base; size_t size; uint32_t n; const BlobEntry *e;
    bool init(const void *p, size_t sz) {
        base = (const char *)p; size = sz;
        if (sz < 16 || memcmp(base, "RRMODEL1", 8) != 0) return false;
        memcpy(&n, base + 8, 4);
        if (16 + (size_t)n * sizeof(BlobEntry) > sz) return false;
        e = (const BlobEntry *)(base + 16);
        for (uint32_t i = 0; i < n; i++) if (e[i].offset + e[i].nbytes > sz) return false;
        return true;
    }
    const BlobEntry *find(const char *name, uint32_t dtype) const {
        for (uint32_t i = 0; i < n; i++) if (strncmp(e[i].name, name, 32) == 0 && e[i].dtype == dtype) return &e[i];
        return nullptr;
    }
    const float *f32(const char *name, size_t min_count = 0) const {
        const BlobEntry *x = find(name, 0);
        if (!x || x->nbytes < min_count * 4) return nullptr;
        return (const float *)(base + x->offset);
    }
    const int32_t *i32(const char *name, size_t min_count = 0) const {
        const BlobEntry *x = find(name, 1);
        if (!x || x->nbytes < min_count * 4) return nullptr;
        return (const int32_t *)(base + x->offset);
    }
    const uint8_t *u8(const char *name, size_t *nbytes) const {
        const BlobEntry *x = find(name, 2);
        if (!x) return nullptr;
        *nbytes = x->nbytes;
        return (const uint8_t *)(base + x->offset);
    }
};

// Every RR_* environment variable of the library (INTEGRATION.md has the table): read_settings() is the one place that reads
// them, once at the top of rr_create; the rest of the code reads these members.  None is needed in production.
#define RUN_AHEAD_MAX 64
struct Settings {
    int tile_w = 0;                // the tile width asked for (0: none); tile_layout ignores a width it cannot use
    bool full_copy = false, split_heavy = true, lookahead = true, collide_ordered = true, coop_all = true;
    bool warmstart = true, edge_contacts = true, pair_cull = true, raster_order = true;
    int run_ahead = 8, split_max_pct = 60, ablate = 0, heavy2_min = 16, os_cap = OS_CAP;
    int force_hcount[2] = {-1, -1};
    int skip_queues[2] = {0, 0};
};
static Settings read_settings() {
    Settings s;
    const char *v;
    if ((v = getenv("RR_TILE_W"))) s.tile_w = atoi(v);                        // width of a raster tile in place of the tile rule's (A/B, tests)
    s.full_copy = getenv("RR_FULL_COPY") != nullptr;                          // the earlier image update: the static layer copied into every image before each frame (tests)
    s.split_heavy = getenv("RR_NO_SPLIT") == nullptr;                         // set: all envs solved and rendered on the main stream (A/B, tests)
    s.lookahead = getenv("RR_NO_LOOKAHEAD") == nullptr;                       // set: every step prepares itself in line (A/B, tests)
    if ((v = getenv("RR_COLLIDE_ORDER"))) s.collide_ordered = atoi(v) != 0;   // 0: k_collide in env order instead of by falling duration of the last pass
    if ((v = getenv("RR_RUN_AHEAD"))) s.run_ahead = std::max(0, std::min(atoi(v), RUN_AHEAD_MAX));   // steps a caller that never waits may get ahead (default 8; 0: unbounded)
    if ((v = getenv("RR_COOP_ALL"))) s.coop_all = atoi(v) != 0;               // 0: the one-launch solve of a small batch four envs to a wave (A/B, tests)
    if ((v = getenv("RR_FORCE_HCOUNT"))) sscanf(v, "%d,%d", &s.force_hcount[0], &s.force_hcount[1]);   // "h,vh": what the placement decisions read instead of the lagged counters (tests)
    if ((v = getenv("RR_SPLIT_MAX_PCT"))) s.split_max_pct = atoi(v);          // the heavy / light split is used while at most this share of the envs is heavy (default 60)
    if ((v = getenv("RR_ABLATE"))) s.ablate = atoi(v);                        // development build only: phase ablations and counters
    if ((v = getenv("RR_HEAVY2_MIN"))) s.heavy2_min = atoi(v);                // generic contacts above which an env is "very heavy" (default 16; 1000: never; A/B 6..30: 13-16 best)
    s.warmstart = getenv("RR_NO_WARMSTART") == nullptr;                       // set: cold start of the contact solver every step (diagnostics)
    s.edge_contacts = getenv("RR_NO_EDGE_CONTACTS") == nullptr;               // set: vertex candidates only, no edge-edge pass (diagnostics)
    if ((v = getenv("RR_SOLVER_POOL"))) s.os_cap = std::max(0, std::min(atoi(v) / 60, (int)OS_CAP));   // LDS floats for object-vs-static rows, 60 per contact; contacts beyond take the generic path (tests)
    if ((v = getenv("RR_NO_PAIR_CULL"))) s.pair_cull = atoi(v) == 0;          // 1: k_collide without the pair cull of its broad phase (tests)
    if ((v = getenv("RR_SKIP_QUEUES"))) sscanf(v, "%d,%d", &s.skip_queues[0], &s.skip_queues[1]);      // "a,b": unused streams created in front of aux / aux2 (create_device)
    s.raster_order = getenv("RR_NO_RASTER_ORDER") == nullptr;                 // set: k_raster keeps its env-major grid instead of the cost order
    return s;
}
static const bool g_debug_sync = getenv("RR_DEBUG_SYNC") != nullptr;          // synchronise and report after every kernel; read when the library is loaded (TIMED)

// What rr_create computes from (cfg, blob) on the host and the handle keeps (parse_model fills it, create_device moves it into the rr_env).
struct ModelTables {
    BodyParams B = {};
    SimParams P = {};
    RenderModel RM = {};
    IkModel IK = {};
    int n_inst_used = 0;
    int n_shapes = 0;
    int shape_uid[MAXSHAPES] = {};   // the uid of every collision shape as in RR_F_MASK (the blob's shape_owner, column 3): RR_RAY_ID
    int shape_kind[MAXSHAPES] = {}, shape_idx[MAXSHAPES] = {};   // owner of every collision shape (0 static, 1 robot body, 2 object; its index): rr_set_distance_pairs
    float table_pos[3] = {};       // target of the default eye camera (env.py:253-255)
    // per-env object dynamics (rr_set_object_dynamics): host copies every upload of D.obj_dyn / D.pair_mat is made from
    std::vector<float> dyn;        // [N][nobj][8] {mass, ixx, iyy, izz, lateral friction, restitution, rolling, spinning}
    std::vector<float> pair_host;  // [N][npairs][4] the env's combined contact materials (pair_materials)
    std::vector<float> shape_mat;  // [ns][4] the blob's {friction, restitution, rolling, spinning} of every collision shape
    std::vector<int> shape_obj;    // [ns] the free object a shape belongs to, -1 for the table / shelf / robot
    std::vector<int> pair_shapes;  // [npairs][2] shapes a, b of every collision pair
    // per-env actuators (rr_set_env_actuators): the host copy every upload of D.env_act is made from, and what rr_get_env_actuators returns
    std::vector<float> act;        // [N][NB][4] {kp, kd, max_force, joint damping}
    float act_default[NB][4] = {}; // the handle's row of every joint: P.kp, P.kd, the motor force of rr_config, the blob's body_damping
    // swept clearance (rr_swept_clearance): R[k][s], how far a point of shape s can be from joint k's origin; 0 where k does not move s
    SweepReach sweep_reach = {};
};

// Everything rr_create needs from the model: the tables above and what is only uploaded.  The pointers point into the blob.
struct HostModel : ModelTables {
    ShapeData S = {};
    float body_tab[NB * BT_STRIDE] = {};   // the body lanes' constants (k_prep16)
    std::vector<float> soa;        // [9][nt] triangle positions
    std::vector<float> rec;        // [nt][32] one 128-byte shading record per triangle {pos[9], nrm[9], inst, -, uv[6], pad}
    std::vector<float> cvs;        // [nt / 64][3][64] the clusters' vertex positions
    std::vector<int32_t> tv4;      // [nt] the corner indices as ds_bpermute byte addresses
    const int32_t *tri_inst = nullptr;     // [nt]
    const float *cluster_sphere = nullptr; // [nt / 64][4]
    const uint8_t *tex = nullptr; size_t tex_bytes = 0;
};

struct rr_env : ModelTables {
    hipError_t step_err = hipSuccess; const char *step_err_what = nullptr;      // first failed event / wait / bound launch of the step path (HIPQ, step_status)
    rr_config cfg = {};
    Settings set;                  // as read when the handle was made; split_heavy also goes off when the device refuses the split's dynamic LDS (create_device)
    RenderModel *RM_dev = nullptr;
    DevPtrs D = {};
    hipStream_t stream = nullptr;
    size_t field_bytes[RR_F_COUNT] = {};
    void *field_ptr[RR_F_COUNT] = {};
    float *state_aos = nullptr;        // [N][61] staging for RR_F_STATE
    unsigned char *mask_dev = nullptr; // [N]
    float *link_out = nullptr;         // [N][nl][7]
    float *plan = nullptr; int *plan_step = nullptr; float *ik_in = nullptr; float *ik_out = nullptr; float *ik_err = nullptr;   // lazily allocated (macro / cartesian adapters)
    // device-resident macro actions (rr_step_macro): the request record [N][4], the list of the envs that need a plan [N] with its length
    // behind it, the `replanned` bytes [N] of the last call; allocated by the first call, with the plan buffers where they are missing
    float *macro_req = nullptr; int *macro_list = nullptr; unsigned char *macro_replanned = nullptr;
    // device-resident cartesian actions (rr_step_cartesian): the request record [N][7], its solution [N][7] and residual [N], the `solved`
    // bytes [N] of the last call, the list of the envs that need a solve [N] with its length behind it, and the staging of a host
    // caller's targets [N][7] and gripper commands [N][2]; one group, allocated by the first call
    float *cart_req = nullptr, *cart_sol = nullptr, *cart_res = nullptr, *cart_stage = nullptr; unsigned char *cart_solved = nullptr; int *cart_list = nullptr;
    float *score_out = nullptr; unsigned char *score_mask = nullptr;            // lazily allocated (rr_evaluate_goals)
    float4 *co_contacts = nullptr; float2 *co_force = nullptr; unsigned *co_partners = nullptr;   // lazily allocated (rr_contact_observations)
    // The output buffers of the ten query families (rr_query.inc): qbuf[family][which], a family's group allocated together on first use for
    // its capacity (query_capacity), once, zero-filled; qk[family]: the rows per env (postures, segments, targets) of the family's last
    // call, 0 before the first.  What else a family keeps on the device comes in the same list (ensure_query).
    void *qbuf[QF_COUNT][QUERY_MAX_BUFFERS] = {};
    int qk[QF_COUNT] = {};
    // the kinematic points, the ray table and the pair table are settings of the handle: a host copy and the device copy the kernels read
    int kin_np = 1;                // points in force: a fresh handle has link 8 (gripper `base`) at the origin of its COM frame
    KinPoints kin_pts = {{8}, {}};
    KinPoints *kin_pts_dev = nullptr;
    int ray_n = 0;                 // rays in force: a fresh handle has none
    RayTable ray_tab = {};
    RayTable *ray_tab_dev = nullptr;
    int dist_n = 0;                // pairs in force: a fresh handle has none
    DistTable dist_tab = {};
    DistTable *dist_tab_dev = nullptr;
    SweepReach *sw_reach_dev = nullptr;      // the device copy of ModelTables::sweep_reach
    // staging of a host caller's tensors, each got with the buffers or by the first host-path call that needs it: ray_stage [N, 64, 6] the
    // segments of rr_ray_cast; pc_stage [N, 32, 11] postures (and the seeds of rr_posture_ik); sw_stage [N, 32, 2, 11] the segments of
    // rr_swept_clearance; pik_stage [N, 32, 7] targets; pd_stage [2][N, 32, 11] the velocities and accelerations of rr_posture_dynamics
    float *ray_stage = nullptr, *pc_stage = nullptr, *sw_stage = nullptr, *pik_stage = nullptr, *pd_stage = nullptr;
    // joint torque inputs of the step (rr_set_joint_torques): the table [N][11], allocated zero-filled on first use; a host caller's rows go
    // through jt_stage [N][11]; jt_on: rr_step launches k_joint_torque (from the first successful set with a table until the clearing call)
    float *jt_table = nullptr;
    float *jt_stage = nullptr;
    bool jt_on = false;
    // external wrenches of the step (rr_set_external_wrenches): the table [N][14][6], allocated zero-filled on first use; a host caller's rows go
    // through xw_stage [N][14][6]; xw_on: rr_step launches k_ext_wrench (from the first successful set with a table until the clearing call)
    float *xw_table = nullptr;
    float *xw_stage = nullptr;
    bool xw_on = false;
    // objects attached to robot links in the posture queries (rr_set_attachments): the table [N][NOBJ][ATT_ROW] (rr_carry.inc), allocated
    // zero-filled -- all free -- on first use with its staging block; att_link [N][nobj]: the host copy of the link ids, -1 free (empty until
    // the first set); att_on: the three posture queries launch their CARRY instantiations (from the first successful set with links until the
    // unmasked detach).  No step reads any of it.
    float *att_table = nullptr;
    float *att_stage = nullptr;
    std::vector<int32_t> att_link;
    bool att_on = false;
    // the swept clearance with carried objects (rr_carried_sweep): chain[k][b], the joint offsets between joint k and body b, built and
    // uploaded by the first call that launches k_swept_clearance<true> (rr_sweep.inc)
    SweepChain sw_chain = {};
    SweepChain *sw_chain_dev = nullptr;
    MemOwner mem;                 // every device and pinned block of the handle (rr_mem.inc); `created`: rr_create is through, zero-fills go on the library's stream
    bool created = false;
    bool timing = false;
    int *h_hcount = nullptr;       // pinned host copy of D.hcount[0] (device-mapped: written by the first solve launch of every step, solve_body)
    bool images_valid = false;     // every env's image holds its previous frame (static layer + the pixels of its fragment list)
    unsigned char *stale_dev = nullptr;  // [N] device: the env's image predates the current static layer (rr_set_camera after its last frame)
    bool stale_any = false;        // some env may be stale: every render checks (cleared by a render of all envs)
    hipEvent_t ev[2 * RR_NUM_KERNELS] = {};
    hipStream_t aux = nullptr;     // side stream: the HBM-bound static-layer copy runs beside the VALU-bound physics / visibility kernels
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_dyn = nullptr, ev_join2 = nullptr, ev_vsolved = nullptr, ev_hsolved = nullptr, ev_rast = nullptr;
    hipStream_t aux2 = nullptr;    // the very heavy envs' solve + render (Settings::heavy2_min)
    std::vector<hipStream_t> unused_streams;   // Settings::skip_queues: created only to take hardware queue ids
    // Look-ahead (DESIGN.md 5.2): the state part of step t+1 (k_prep_ab16, k_collide) runs on the side streams behind the render
    // of the heavy / very heavy envs of step t, beside the main stream's shading.
    struct Frame { float4 *clist; int *ccount; float *cwarm; int *hgflag, *hlist, *hcount, *hlist2, *hcount2; } fr[2] = {};
    int cur = 0;                   // fr[cur]: the frame of the last solved step (rr_get_contacts, contact history); fr[cur ^ 1]: the look-ahead's
    bool la_valid = false;         // fr[cur ^ 1] and the scratch slab hold the collision pass / dynamics of the next step for the present state
    // cost-ordered dispatch of k_raster (Settings::raster_order)
    unsigned *item_perm = nullptr; // [8 * ceil(N / 8) * ntiles] the order, written by the extra workgroups of k_shade
    bool ord_valid = false, ord_pending = false;   // item_perm holds an order; a k_raster has left costs that the next k_shade launch turns into one
    void *obs_host = nullptr;      // rr_map_observations: mapped pinned block {joints [N][9], touch [N][4], poses [N][nobj][7], timestep [N], errflags [N]} or nullptr
    ObsMirror obs_dev = {};        // its device-visible addresses
    hipEvent_t ev_obs = nullptr;   // recorded behind the mirror's launches: rr_sync_observations waits for it alone
    bool ev_obs_set = false;
    void *img_host[3] = {};        // rr_map_images: pinned host copies of RGB / depth / mask that every rendered step refreshes (or nullptr)
    int img_sel = 7;               // rr_select_image_mirror: which of them a rendered step refreshes (bit 0 RGB, 1 depth, 2 mask)
    // Bounded run-ahead: a caller that never waits (bench.py, a training loop reading device buffers) gets hundreds of steps ahead of the
    // device -- the "lagged" list lengths that pick a step's placement are then those of a step 100+ steps back (measured on the macro
    // workload: readings 1 494 / 201 heavy / very heavy envs while the device solved 1 848 / 368, and 5 % of the step time lost to a
    // placement chosen for the smaller lists).  Every run_ahead / 2 steps rr_step records an event behind the step and first waits for
    // the one it recorded run_ahead steps earlier: the device always has run_ahead / 2 .. run_ahead steps in its queues, the readings are
    // that old at most, and the marker's few microseconds on the main stream are paid once in run_ahead / 2 steps (one every step cost
    // the headline 0.7 %).  Settings::run_ahead, 0: unbounded.
    hipEvent_t ahead_ev[2] = {};
    unsigned long long step_no = 0;
    float t_ms[RR_NUM_KERNELS] = {};
    int t_n[RR_NUM_KERNELS] = {};
    // pinned staging ring for per-step host inputs (commands, render flags): a hipMemcpyAsync from pageable memory blocks
    // the host until the copy is done; from these slots it is asynchronous, and a slot is reused only after the event
    // recorded behind its copy has completed
    char *pin_buf[4] = {}; hipEvent_t pin_ev[4] = {}; bool pin_used[4] = {}; int pin_next = 0; size_t pin_bytes = 0;
    // per-env cameras (rr_set_env_cameras): allocated by its first call; D.env_cam / D.static_* point at them while the handle is in
    // per-env mode, at the shared layer below otherwise (rr_set_camera)
    std::vector<float> cam_host;   // [N][cam_floats(ntiles)] host copy of every env's record
    float *cam_dev = nullptr;      // [N][cam_floats(ntiles)]
    int *cam_sel = nullptr;        // [N] class array of the rebuild launches: 0 the envs whose layer is rebuilt (sel 1 selects them), 1 the others
    unsigned long long *env_static_vis = nullptr; unsigned char *env_static_rgb = nullptr; float *env_static_depth = nullptr; int *env_static_mask = nullptr;   // [N][H*W]
    unsigned long long *shared_static_vis = nullptr; unsigned char *shared_static_rgb = nullptr; float *shared_static_depth = nullptr; int *shared_static_mask = nullptr;   // [H*W]
    bool cam_per_env = false, app_per_env = false; // which of the two per-env settings is in force; the per-env layers are in use (D.env_cam set) while either is
    // per-env appearance (rr_set_env_appearance): allocated by its first call; D.env_colour / D.env_light point at them while it is in force
    std::vector<float> colour_host, light_host;    // [N][MAXINST][3], [N][4] (unit vectors): what is uploaded, and what rr_get_env_appearance returns
    float *colour_dev = nullptr, *light_dev = nullptr;
    // goals and episodes (rr_set_goals .. rr_episode_update): a setting of the handle like the cameras.  The record's buffers are
    // allocated on first use and kept; the table and RR_EP_GOAL_RGB are replaced by rr_set_goals.
    GoalTable goals = {};          // device table in force (G 0: none)
    unsigned char *goals_rgb = nullptr;      // [G][H*W*3] the table's images or nullptr
    EpisodeRec ep = {};            // ep.score == nullptr: not allocated yet
    int *ep_index_stage = nullptr; // [N] staging of rr_set_env_goals' indices
    unsigned char *ep_goal_rgb = nullptr;    // RR_EP_GOAL_RGB [N][H*W*3]: exists exactly while the table has images
    size_t ep_bytes[RR_EP_COUNT] = {};
    int ep_horizon = 0, ep_stride = 1;
    // env forks and snapshot slots (rr_snapshot_slots, rr_copy_envs): a setting-free copy of env records on the device
    char *snap = nullptr; int n_slots = 0;   // the slots: one allocation of n_slots * fork_slot_bytes(N), replaced as a whole
    char *fork_stage = nullptr;    // the hidden staging slot of the in-place copies: allocated by the first one
    int *fork_index = nullptr;     // [N] device staging of a host index
};

// The combining rule of the contact materials of two shapes (btManifoldResult::calculateCombinedFriction / Restitution /
// RollingFriction / SpinningFriction, SURVEY A.1.6): products of friction and restitution, r_a mu_b + r_b mu_a at most 10 for
// rolling and spinning.  The one place that knows it: the blob's table (rr_create) and every env's (rr_set_object_dynamics).
// Host arithmetic on purpose: the device would contract the sums into fused multiply-adds of other last bits.
static void pair_materials(const float *a, const float *b, float *out) {
    out[0] = a[0] * b[0]; out[1] = a[1] * b[1];
    out[2] = std::min(a[2] * b[0] + b[2] * a[0], 10.0f);
    out[3] = std::min(a[3] * b[0] + b[3] * a[0], 10.0f);
}
static int upload_dynamics(rr_env *e);
static int upload_actuators(rr_env *e);

// The lagged host copies of the heavy / very heavy list lengths: written to mapped pinned memory by a recent step's kernels while
// the host runs, read here without any synchronisation -- ONCE per step (rr_step), so that every decision of a step's plan
// (plan_step, rr_plan.inc) rests on the same two numbers.  They only ever select a launch shape or a placement, never a result
// (every placement is forced and compared bitwise in tests/test_gpu_round4.py).  Settings::force_hcount pins what is read, here and
// nowhere else; without the pinned words a reading is known only when both are pinned.
static inline PlanCounts lagged_counts(const rr_env *e) {
    const int *f = e->set.force_hcount;
    PlanCounts c = {0, 0, e->h_hcount != nullptr || (f[0] >= 0 && f[1] >= 0)};
    if (e->h_hcount) { c.h = ((volatile int *)e->h_hcount)[0]; c.vh = ((volatile int *)e->h_hcount)[1]; }
    if (f[0] >= 0) c.h = f[0];
    if (f[1] >= 0) c.vh = f[1];
    return c;
}

// k_obs (joint angles and object poses of the state -> observation buffers) and, when mapped, the host mirror behind it
static int launch_mirror(rr_env *e, bool rendered = false) {
    if (e->obs_host) hipLaunchKernelGGL(k_obs_mirror, dim3((e->P.N + 63) / 64), dim3(64), 0, e->stream, e->P, e->D, e->obs_dev);
    if (rendered) {
        const int f[3] = {RR_F_RGB, RR_F_DEPTH, RR_F_MASK};
        for (int i = 0; i < 3; i++)
            if (e->img_host[i] && ((e->img_sel >> i) & 1) && e->field_ptr[f[i]]) HIPCHK(hipMemcpyAsync(e->img_host[i], e->field_ptr[f[i]], e->field_bytes[f[i]], hipMemcpyDeviceToHost, e->stream));
    }
    if (e->obs_host || e->img_host[0] || e->img_host[1] || e->img_host[2]) {
        if (!e->ev_obs) HIPCHK(hipEventCreateWithFlags(&e->ev_obs, hipEventDisableTiming));
        HIPCHK(hipEventRecord(e->ev_obs, e->stream));
        e->ev_obs_set = true;
    }
    HIPCHK(hipGetLastError());
    return RR_OK;
}
static void launch_obs(rr_env *e) {
    hipLaunchKernelGGL(k_obs, dim3((e->P.N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D);
    launch_mirror(e);
}

// The HIP backend of the handle's memory owner (rr_mem.inc): the one place that allocates and frees for an rr_env.  A failure is taken
// off HIP's last error -- not left behind for the next step's launch check.  Zero-fills of on-demand memory go on the library's stream:
// every consumer runs on it or on a side stream ordered behind it by ev_fork (rr_create's, in front of its blocking uploads, are hipMemset).
static const char *hip_mem_error(hipError_t rc) { if (rc == hipSuccess) return nullptr; (void)hipGetLastError(); return hipGetErrorString(rc); }
static void *hip_mem_alloc(void *, MemKind kind, size_t bytes, const char **err) {
    void *p = nullptr;
    *err = hip_mem_error(kind == MEM_DEVICE ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, kind == MEM_PINNED_MAPPED ? hipHostMallocMapped : hipHostMallocDefault));
    return *err ? nullptr : p;
}
static const char *hip_mem_zero(void *ctx, void *p, size_t bytes) {
    const rr_env *e = (const rr_env *)ctx;
    return hip_mem_error(e->created ? hipMemsetAsync(p, 0, bytes, e->stream) : hipMemset(p, 0, bytes));
}
static void hip_mem_release(void *, MemKind kind, void *p) { if (kind == MEM_DEVICE) (void)hipFree(p); else (void)hipHostFree(p); }
// a group of parts for the handle, all or nothing; `what`: "<entry point>: allocating <what>"
static int mem_get(rr_env *e, const MemPart *parts, size_t n, const char *what) {
    const char *err = e->mem.acquire(parts, n);
    return err ? fail(RR_EDEVICE, std::string(what) + ": " + err) : RR_OK;
}
static int mem_get(rr_env *e, std::initializer_list<MemPart> parts, const char *what) { return mem_get(e, parts.begin(), parts.size(), what); }
#define RRCHK(x) do { const int rc_ = (x); if (rc_ != RR_OK) return rc_; } while (0)

// VP = proj * view (row-major 4x4): the one product of a camera's matrices (rr_set_camera, rr_set_env_cameras, the default eye)
static void camera_vp(const float *view16, const float *proj16, float *VP) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            float a = 0;
            for (int k = 0; k < 4; k++) a += proj16[4 * i + k] * view16[4 * k + j];
            VP[4 * i + j] = a;
        }
}

static void look_at_persp(float *VP, const float *table_pos, int W, int H) {
    float eye[3] = {0.01f, 0.0f, 1.2f};                       // env.py:136
    float tgt[3] = {table_pos[0], table_pos[1], table_pos[2]};  // env.py:253-255 (table position)
    float up[3] = {0, 0, 1};
    float f[3] = {tgt[0] - eye[0], tgt[1] - eye[1], tgt[2] - eye[2]};
    float fl = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    f[0] /= fl; f[1] /= fl; f[2] /= fl;
    float s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    float sl = sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    s[0] /= sl; s[1] /= sl; s[2] /= sl;
    float u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    float V[16] = {s[0], s[1], s[2], -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]),
                   u[0], u[1], u[2], -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]),
                   -f[0], -f[1], -f[2], (f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]),
                   0, 0, 0, 1};
    float fov = 80.0f, nearv = 0.1f, farv = 100.0f;           // env.py:518,548-551
    float aspect = (float)W / (float)H;
    float yscale = 1.0f / tanf(fov * 3.14159265358979323846f / 360.0f);
    float xscale = yscale / aspect;
    float Pm[16] = {xscale, 0, 0, 0, 0, yscale, 0, 0, 0, 0, (nearv + farv) / (nearv - farv), 2 * nearv * farv / (nearv - farv), 0, 0, -1, 0};
    camera_vp(V, Pm, VP);
}

// The frustum planes' norms and the tiles' planes (RenderModel::plane_norm, tile_plane) of the camera VP, for RM's raster tiles:
// the handle's camera (rr_set_camera) and every env's record (rr_set_env_cameras) come from this one function.
static void frustum_plane_norms(const RenderModel &RM, const float *V, float *plane_norm, float (*tile_plane)[8]) {
    const float sg[4] = {1, -1, 1, -1};
    const int row[4] = {0, 0, 1, 1};
    for (int k = 0; k < 4; k++) {
        float a = V[12] + sg[k] * V[4 * row[k]], b = V[13] + sg[k] * V[4 * row[k] + 1], c = V[14] + sg[k] * V[4 * row[k] + 2];
        plane_norm[k] = sqrtf(a * a + b * b + c * c);
    }
    plane_norm[4] = sqrtf(V[12] * V[12] + V[13] * V[13] + V[14] * V[14]);
    // the two tile-boundary planes of every raster tile (conservative cull of a cluster against the tile's sample rows)
    for (int tile = 0; tile < RM.ntiles && tile < 256; tile++) {
        const int tyi = tile / RM.ntx, tx0 = (tile - tyi * RM.ntx) * RM.tile_w, cols = std::min(RM.tile_w, RM.W - tx0);
        const int row0 = tyi * RM.tile_h, rows = std::min(RM.tile_h, RM.H - row0);
        const float ty0 = (float)(RM.H - 1 - (row0 + rows - 1)), ty1 = (float)(RM.H - 1 - row0);
        for (int k = 0; k < 2; k++) {
            const float ndc = 2.0f * (k ? ty1 : ty0) / (float)RM.H - 1.0f;
            const float a = V[4] - ndc * V[12], b = V[5] - ndc * V[13], c = V[6] - ndc * V[14];
            tile_plane[tile][2 * k] = ndc; tile_plane[tile][2 * k + 1] = sqrtf(a * a + b * b + c * c);
            // (sample column px sits at NDC x = 2 px / W - 1: the viewport maps (x + 1) W / 2)
            const float ndx = 2.0f * (float)(k ? tx0 + cols - 1 : tx0) / (float)RM.W - 1.0f;
            const float ax = V[0] - ndx * V[12], bx = V[1] - ndx * V[13], cx = V[2] - ndx * V[14];
            tile_plane[tile][4 + 2 * k] = ndx; tile_plane[tile][5 + 2 * k] = sqrtf(ax * ax + bx * bx + cx * cx);
        }
    }
}

// Raster tiles of <= TILE_PIX pixels: full-width strips up to 128 columns (the 128 x 128 benchmark camera: four strips of 32
// rows); 64 x 64 squares for wider images -- a cluster of the arm is ~25 pixels across at 320 x 240 and met three of the
// 12-row strips a full-width tile would be there (set-up work x 3.1; squares: x 1.9).  Settings::tile_w overrides (A/B, tests).
// The one place that knows the rule: rr_create's size check and the RenderModel both come from here.
struct TileLayout { int tile_w, tile_h, ntx, ntiles, tile_xbits; unsigned w_magic; };
static TileLayout tile_layout(int W, int H, int tile_w_override) {
    TileLayout t;
    t.tile_w = W <= 128 ? W : 64;
    if (tile_w_override >= 4 && tile_w_override <= W && tile_w_override <= TILE_PIX) t.tile_w = tile_w_override;
    t.ntx = (W + t.tile_w - 1) / t.tile_w;
    t.tile_h = std::min(TILE_PIX / t.tile_w, H);
    t.ntiles = t.ntx * ((H + t.tile_h - 1) / t.tile_h);
    t.tile_xbits = 0; while ((1 << t.tile_xbits) < t.tile_w) t.tile_xbits++;
    t.w_magic = (unsigned)((0x100000000ull + (unsigned long long)t.tile_w - 1) / (unsigned long long)t.tile_w);
    return t;
}

// Phase 1 of rr_create, host only: everything the handle needs from (cfg, blob), checked.  Calls no HIP function and owns every
// RR_EMODEL exit, so a malformed model is reported as such on any machine.  cfg has passed rr_create's argument checks.
static int parse_model(const rr_config &cfg, const Blob &b, const Settings &set, HostModel &M) {
    const int32_t *dims = b.i32("dims", 11);
    if (!dims) return fail(RR_EMODEL, "rr_create: blob has no dims");
    const int nb = dims[0], nl = dims[1], ns = dims[2], ni = dims[3], nt = dims[4], ntex = dims[5], n_static = dims[6], n_robot = dims[7];
    if (nb != NB || ns > MAXSHAPES || dims[8] != VMAXC || dims[9] != FMAXC || ni > MAXINST || ni > RASTER_INST || nl > NLINK_MAX || ntex > 16 ||
        n_static != 3 || n_robot != 16)
        return fail(RR_EMODEL, "rr_create: blob dims do not match this build");
    const int N = cfg.num_envs;
#define NEED(p) if (!(p)) return fail(RR_EMODEL, "rr_create: blob entry missing/short: " #p)
    const float *f; const int32_t *ip;
    BodyParams &B = M.B;
    NEED(ip = b.i32("body_parent", NB)); memcpy(B.parent, ip, sizeof B.parent);
    if (memcmp(B.parent, PARENT_HOST, sizeof PARENT_HOST) != 0) return fail(RR_EMODEL, "rr_create: kinematic tree differs from the compiled-in one");
    NEED(f = b.f32("body_jpos", NB * 3)); memcpy(B.jpos, f, sizeof B.jpos);
    NEED(f = b.f32("body_jrot", NB * 9)); memcpy(B.jrot, f, sizeof B.jrot);
    NEED(f = b.f32("body_axis", NB * 3)); memcpy(B.axis, f, sizeof B.axis);
    NEED(f = b.f32("body_mass", NB)); memcpy(B.mass, f, sizeof B.mass);
    NEED(f = b.f32("body_com", NB * 3)); memcpy(B.com, f, sizeof B.com);
    NEED(f = b.f32(cfg.use_urdf_inertia ? "body_inertia_urdf" : "body_inertia", NB * 6)); memcpy(B.inertia, f, sizeof B.inertia);
    NEED(f = b.f32("body_damping", NB)); memcpy(B.damping, f, sizeof B.damping);
    NEED(f = b.f32("body_limits", NB * 2)); memcpy(B.limits, f, sizeof B.limits);
    NEED(f = b.f32("robot_pos", 3)); memcpy(B.robot_pos, f, sizeof B.robot_pos);
    NEED(f = b.f32("obj_mass", NOBJ)); memcpy(B.obj_mass, f, sizeof B.obj_mass);
    NEED(f = b.f32("obj_inertia", NOBJ * 3)); memcpy(B.obj_inertia, f, sizeof B.obj_inertia);
    NEED(f = b.f32("obj_pose0", NOBJ * 7)); memcpy(B.obj_pose0, f, sizeof B.obj_pose0);
    NEED(f = b.f32("table_pos", 3)); memcpy(M.table_pos, f, sizeof M.table_pos); B.table_z = f[2];
    NEED(f = b.f32("act_min", 9)); memcpy(B.act_min, f, sizeof B.act_min);
    NEED(f = b.f32("act_max", 9)); memcpy(B.act_max, f, sizeof B.act_max);
    NEED(f = b.f32("act_maxdiff", 9)); memcpy(B.act_maxdiff, f, sizeof B.act_maxdiff);
    NEED(ip = b.i32("touch_links", 4)); memcpy(B.touch_links, ip, sizeof B.touch_links);
    if (cfg.solver_flags & RR_SOLVER_NO_RATE_LIMIT)      // env.py:314-321 skipped: +-inf never clips (fminf / fmaxf of the command part)
        for (int k = 0; k < 9; k++) B.act_maxdiff[k] = INFINITY;
    for (int j = 0; j < NB; j++) {      // the body lanes' constants (k_prep16)
        float *t = M.body_tab + j * BT_STRIDE;
        for (int k = 0; k < 3; k++) { t[BT_COM + k] = B.com[j][k]; t[BT_AXIS + k] = B.axis[j][k]; }
        for (int k = 0; k < 6; k++) t[BT_INERTIA + k] = B.inertia[j][k];
        t[BT_MASS] = B.mass[j]; t[BT_DAMP] = B.damping[j];
    }
    const float *link_pos, *link_rot; const int32_t *link_body;
    NEED(link_body = b.i32("link_body", nl)); NEED(link_pos = b.f32("link_pos", nl * 3)); NEED(link_rot = b.f32("link_rot", nl * 9));
    {   // arm chain + gripper base frame (link id 8 = `base`, rigidly attached to body 6) for the IK kernels
        IkModel &K = M.IK;
        for (int j = 0; j < 7; j++) { memcpy(K.jpos[j], B.jpos[j], 12); memcpy(K.jrot[j], B.jrot[j], 36); memcpy(K.axis[j], B.axis[j], 12); }
        memcpy(K.robot_pos, B.robot_pos, 12);
        const int ee = 8;       // URDF depth-first id of the gripper `base` link (pybullet link index 7)
        if (nl <= ee || link_body[ee] != 6) return fail(RR_EMODEL, "rr_create: gripper base link not found");
        memcpy(K.ee_pos, link_pos + 3 * ee, 12); memcpy(K.ee_rot, link_rot + 9 * ee, 36);
        K.single_seed = (cfg.solver_flags & RR_SOLVER_IK_SINGLE_SEED) ? 1 : 0;
    }

    SimParams &P = M.P;
    P.N = N; P.nobj = cfg.n_objects; P.iters = cfg.solver_iters > 0 ? cfg.solver_iters : 50;
    P.dt = cfg.dt > 0 ? cfg.dt : 0.005f; P.gravity = 9.81f; P.erp = cfg.erp > 0 ? cfg.erp : 0.2f;
    P.margin = cfg.margin > 0 ? cfg.margin : 0.02f;
    // the UPSTREAM constants (pybullet's defaults, SURVEY A.1.2 / A.1.4 / A.1.5) are parameters of the handle: 0 -> default, < 0 -> literal zero
    auto upstream = [](float v, float dflt) { return v > 0.0f ? v : (v < 0.0f ? 0.0f : dflt); };
    P.kp = upstream(cfg.motor_kp, 0.1f); P.kd = upstream(cfg.motor_kd, 1.0f);
    P.max_impulse = upstream(cfg.motor_max_force, 100000.0f) * P.dt;
    P.ablate = set.ablate; P.heavy2_min = set.heavy2_min; P.edge_contacts = set.edge_contacts ? 1 : 0; P.os_cap = set.os_cap;
    P.warmstart = set.warmstart ? upstream(cfg.warmstart, 0.85f) : 0.0f;
    P.lin_damp = upstream(cfg.lin_damping, 0.04f); P.ang_damp = upstream(cfg.ang_damping, 0.04f); P.rest_thresh = 0.2f;

    // shapes + pair table (same order as the oracle's collide())
    ShapeData &S = M.S;
    NEED(ip = b.i32("shape_owner", ns * 4));
    for (int s = 0; s < ns; s++) { S.otype[s] = ip[4 * s]; S.oidx[s] = ip[4 * s + 1]; S.link[s] = ip[4 * s + 2]; M.shape_uid[s] = ip[4 * s + 3]; M.shape_kind[s] = ip[4 * s]; M.shape_idx[s] = ip[4 * s + 1]; }
    NEED(ip = b.i32("shape_nv", ns)); memcpy(S.nv, ip, ns * 4);
    NEED(ip = b.i32("shape_nf", ns)); memcpy(S.nf, ip, ns * 4);
    NEED(f = b.f32("shape_verts", ns * VMAXC * 3)); memcpy(S.verts, f, (size_t)ns * VMAXC * 3 * 4);
    NEED(f = b.f32("shape_planes", ns * FMAXC * 4)); memcpy(S.planes, f, (size_t)ns * FMAXC * 4 * 4);
    NEED(f = b.f32("shape_sphere", ns * 4)); memcpy(S.sphere, f, (size_t)ns * 4 * 4);
    NEED(f = b.f32("shape_mat", ns * 2));
    for (int s = 0; s < ns; s++) { S.fric[s] = f[2 * s]; S.rest[s] = f[2 * s + 1]; }
    NEED(f = b.f32("shape_roll", ns * 2));       // URDF <rolling_friction>, <spinning_friction> (cube.urdf:6-7, kuka_gripper.urdf:292-296 ...)
    for (int s = 0; s < ns; s++) { S.roll[s] = f[2 * s]; S.spin[s] = f[2 * s + 1]; }
    {   // (optional field: the radii hold for margins up to the one they were compiled for)
        const float *ro = b.f32("shape_roff", ns + 1);
        for (int s = 0; s < ns; s++) S.roff[s] = (ro && P.margin <= ro[ns] && set.pair_cull) ? ro[s] : INFINITY;
    }
    NEED(ip = b.i32("shape_ne", ns)); memcpy(S.ne, ip, ns * 4);
    NEED(f = b.f32("shape_edges", ns * EMAXC * 12)); memcpy(S.edges, f, (size_t)ns * EMAXC * 12 * 4);
    for (int s = 0; s < ns; s++) if (S.ne[s] < 0 || S.ne[s] > EMAXC) return fail(RR_EMODEL, "rr_create: bad shape_ne");
    int np = 0, s_obj0 = n_static + n_robot;
    for (int i = 0; i < P.nobj; i++) for (int s = 0; s < n_static; s++) { S.pair_a[np] = s_obj0 + i; S.pair_b[np++] = s; }
    for (int i = 0; i < P.nobj; i++) for (int j = i + 1; j < P.nobj; j++) { S.pair_a[np] = s_obj0 + i; S.pair_b[np++] = s_obj0 + j; }
    for (int r = 0; r < n_robot; r++) for (int s = 0; s < 2; s++) { S.pair_a[np] = n_static + r; S.pair_b[np++] = s; }
    for (int r = 0; r < n_robot; r++) for (int i = 0; i < P.nobj; i++) { S.pair_a[np] = n_static + r; S.pair_b[np++] = s_obj0 + i; }
    P.npairs = np;
    M.n_shapes = ns;
    if (ns > CSHAPES) return fail(RR_EMODEL, "rr_create: more collision shapes than k_collide stages in LDS");
    // the reach table of rr_swept_clearance, in float64 and rounded up: |sphere centre| + radius in the shape's body b, plus the joint
    // offsets |jpos[m]| of the bodies m from b up to the child of k on b's chain
    for (int s = 0; s < ns; s++) {
        if (S.otype[s] != 1 || S.oidx[s] < 0 || S.oidx[s] >= NB) continue;
        const double c[3] = {S.sphere[s][0], S.sphere[s][1], S.sphere[s][2]};
        double r = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + (double)S.sphere[s][3];
        for (int k = S.oidx[s]; k >= 0; k = PARENT_HOST[k]) {
            float f = (float)r;
            if ((double)f < r) f = std::nextafterf(f, INFINITY);
            M.sweep_reach.r[k][s] = f;
            const double j[3] = {B.jpos[k][0], B.jpos[k][1], B.jpos[k][2]};
            r += std::sqrt(j[0] * j[0] + j[1] * j[1] + j[2] * j[2]);
        }
    }
    for (int k = 0; k < np; k++) {
        const int sa = S.pair_a[k], sb = S.pair_b[k];
        S.pair_meta[k][0] = S.otype[sa] == 0 ? -1 : (S.otype[sa] == 1 ? S.oidx[sa] : 16 + S.oidx[sa]);
        S.pair_meta[k][1] = S.otype[sb] == 0 ? -1 : (S.otype[sb] == 1 ? S.oidx[sb] : 16 + S.oidx[sb]);
        S.pair_meta[k][2] = S.link[sa]; S.pair_meta[k][3] = 0;
        const float ma[4] = {S.fric[sa], S.rest[sa], S.roll[sa], S.spin[sa]}, mb[4] = {S.fric[sb], S.rest[sb], S.roll[sb], S.spin[sb]};
        pair_materials(ma, mb, S.pair_mat[k]);
        M.pair_shapes.push_back(sa); M.pair_shapes.push_back(sb);
    }
    for (int s = 0; s < ns; s++) {
        M.shape_mat.insert(M.shape_mat.end(), {S.fric[s], S.rest[s], S.roll[s], S.spin[s]});
        M.shape_obj.push_back(S.otype[s] == 2 && S.oidx[s] >= 0 && S.oidx[s] < P.nobj ? S.oidx[s] : -1);
    }
    // the default dynamics of every env: the blob's mass and inertia of an object, the materials of its first collision shape
    // (the model has one per object), and the blob's pair table
    M.dyn.assign((size_t)N * P.nobj * 8, 0.0f);
    for (int i = 0; i < P.nobj; i++) {
        float row[8] = {B.obj_mass[i], B.obj_inertia[i][0], B.obj_inertia[i][1], B.obj_inertia[i][2], 0.0f, 0.0f, 0.0f, 0.0f};
        for (int s = ns - 1; s >= 0; s--) if (M.shape_obj[s] == i) memcpy(row + 4, &M.shape_mat[4 * s], 16);
        for (int n = 0; n < N; n++) memcpy(&M.dyn[((size_t)n * P.nobj + i) * 8], row, 32);
    }
    // the default actuators of every env: the handle's motor constants, the blob's joint damping
    for (int j = 0; j < NB; j++) {
        const float row[4] = {P.kp, P.kd, upstream(cfg.motor_max_force, 100000.0f), B.damping[j]};
        memcpy(M.act_default[j], row, 16);
    }
    M.act.resize((size_t)N * NB * 4);
    for (int n = 0; n < N; n++) memcpy(&M.act[(size_t)n * NB * 4], M.act_default, sizeof M.act_default);
    M.pair_host.resize((size_t)N * np * 4);
    for (int n = 0; n < N; n++) memcpy(&M.pair_host[(size_t)n * np * 4], S.pair_mat, (size_t)np * 16);

    // k_collide's warm-start matching looks for the previous contacts of the same bodies (bodyA, bodyB, linkA) among the
    // pairs pair-2 .. pair+2 only: pairs with equal keys must form runs of at most three consecutive pairs (one collision shape
    // per robot link against table / shelf, one per object against the three statics)
    for (int k = 0; k < np; k++)
        for (int j = 0; j < np; j++) {
            const bool same = S.pair_meta[k][0] == S.pair_meta[j][0] && S.pair_meta[k][1] == S.pair_meta[j][1] && S.pair_meta[k][2] == S.pair_meta[j][2];
            if (same && std::abs(k - j) > 2) return fail(RR_EMODEL, "rr_create: collision pairs of the same bodies are more than two apart in the pair table (warm-start matching window)");
        }

    // render model
    RenderModel &RM = M.RM;
    RM.ni = ni; RM.nt = nt; RM.W = cfg.width; RM.H = cfg.height; RM.nl = nl;
    const TileLayout tl = tile_layout(RM.W, RM.H, set.tile_w);
    RM.tile_w = tl.tile_w; RM.tile_h = tl.tile_h; RM.ntx = tl.ntx; RM.ntiles = tl.ntiles; RM.tile_xbits = tl.tile_xbits; RM.w_magic = tl.w_magic;
    NEED(ip = b.i32("inst_owner", ni * 4));
    for (int i = 0; i < ni; i++) { RM.in_otype[i] = ip[4 * i]; RM.in_oidx[i] = ip[4 * i + 1]; RM.in_uid[i] = ip[4 * i + 2]; RM.in_tex[i] = ip[4 * i + 3]; }
    NEED(f = b.f32("inst_color", ni * 3)); memcpy(RM.in_color, f, (size_t)ni * 12);
    NEED(ip = b.i32("tex_info", ntex * 3));
    for (int t = 0; t < ntex; t++) { RM.tex_off[t] = ip[3 * t]; RM.tex_w[t] = ip[3 * t + 1]; RM.tex_h[t] = ip[3 * t + 2]; }
    NEED(M.tex = b.u8("tex_data", &M.tex_bytes));
    // a one-texel texture (the arm's colours: tools/compile_model.py stores uniform images as 1 x 1) travels with the instance
    // constants -- width -1, the texel in place of the offset: its fragments fetch neither texture coordinates nor texels
    for (int t = 0; t < ntex; t++)
        if (RM.tex_w[t] == 1 && RM.tex_h[t] == 1 && (size_t)RM.tex_off[t] * 4 + 4 <= M.tex_bytes) {
            uint32_t px; memcpy(&px, M.tex + (size_t)RM.tex_off[t] * 4, 4);
            RM.tex_off[t] = (int)px; RM.tex_w[t] = -1;
        }
    memcpy(RM.link_body, link_body, nl * 4); memcpy(RM.link_pos, link_pos, (size_t)nl * 12); memcpy(RM.link_rot, link_rot, (size_t)nl * 36);
    NEED(ip = b.i32("inst_range", ni * 2));
    const int n_static_inst = dims[10];
    RM.first_dynamic_tri = (n_static_inst < ni) ? ip[2 * n_static_inst] : nt;
    look_at_persp(RM.VP, M.table_pos, RM.W, RM.H);
    frustum_plane_norms(RM, RM.VP, RM.plane_norm, RM.tile_plane);
    M.n_inst_used = ni - (NOBJ - P.nobj);

    // geometry: positions SoA [9][NT], one shading record per triangle, the clusters' vertices and corner indices
    const float *tp, *tn, *tu, *cvb; const int32_t *tv;
    NEED(tp = b.f32("tri_pos", (size_t)nt * 9)); NEED(tn = b.f32("tri_nrm", (size_t)nt * 9));
    NEED(tu = b.f32("tri_uv", (size_t)nt * 6)); NEED(M.tri_inst = b.i32("tri_inst", nt));
    if (nt % 64 != 0 || nt / 64 > MAXWIN || nt >= (1 << 18)) return fail(RR_EMODEL, "rr_create: triangle count must be a multiple of the cluster size 64 and below 65536");
    NEED(M.cluster_sphere = b.f32("cluster_sphere", (size_t)(nt / 64) * 4));
    NEED(cvb = b.f32("cluster_verts", (size_t)nt * 3)); NEED(tv = b.i32("tri_vidx", nt));
#undef NEED
    M.soa.resize((size_t)nt * 9);
    for (int t = 0; t < nt; t++) for (int k = 0; k < 9; k++) M.soa[(size_t)k * nt + t] = tp[(size_t)t * 9 + k];
    M.rec.assign((size_t)nt * 32, 0.0f);
    for (int t = 0; t < nt; t++) {
        float *r = &M.rec[(size_t)t * 32];
        memcpy(r, tp + (size_t)t * 9, 36); memcpy(r + 9, tn + (size_t)t * 9, 36); memcpy(r + 18, M.tri_inst + t, 4);
        memcpy(r + 20, tu + (size_t)t * 6, 24);          // (chunks 5, 6: only textured instances' fragments fetch them, load_tri_rec)
    }
    M.cvs.resize((size_t)nt * 3);          // [cluster][64][3] -> [cluster][3][64]
    for (int c = 0; c < nt / 64; c++)
        for (int v = 0; v < 64; v++)
            for (int k = 0; k < 3; k++) M.cvs[((size_t)c * 3 + k) * 64 + v] = cvb[((size_t)c * 64 + v) * 3 + k];
    // (the corner indices go to the device as ds_bpermute byte addresses, index x 4 in each byte: one bit-field extract per
    // corner in the window loop instead of a shift and a mask)
    M.tv4.resize((size_t)nt);
    for (int t = 0; t < nt; t++) {
        const int a0 = tv[t] & 63, a1 = (tv[t] >> 8) & 63, a2 = (tv[t] >> 16) & 63;
        M.tv4[t] = (a0 << 2) | (a1 << 10) | (a2 << 18);
    }
    return RR_OK;
}

extern "C" {

const char *rr_last_error(void) { return g_err.c_str(); }
int rr_abi_version(void) { return RR_ABI_VERSION; }

int rr_destroy(rr_env *e) {
    if (!e) return RR_OK;
    hipSetDevice(e->cfg.device);
    hipStreamSynchronize(e->stream);
    for (int i = 0; i < 2 * RR_NUM_KERNELS; i++) if (e->ev[i]) hipEventDestroy(e->ev[i]);
    if (e->aux) { hipStreamSynchronize(e->aux); hipStreamDestroy(e->aux); }
    if (e->aux2) { hipStreamSynchronize(e->aux2); hipStreamDestroy(e->aux2); }
    for (hipStream_t s : e->unused_streams) hipStreamDestroy(s);
    for (hipEvent_t ev : {e->ev_join2, e->ev_vsolved, e->ev_hsolved, e->ev_rast, e->ev_fork, e->ev_join, e->ev_dyn, e->ev_obs, e->ahead_ev[0], e->ahead_ev[1]})
        if (ev) hipEventDestroy(ev);
    for (hipEvent_t ev : e->pin_ev) if (ev) hipEventDestroy(ev);
    e->mem.release_all();
    delete e;
    return RR_OK;
}

// points the device view at the contact frames: current = fr[cur], next = fr[cur ^ 1]
static void bind_frames(rr_env *e) {
    const rr_env::Frame &C = e->fr[e->cur], &X = e->fr[e->cur ^ 1];
    DevPtrs &D = e->D;
    D.clist = C.clist; D.ccount = C.ccount; D.cwarm = C.cwarm; D.hgflag = C.hgflag; D.hlist = C.hlist; D.hcount = C.hcount; D.hlist2 = C.hlist2; D.hcount2 = C.hcount2;
    D.clist_next = X.clist; D.ccount_next = X.ccount; D.cwarm_next = X.cwarm; D.hgflag_next = X.hgflag; D.hlist_next = X.hlist; D.hcount_next = X.hcount;
    D.hlist2_next = X.hlist2; D.hcount2_next = X.hcount2;
}

// The contact count and the class of every env belong to the contact frame of the last solved step, which changes place every
// step: the solve kernels publish both into fixed [N] buffers, so that a pointer from rr_get_buffer stays valid (realrobot.h).
static void refresh_frame_fields(rr_env *e) {
    e->field_ptr[RR_F_CONTACT_COUNT] = e->D.ccount_pub;
    e->field_ptr[RR_F_ENV_CLASS] = e->D.class_pub;
}

static ImageOut env_images(const rr_env *e) {
    ImageOut o;
    o.rgb = e->D.rgb; o.depth = e->D.depth; o.mask = e->D.mask; o.env_stride = (size_t)e->RM.W * e->RM.H;
    return o;
}

// (Re)builds the shared static layer for the current camera: background everywhere, then the never-moving instances (table,
// shelf, robot base; the eye camera is fixed, env.py:136-141, 253-255) are rasterised and shaded once; their visibility keys
// seed every env's frame.
static int build_static_layer(rr_env *e) {
    hipLaunchKernelGGL(k_background, dim3(64), dim3(256), 0, e->stream, e->RM_dev, e->D, 1, (const unsigned char *)nullptr);
    ImageOut so;
    so.rgb = e->D.static_rgb; so.depth = e->D.static_depth; so.mask = e->D.static_mask; so.env_stride = 0;
    e->D.static_vis = nullptr;
    hipLaunchKernelGGL(k_render_setup, dim3((e->P.N * MAXINST + 63) / 64), dim3(64), 0, e->stream, e->B, e->P, e->RM_dev, e->D, 0);
    hipLaunchKernelGGL(k_raster, dim3(1, e->RM.ntiles), dim3(RASTER_THREADS), 0, e->stream, e->P, e->RM_dev, e->D, e->n_inst_used, 1, 0, 0, 0);
    hipLaunchKernelGGL(k_shade, dim3(1, e->RM.ntiles, SHADE_SPLIT), dim3(SHADE_THREADS), 0, e->stream, e->RM_dev, e->D, so, 0, 0, 0, 0, (unsigned *)nullptr);
    // the pass above used env 0's fragment list; from here on the lists describe what differs from the static layer
    if (hipMemsetAsync(e->D.frag_count, 0, (size_t)e->P.N * e->RM.ntiles * sizeof(unsigned), e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) return fail(RR_EDEVICE, "static layer pass failed");
    e->D.static_vis = e->D.static_vis_out;
    // Before the first frame of a handle every image starts from a full copy of the static layer.  Later (rr_set_camera) an
    // env's image is its last frame, which a step that does not render it must leave alone: each env takes the full copy of the
    // new layer at its own next render instead.
    if (e->images_valid) {
        if (hipMemsetAsync(e->stale_dev, 1, (size_t)e->P.N, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess)
            return fail(RR_EDEVICE, "static layer pass failed");
        e->stale_any = true;
    }
    return RR_OK;
}

// Phase 2 of rr_create, device: allocations, uploads, streams and events, first reset and the static layer.  rr_create owns the
// handle: every failure here just returns, and the caller's guard destroys what was built.
static int create_device(rr_env *e, const rr_config &cfg, const Settings &set, HostModel &M, void *stream) {
    e->cfg = cfg;
    e->stream = (hipStream_t)stream;
    HIPCHK(hipSetDevice(cfg.device));
    static_cast<ModelTables &>(*e) = std::move(static_cast<ModelTables &>(M));
    e->set = set;
    e->mem.be = MemBackend{e, hip_mem_alloc, hip_mem_zero, hip_mem_release};
    if (!e->mem.acquire({mem_part(&e->h_hcount, 4 * sizeof(int), true, MEM_PINNED_MAPPED)})) e->h_hcount[2] = -1;      // (the step runs without the word)
    const SimParams &P = e->P;
    const RenderModel &RM = e->RM;
    const int N = P.N, nt = RM.nt, np = P.npairs;
    DevPtrs &D = e->D;
    // (one allocation per buffer, in this order; zeroed unless uploaded over)
#define ALLOC(ptr, count) RRCHK(mem_get(e, {mem_part(&(ptr), (count) * sizeof *(ptr))}, "rr_create: allocating device memory"))
#define COPY(ptr, src, count, bytes) do { ALLOC(ptr, count); HIPCHK(hipMemcpy((void *)(ptr), (src), (bytes) ? (bytes) : (count) * sizeof *(ptr), hipMemcpyHostToDevice)); } while (0)      // (bytes 0: the whole array)
    ALLOC(D.state, (size_t)ST_TOTAL * N);
    ALLOC(D.scratch, (size_t)S_TOTAL * N);
    for (int f = 0; f < 2; f++) {
        rr_env::Frame &F = e->fr[f];
        ALLOC(F.clist, (size_t)N * MAXC * 3); ALLOC(F.ccount, (size_t)N); ALLOC(F.cwarm, (size_t)N * MAXC);
        ALLOC(F.hgflag, (size_t)N); ALLOC(F.hlist, (size_t)N); ALLOC(F.hcount, (size_t)4); ALLOC(F.hlist2, (size_t)N); ALLOC(F.hcount2, (size_t)4);
    }
    bind_frames(e);
    ALLOC(D.cforce, (size_t)N * MAXC);
    COPY(D.body_tab, M.body_tab, (size_t)NB * BT_STRIDE, 0);
    ALLOC(D.collide_cost, (size_t)N); ALLOC(D.collide_bin, (size_t)N); ALLOC(D.collide_perm, (size_t)8 * ((N + 7) / 8));      // (zeroed: the first order is arbitrary)
    ALLOC(D.ccount_pub, (size_t)N); ALLOC(D.class_pub, (size_t)N);
    if (e->h_hcount && hipHostGetDevicePointer((void **)&D.hcount_host, e->h_hcount, 0) != hipSuccess) D.hcount_host = nullptr;
    ALLOC(D.timestep, (size_t)N);
    ALLOC(D.errflags, (size_t)N);
    ALLOC(D.obj_home, (size_t)NOBJ * 7 * N);
    {
        float *od_ = nullptr; float4 *pm_ = nullptr; float *ea_ = nullptr;
        ALLOC(od_, (size_t)NOBJ * 4 * N); ALLOC(pm_, (size_t)N * np);
        D.obj_dyn = od_; D.pair_mat = pm_;
        RRCHK(upload_dynamics(e));
        ALLOC(ea_, (size_t)NB * 4 * N);
        D.env_act = ea_;
        RRCHK(upload_actuators(e));
    }
    ALLOC(D.grows, (size_t)N * GP_RECS * 16);        // (zeroed: the dummy block / contact records stay all zero)
    ALLOC(D.cmd, (size_t)N * 9);
    ALLOC(D.joints, (size_t)N * 9);
    ALLOC(D.touch, (size_t)N * 4);
    ALLOC(D.objpose, (size_t)N * P.nobj * 7);
    ALLOC(D.inst_xf, (size_t)N * MAXINST * 32);
    ALLOC(D.render_flags, (size_t)N);
    ALLOC(e->stale_dev, (size_t)N);
    const size_t npx = (size_t)N * RM.W * RM.H;
    ALLOC(D.rgb, npx * 3);
    ALLOC(D.depth, npx);
    if (!(cfg.flags & RR_FLAG_NO_MASK)) ALLOC(D.mask, npx);
    ALLOC(e->state_aos, (size_t)N * NSTATE);
    ALLOC(e->mask_dev, (size_t)N);
    ALLOC(e->link_out, (size_t)N * RM.nl * 7);
    COPY(D.tri_pos, M.soa.data(), (size_t)nt * 9, 0);
    COPY(D.tri_rec, M.rec.data(), (size_t)nt * 8, 0);
    COPY(D.tri_inst, M.tri_inst, (size_t)nt, 0);
    COPY(D.tex, M.tex, M.tex_bytes / 4 + 1, M.tex_bytes);
    COPY(D.shapes, &M.S, (size_t)1, 0);
    ALLOC(e->RM_dev, 1);
    HIPCHK(hipMemcpy(e->RM_dev, &e->RM, sizeof e->RM, hipMemcpyHostToDevice));
    COPY(D.cluster_verts, M.cvs.data(), (size_t)nt * 3, 0);
    COPY(D.tri_vidx, M.tv4.data(), (size_t)nt, 0);
    COPY(D.cluster_sphere, M.cluster_sphere, (size_t)nt / 64, 0);
    for (int i = 0; i < 2 * RR_NUM_KERNELS; i++) HIPCHK(hipEventCreate(&e->ev[i]));
    {
        // fork / join events order two streams of the same device: no timing, no system-scope fence (the cache writeback
        // and invalidation a default event performs when it is recorded costs ~6 us on the stream that records it)
        const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
        // the side stream carries the step's longest chain (the heavy envs' solve, then their render): with a higher
        // priority its few workgroups are dispatched ahead of the main stream's render when both are ready
        int prio_lo = 0, prio_hi = 0;
        hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        // (a runtime without stream priorities: plain non-blocking streams)
        auto side_stream = [&](hipStream_t *st) { return hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_hi) == hipSuccess || hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess; };
        // Which hardware queue a stream gets follows from the streams the PROCESS has created before it, and the step is very
        // sensitive to it: with one unused stream created in front of `aux` (or of `aux2`) the headline step takes 0.89 ms instead of
        // 0.585, with one in front of each 0.585 again (round 6, NOTEBOOK.md B; tools/ubench/queue_probe.hip shows 50-70 us of extra
        // launch latency between some pairs of queues).  The order below is the one measured in bench.py's process, alone and behind an
        // RCCL process group; Settings::skip_queues creates a / b unused streams in front of aux / aux2 -- for a host process whose
        // stream history differs (scratch/streams_check.py compares the settings on the spot).  Do not reorder these calls.
        auto skip_queues = [&](int n) { for (int i = 0; i < n && i < 8; i++) { hipStream_t unused; if (hipStreamCreateWithFlags(&unused, hipStreamNonBlocking) != hipSuccess) return false; e->unused_streams.push_back(unused); } return true; };
        if (!skip_queues(set.skip_queues[0]) || !side_stream(&e->aux) || hipEventCreateWithFlags(&e->ev_fork, evf) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_join, evf) != hipSuccess || hipEventCreateWithFlags(&e->ev_dyn, evf) != hipSuccess ||
            !skip_queues(set.skip_queues[1]) || !side_stream(&e->aux2) || hipEventCreateWithFlags(&e->ev_join2, evf) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_vsolved, evf) != hipSuccess || hipEventCreateWithFlags(&e->ev_hsolved, evf) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_rast, evf) != hipSuccess) return fail(RR_EDEVICE, "rr_create: side stream");
    }
    e->field_ptr[RR_F_JOINTS] = D.joints; e->field_bytes[RR_F_JOINTS] = (size_t)N * 9 * 4;
    e->field_ptr[RR_F_TOUCH] = D.touch; e->field_bytes[RR_F_TOUCH] = (size_t)N * 4 * 4;
    e->field_ptr[RR_F_OBJ_POSE] = D.objpose; e->field_bytes[RR_F_OBJ_POSE] = (size_t)N * P.nobj * 7 * 4;
    e->field_ptr[RR_F_RGB] = D.rgb; e->field_bytes[RR_F_RGB] = npx * 3;
    e->field_ptr[RR_F_DEPTH] = D.depth; e->field_bytes[RR_F_DEPTH] = npx * 4;
    e->field_ptr[RR_F_MASK] = D.mask; e->field_bytes[RR_F_MASK] = D.mask ? npx * 4 : 0;
    e->field_ptr[RR_F_TIMESTEP] = D.timestep; e->field_bytes[RR_F_TIMESTEP] = (size_t)N * 4;
    e->field_ptr[RR_F_ERRFLAGS] = D.errflags; e->field_bytes[RR_F_ERRFLAGS] = (size_t)N * 4;
    e->field_ptr[RR_F_STATE] = e->state_aos; e->field_bytes[RR_F_STATE] = (size_t)N * NSTATE * 4;
    e->field_bytes[RR_F_FRAG_COUNT] = (size_t)N * RM.ntiles * 4;     // pointer set once the list is allocated
    e->field_bytes[RR_F_CONTACT_COUNT] = (size_t)N * 4; e->field_bytes[RR_F_ENV_CLASS] = (size_t)N * 4;
    e->field_ptr[RR_F_PREP] = D.scratch; e->field_bytes[RR_F_PREP] = (size_t)N * S_TOTAL * 4;
    static_assert(S_TOTAL == 378, "include/realrobot.h documents RR_F_PREP as 378 floats per env");
    // (pointers set once the buffers exist: ensure_contact_obs)
    e->field_bytes[RR_F_CONTACTS] = (size_t)N * MAXC * 12 * 4; e->field_bytes[RR_F_BODY_FORCE] = (size_t)N * RR_CONTACT_ROWS * 2 * 4;
    e->field_bytes[RR_F_BODY_PARTNERS] = (size_t)N * RR_CONTACT_ROWS * 4;
    refresh_frame_fields(e);
    for (int i = 0; i < NOBJ; i++) RRCHK(rr_set_object_home(e, -1, i, e->B.obj_pose0[i]));
    RRCHK(rr_reset(e, nullptr));
    const size_t spx = (size_t)RM.W * RM.H, items = (size_t)N * RM.ntiles;
    ALLOC(D.static_rgb, spx * 3); ALLOC(D.static_depth, spx); ALLOC(D.static_mask, spx); ALLOC(D.frag_count, items);
    RRCHK(mem_get(e, {mem_part(&D.frag_list, items * TILE_PIX * sizeof *D.frag_list, false)}, "rr_create: allocating the fragment lists"));
    if (set.raster_order && items >= 2048 && items <= (1 << 20) && N < (1 << 24)) {
        ALLOC(D.item_cost, items); ALLOC(D.item_bin, items); ALLOC(e->item_perm, (size_t)8 * ((N + 7) / 8) * RM.ntiles);
    }
    ALLOC(D.static_vis_out, spx);
#undef COPY
#undef ALLOC
    e->field_ptr[RR_F_FRAG_COUNT] = D.frag_count;
    e->shared_static_vis = D.static_vis_out; e->shared_static_rgb = D.static_rgb;
    e->shared_static_depth = D.static_depth; e->shared_static_mask = D.static_mask;
    RRCHK(build_static_layer(e));
    // the 256-thread form of k_solve (heavy solver groups, four per workgroup) and the light envs' solve with an object wave (five
    // waves, sixteen envs) ask for 158 KiB of dynamic LDS: only the heavy / light split launches them, and a device that cannot grant
    // it runs without the split (same results, one launch)
    const int lds_split = (int)(4 * SGRP * LF_TOTAL * sizeof(float));
    if (e->set.split_heavy && (hipFuncSetAttribute((const void *)k_solve, hipFuncAttributeMaxDynamicSharedMemorySize, lds_split) != hipSuccess ||
                           hipFuncSetAttribute((const void *)k_solve_rs, hipFuncAttributeMaxDynamicSharedMemorySize, lds_split) != hipSuccess ||
                           hipFuncSetAttribute((const void *)k_solve_light_ow, hipFuncAttributeMaxDynamicSharedMemorySize, lds_split) != hipSuccess)) {
        (void)hipGetLastError();
        e->set.split_heavy = false;
    }
    if (hipGetLastError() != hipSuccess) return fail(RR_EDEVICE, "rr_create: device error during set-up");
    e->created = true;
    return RR_OK;
}

int rr_create(const rr_config *cfg, const void *model_blob, size_t blob_bytes, void *stream, rr_env **out) {
    if (!cfg || !model_blob || !out) return fail(RR_EINVAL, "rr_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != RR_ABI_VERSION) return fail(RR_EINVAL, "rr_create: abi_version mismatch");
    if (cfg->num_envs < 1) return fail(RR_EINVAL, "rr_create: num_envs < 1");
    if ((unsigned long long)cfg->num_envs * GP_ENV_BYTES + 4096ull >= (1ull << 32)) return fail(RR_EINVAL, "rr_create: more than 33222 envs per rr_env (32-bit byte offsets of the solver's row store)");
    if (cfg->n_objects < 1 || cfg->n_objects > NOBJ) return fail(RR_EINVAL, "rr_create: n_objects must be 1..3");
    for (float v : {cfg->motor_kp, cfg->motor_kd, cfg->motor_max_force, cfg->warmstart, cfg->lin_damping, cfg->ang_damping, cfg->dt, cfg->erp, cfg->margin})
        if (!std::isfinite(v)) return fail(RR_EINVAL, "rr_create: non-finite motor / solver constant");
    if (cfg->solver_flags & ~(RR_SOLVER_NO_RATE_LIMIT | RR_SOLVER_IK_SINGLE_SEED)) return fail(RR_EINVAL, "rr_create: unknown solver_flags bit");
    if (cfg->width < 4 || cfg->height < 1 || cfg->width % 4 != 0 || cfg->width > 1024 || cfg->height > 1024)
        return fail(RR_EINVAL, "rr_create: width must be a multiple of 4 in [4,1024], height in [1,1024] (10-bit box origins in the rasteriser's records)");
    const Settings set = read_settings();
    if (tile_layout(cfg->width, cfg->height, set.tile_w).ntiles > 255)      // (the tile index is 8 bits with one sentinel)
        return fail(RR_EINVAL, "rr_create: image too large: more than 255 raster tiles of 4096 pixels (e.g. 1024 x 960 fits, 1024 x 961 does not)");
    Blob b;
    if (!b.init(model_blob, blob_bytes)) return fail(RR_EMODEL, "rr_create: bad model blob header");
    const std::unique_ptr<HostModel> M(new HostModel());
    const int rm = parse_model(*cfg, b, set, *M);
    if (rm != RR_OK) return rm;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(RR_EDEVICE, "rr_create: no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(RR_EINVAL, "rr_create: bad device ordinal");
    struct Destroy { void operator()(rr_env *p) const { rr_destroy(p); } };
    std::unique_ptr<rr_env, Destroy> e(new rr_env());       // the one owner of the half-built handle
    const int rc = create_device(e.get(), *cfg, set, *M, stream);
    if (rc != RR_OK) return rc;
    *out = e.release();
    return RR_OK;
}

int rr_set_stream(rr_env *e, void *stream) {
    if (!e) return fail(RR_EINVAL, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->stream = (hipStream_t)stream;
    return RR_OK;
}

int rr_reset(rr_env *e, const uint8_t *mask_host) {
    if (!e) return fail(RR_EINVAL, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    const unsigned char *m = nullptr;
    if (mask_host) {
        HIPCHK(hipMemcpyAsync(e->mask_dev, mask_host, e->P.N, hipMemcpyHostToDevice, e->stream));
        m = e->mask_dev;
    }
    e->la_valid = false;          // the state changes from outside: the next step prepares itself in line
    hipLaunchKernelGGL(k_reset, dim3((e->P.N + 255) / 256), dim3(256), 0, e->stream, e->B, e->P, e->D, m);
    launch_obs(e);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// The pose an object returns to on reset and when it leaves the table (robot.py:19-24 `object_poses`, which callers of the
// reference edit in place, e.g. tests/test_actions.py:95-98). env_index < 0: every env.
int rr_set_object_home(rr_env *e, int32_t env_index, int32_t obj, const float *pose7) {
    if (!e || !pose7) return fail(RR_EINVAL, "null argument");
    if (env_index >= e->P.N || obj < 0 || obj >= NOBJ) return fail(RR_EINVAL, "rr_set_object_home: index out of range");
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;          // the out-of-bounds rule of the look-ahead used the old home pose
    const size_t N = e->P.N;
    if (env_index >= 0) {
        for (int k = 0; k < 7; k++)
            HIPCHK(hipMemcpyAsync(e->D.obj_home + (size_t)(7 * obj + k) * N + env_index, pose7 + k, 4, hipMemcpyHostToDevice, e->stream));
    } else {
        std::vector<float> col(N);
        for (int k = 0; k < 7; k++) {
            std::fill(col.begin(), col.end(), pose7[k]);
            HIPCHK(hipMemcpyAsync(e->D.obj_home + (size_t)(7 * obj + k) * N, col.data(), N * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream));   // pose7 is host memory
    return RR_OK;
}

// The device tables of the per-env object dynamics from the host copies: D.obj_dyn ({mass, inertia} of every object, SoA; objects
// the handle does not simulate keep the blob's values) and D.pair_mat (every env's combined materials).  Synchronous.
static int upload_dynamics(rr_env *e) {
    const size_t N = e->P.N;
    const int no = e->P.nobj;
    std::vector<float> od((size_t)NOBJ * 4 * N);
    for (int i = 0; i < NOBJ; i++)
        for (int k = 0; k < 4; k++)
            for (size_t n = 0; n < N; n++)
                od[(size_t)(4 * i + k) * N + n] = i < no ? e->dyn[(n * no + i) * 8 + k] : (k == 0 ? e->B.obj_mass[i] : e->B.obj_inertia[i][k - 1]);
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;          // the look-ahead's object terms and contact list were made with the old values
    HIPCHK(hipMemcpyAsync((void *)e->D.obj_dyn, od.data(), od.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync((void *)e->D.pair_mat, e->pair_host.data(), e->pair_host.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // the sources are host memory
    return RR_OK;
}

// changeDynamics / getDynamicsInfo of the free objects, per env (rows {mass, ixx, iyy, izz, lateral friction, restitution, rolling,
// spinning}).  The rows of the masked envs are checked first and the call changes nothing unless all of them are valid; an object's
// materials apply to all of its collision shapes, the pair materials of the env are combined again on the host (pair_materials).
int rr_set_object_dynamics(rr_env *e, const float *dyn_host, const uint8_t *env_mask_host) {
    if (!e || !dyn_host) return fail(RR_EINVAL, "null argument");
    const int N = e->P.N, no = e->P.nobj;
    for (int n = 0; n < N; n++) {
        if (env_mask_host && !env_mask_host[n]) continue;
        for (int i = 0; i < no; i++) {
            const float *r = dyn_host + ((size_t)n * no + i) * 8;
            for (int k = 0; k < 8; k++)
                if (!std::isfinite(r[k]) || (k < 4 ? !(r[k] > 0.0f) : !(r[k] >= 0.0f)))
                    return fail(RR_EINVAL, "rr_set_object_dynamics: env " + std::to_string(n) + " object " + std::to_string(i) +
                                               (k < 4 ? ": mass and inertia must be finite and > 0" : ": friction, restitution, rolling and spinning friction must be finite and >= 0"));
        }
    }
    const int np = e->P.npairs;
    for (int n = 0; n < N; n++) {
        if (env_mask_host && !env_mask_host[n]) continue;
        memcpy(&e->dyn[(size_t)n * no * 8], dyn_host + (size_t)n * no * 8, (size_t)no * 32);
        for (int k = 0; k < np; k++) {
            float m[2][4];
            for (int j = 0; j < 2; j++) {
                const int s = e->pair_shapes[2 * k + j], o = e->shape_obj[s];
                memcpy(m[j], o >= 0 ? &e->dyn[((size_t)n * no + o) * 8 + 4] : &e->shape_mat[4 * s], 16);
            }
            pair_materials(m[0], m[1], &e->pair_host[((size_t)n * np + k) * 4]);
        }
    }
    return upload_dynamics(e);
}

int rr_get_object_dynamics(rr_env *e, float *dyn_out_host) {
    if (!e || !dyn_out_host) return fail(RR_EINVAL, "null argument");
    memcpy(dyn_out_host, e->dyn.data(), e->dyn.size() * 4);
    return RR_OK;
}

// The device table of the per-env actuators from the host copy: D.env_act, SoA with the env index innermost, the motor force as the
// impulse bound max_force * dt (the float product rr_create makes for P.max_impulse: the default table holds that very value).  Synchronous.
static int upload_actuators(rr_env *e) {
    const size_t N = e->P.N;
    std::vector<float> ea((size_t)NB * 4 * N);
    for (int j = 0; j < NB; j++)
        for (int k = 0; k < 4; k++)
            for (size_t n = 0; n < N; n++) {
                const float v = e->act[(n * NB + j) * 4 + k];
                ea[(size_t)(k * NB + j) * N + n] = k == 2 ? v * e->P.dt : v;
            }
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;          // the look-ahead's unconstrained joint velocities were made with the old damping
    HIPCHK(hipMemcpyAsync((void *)e->D.env_act, ea.data(), ea.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // the source is host memory
    return RR_OK;
}

// setJointMotorControl2(positionGain=, velocityGain=, force=) / changeDynamics(jointDamping=) of the robot's joints, per env (rows
// {kp, kd, max_force, joint damping} in the order of q[11]).  The rows of the masked envs are checked first and the call changes
// nothing unless all of them are valid; a null table puts the masked envs back on the handle's values.
int rr_set_env_actuators(rr_env *e, const float *act_host, const uint8_t *env_mask_host) {
    if (!e) return fail(RR_EINVAL, "null argument");
    const int N = e->P.N;
    static const char *const what[4] = {"kp", "kd", "max_force", "joint_damping"};
    if (act_host)
        for (int n = 0; n < N; n++) {
            if (env_mask_host && !env_mask_host[n]) continue;
            for (int j = 0; j < NB; j++)
                for (int k = 0; k < 4; k++) {
                    const float v = act_host[((size_t)n * NB + j) * 4 + k];
                    if (!std::isfinite(v) || !(v >= 0.0f) || (k == 2 && !std::isfinite(v * e->P.dt)))
                        return fail(RR_EINVAL, "rr_set_env_actuators: env " + std::to_string(n) + " joint " + std::to_string(j) + ": " + what[k] +
                                                   " must be finite and >= 0");
                }
        }
    for (int n = 0; n < N; n++) {
        if (env_mask_host && !env_mask_host[n]) continue;
        memcpy(&e->act[(size_t)n * NB * 4], act_host ? act_host + (size_t)n * NB * 4 : &e->act_default[0][0], sizeof e->act_default);
    }
    return upload_actuators(e);
}

int rr_get_env_actuators(rr_env *e, float *act_out_host) {
    if (!e || !act_out_host) return fail(RR_EINVAL, "null argument");
    memcpy(act_out_host, e->act.data(), e->act.size() * 4);
    return RR_OK;
}

int rr_set_object_pose(rr_env *e, int32_t env_index, int32_t obj, const float *pose7) {
    if (!e || !pose7) return fail(RR_EINVAL, "null argument");
    if (env_index < 0 || env_index >= e->P.N || obj < 0 || obj >= e->P.nobj) return fail(RR_EINVAL, "rr_set_object_pose: index out of range");
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;
    const size_t N = e->P.N;
    float zero = 0.0f;
    for (int k = 0; k < 3; k++) {
        HIPCHK(hipMemcpyAsync(e->D.state + (ST_OPOS + 3 * obj + k) * N + env_index, pose7 + k, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->D.state + (ST_OVEL + 3 * obj + k) * N + env_index, &zero, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->D.state + (ST_OANG + 3 * obj + k) * N + env_index, &zero, 4, hipMemcpyHostToDevice, e->stream));
    }
    for (int k = 0; k < 4; k++)
        HIPCHK(hipMemcpyAsync(e->D.state + (ST_OQUAT + 4 * obj + k) * N + env_index, pose7 + 3 + k, 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));   // pose7/zero are stack/host memory
    launch_obs(e);
    return RR_OK;
}

// Batched form of rr_set_object_pose: one upload and one kernel for the whole batch (set_goal of N envs, env.py:151-166).
int rr_set_object_poses(rr_env *e, const float *poses_host, const uint8_t *env_mask_host) {
    if (!e || !poses_host) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;
    const int N = e->P.N;
    static_assert(NSTATE >= NOBJ * 7, "the state staging buffer doubles as pose staging");
    HIPCHK(hipMemcpyAsync(e->state_aos, poses_host, (size_t)N * e->P.nobj * 28, hipMemcpyHostToDevice, e->stream));
    const unsigned char *m = nullptr;
    if (env_mask_host) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask_host, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_set_object_poses, dim3((N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, e->state_aos, m);
    launch_obs(e);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));   // the arguments are host memory
    return RR_OK;
}

#define TIMED(id, launch)                                                   \
    do {                                                                    \
        if (e->timing) hipEventRecord(e->ev[2 * (id)], e->stream);          \
        launch;                                                             \
        if (g_debug_sync) { hipError_t e__ = hipStreamSynchronize(e->stream); fprintf(stderr, "[rr] kernel %d done: %s\n", (id), hipGetErrorString(e__)); } \
        if (e->timing) {                                                    \
            hipEventRecord(e->ev[2 * (id) + 1], e->stream);                 \
            hipEventSynchronize(e->ev[2 * (id) + 1]);                       \
            float ms_ = 0;                                                  \
            hipEventElapsedTime(&ms_, e->ev[2 * (id)], e->ev[2 * (id) + 1]); \
            e->t_ms[id] += ms_; e->t_n[id] += 1;                            \
        }                                                                   \
    } while (0)

// Image set-up that precedes a frame: the first frame of a handle starts every image (all envs) from a full copy of the static
// layer; after a new static layer (rr_set_camera) each env rendered in this frame whose image predates it takes the full copy.
static int ensure_images(rr_env *e, DevPtrs &D) {
    const int N = e->P.N;
    const ImageOut io = env_images(e);
    const int copy_blocks = std::min(16, (e->RM.W * e->RM.H / 4 + COPY_THREADS - 1) / COPY_THREADS);
    if (!e->images_valid || e->set.full_copy) {
        DevPtrs Dall = D;
        if (!e->images_valid) Dall.render_flags = nullptr;      // first frame: every env, flagged or not -- all images become valid
        TIMED(5, hipLaunchKernelGGL(k_static_copy, dim3(copy_blocks, std::min(N, 65535)), dim3(COPY_THREADS), 0, e->stream, e->RM_dev, Dall, io, 1, N,
                                    (const unsigned char *)nullptr));
        if (!e->images_valid) HIPCHK(hipMemsetAsync(e->D.frag_count, 0, (size_t)N * e->RM.ntiles * sizeof(unsigned), e->stream));
        if (!e->images_valid || !D.render_flags) {       // (every image now holds the current static layer)
            if (e->stale_any) HIPCHK(hipMemsetAsync(e->stale_dev, 0, (size_t)N, e->stream));
            e->stale_any = false;
        }
        e->images_valid = true;
        return 0;           // the lists are empty: nothing to restore
    }
    if (e->stale_any) {
        TIMED(5, hipLaunchKernelGGL(k_static_copy, dim3(copy_blocks, std::min(N, 65535)), dim3(COPY_THREADS), 0, e->stream, e->RM_dev, D, io, 1, N,
                                    (const unsigned char *)e->stale_dev));
        hipLaunchKernelGGL(k_stale_clear, dim3((N + 255) / 256), dim3(256), 0, e->stream, e->RM_dev, D, N, e->stale_dev);
        if (!D.render_flags) e->stale_any = false;      // a frame of every env: none is stale any more
    }
    return 1;
}

// The first failed event / wait / bound launch of the step path (HIPQ, LAUNCH_EV), reported once by the entry point that queued it.
static int step_status(rr_env *e) {
    if (e->step_err == hipSuccess) return RR_OK;
    const std::string msg = std::string(e->step_err_what ? e->step_err_what : "step") + ": " + hipGetErrorString(e->step_err);
    e->step_err = hipSuccess; e->step_err_what = nullptr;
    e->la_valid = false;                 // (whatever the look-ahead queued is not to be trusted)
    return fail(RR_EDEVICE, msg);
}
// Visibility pass of the envs selected by `sel` (all, or the light ones): one workgroup per (env, tile), dispatched in the order of the
// last frame's costs when the batch is large enough to matter; the shading launch behind it makes the next order (DESIGN.md 5).
static void launch_raster(rr_env *e, const DevPtrs &D, int restore, int sel, hipStream_t st) {
    const int N = e->P.N, nt = e->RM.ntiles;
    DevPtrs Do = D;
    Do.item_perm = e->item_perm && e->ord_valid ? e->item_perm : nullptr;
    hipLaunchKernelGGL(k_raster, Do.item_perm ? dim3((unsigned)(8 * ((N + 7) / 8) * nt)) : dim3(N, nt), dim3(RASTER_THREADS), 0, st, e->P, e->RM_dev, Do, e->n_inst_used, 0, 0, restore, sel);
    e->ord_pending = e->item_perm != nullptr;
}
// A launch with an event that completes with it: bound to the launch itself (hipExtLaunchKernelGGL's stop event) instead of recorded
// by a marker of its own behind it -- the next launch of the stream and whoever waits for the event are one packet closer
// (A/B: headline 0.593 -> 0.591 ms, config 2 0.3666 -> 0.3648 ms).  done == nullptr: a plain launch.
// A bound launch that FAILS (e.g. a dynamic LDS request the device refuses) would leave its event at its previous recording and
// every hipStreamWaitEvent on it would pass at once -- the streams would race on the contact frames instead of failing cleanly:
// the launch result is checked on the spot, the error kept for rr_step's return (HIPQ) and the event recorded explicitly.
#define HIPQ(x) do { const hipError_t q_ = (x); if (q_ != hipSuccess && e->step_err == hipSuccess) { e->step_err = q_; e->step_err_what = #x; } } while (0)
#define LAUNCH_EV(done, kernel, grid, block, lds, st, ...)                                                        \
    do { if (done) { hipExtLaunchKernelGGL(kernel, grid, block, lds, st, nullptr, (done), 0, __VA_ARGS__);        \
                     const hipError_t l_ = hipGetLastError();                                                     \
                     if (l_ != hipSuccess) { if (e->step_err == hipSuccess) { e->step_err = l_; e->step_err_what = "launch of " #kernel; } (void)hipEventRecord((done), st); } } \
         else hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__); } while (0)
static void launch_shade(rr_env *e, const DevPtrs &D, const ImageOut &io, int sel, hipStream_t st, hipEvent_t done = nullptr) {
    const int N = e->P.N;
    const bool ord = e->ord_pending && sel <= 1;       // (behind launch_raster on the same stream)
    LAUNCH_EV(done, k_shade, dim3(N + (ord ? 1 : 0), e->RM.ntiles, SHADE_SPLIT), dim3(SHADE_THREADS), 0, st, e->RM_dev, D, io, 1, 0, sel, ord ? N : 0, e->item_perm);
    if (ord) { e->ord_pending = false; e->ord_valid = true; }
}
// The three render kernels for the envs selected by `sel` (env_selected) on `st`.  The images persist in HBM from frame to
// frame: only the pixels of the previous frame's fragment lists are put back to the static layer (`restore`), DESIGN.md 5.
// `setup_done`: the instances of these envs are set up already (by the light solve).
// `done`: an event that completes with the last launch.
// The heavy list (sel 2) in the form the plan picked (StepPlan::heavy_render); the very heavy one (sel 3) is always walked by one launch.
static void launch_render(rr_env *e, const StepPlan &pl, const DevPtrs &D, int restore, int sel, hipStream_t st, bool setup_done = false, hipEvent_t done = nullptr) {
    const int N = e->P.N;
    const ImageOut io = env_images(e);
    if (sel == 3 || (sel == 2 && pl.heavy_render == RENDER_WALKER)) {
        LAUNCH_EV(done, k_render_list, dim3(std::min(N * e->RM.ntiles, sel == 3 ? 256 : RENDER_LIST_WGS)), dim3(RASTER_THREADS), 0, st, e->B, e->P, e->RM_dev, D, io, e->n_inst_used, restore, sel == 3 ? 1 : 0, setup_done ? 1 : 0);
        return;
    }
    if (!setup_done) hipLaunchKernelGGL(k_render_setup, dim3((N * MAXINST + 63) / 64), dim3(64), 0, st, e->B, e->P, e->RM_dev, D, sel);
    if (sel == 2 && pl.heavy_render == RENDER_GRID) { DevPtrs Dp = D; Dp.item_perm = nullptr; hipLaunchKernelGGL(k_raster, dim3(N, e->RM.ntiles), dim3(RASTER_THREADS), 0, st, e->P, e->RM_dev, Dp, e->n_inst_used, 0, 0, restore, sel); }
    else if (sel == 2) hipLaunchKernelGGL(k_raster_list, dim3(std::min(N * e->RM.ntiles, RASTER_LIST_WGS)), dim3(RASTER_THREADS), 0, st, e->P, e->RM_dev, D, e->n_inst_used, restore, 0);
    else launch_raster(e, D, restore, sel, st);
    launch_shade(e, D, io, sel, st, done);
}
// The same three kernels under their timers (rr_render, a single-class step, the timing leg): the grid kernels whatever the class.
static void launch_render_timed(rr_env *e, const DevPtrs &D, int restore, int sel, hipStream_t st, bool setup_done = false) {
    const ImageOut io = env_images(e);
    if (!setup_done) TIMED(3, hipLaunchKernelGGL(k_render_setup, dim3((e->P.N * MAXINST + 63) / 64), dim3(64), 0, st, e->B, e->P, e->RM_dev, D, sel));
    TIMED(4, launch_raster(e, D, restore, sel, st));
    TIMED(6, launch_shade(e, D, io, sel, st));
}

static int do_render(rr_env *e, bool use_flags) {
    DevPtrs D = e->D;
    if (!use_flags) D.render_flags = nullptr;
    const int restore = ensure_images(e, D);
    launch_render_timed(e, D, restore, 0, e->stream);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// ---- look-ahead: the state part of the NEXT step (k_prep_a16 -> k_collide, k_prep_b16 beside them) --------------------------
// Per-class launches (sel: pick_env) cover N work items whatever the class.
#define COLLIDE_ORDER_MIN_N 1024   // up to this many envs all collision workgroups are resident at once: no order needed
// (collision pass in cost order: the eight sorting workgroups ride on the preparation launch in front of it -- batches of more than
// one round of collision workgroups, all envs; Settings::collide_ordered off: env order)
static inline bool collide_in_order(const rr_env *e, int sel) { return sel == 0 && e->set.collide_ordered && e->P.N > COLLIDE_ORDER_MIN_N; }
// (k_prep16: one env per 16-lane group, four envs per workgroup -- of 128 threads where the objects' wave rides along)
static inline dim3 prep16_grid(const rr_env *e, int sel, bool order) { return dim3((e->P.N + P16_ENVS - 1) / P16_ENVS + (order && collide_in_order(e, sel) ? 8 : 0)); }
static void launch_prep_a(rr_env *e, int sel, int zero_counts, hipStream_t st, hipEvent_t done = nullptr) {
    LAUNCH_EV(done, k_prep_a16, prep16_grid(e, sel, true), dim3(128), 0, st, e->B, e->P, e->D, sel, zero_counts, collide_in_order(e, sel) ? e->P.N : 0);
}
static void launch_prep_b(rr_env *e, int sel, hipStream_t st, hipEvent_t done = nullptr) {
    LAUNCH_EV(done, k_prep_b16, prep16_grid(e, sel, false), dim3(64), 0, st, e->B, e->P, e->D, sel);
}
static void launch_collide(rr_env *e, int sel, hipStream_t st, hipEvent_t done = nullptr) {
    const bool ordered = collide_in_order(e, sel);
    const dim3 grid(ordered ? 8 * ((e->P.N + 7) / 8) : e->P.N);
    LAUNCH_EV(done, k_collide, grid, dim3(COLLIDE_THREADS), 0, st, e->P, e->D, e->n_shapes, sel, ordered ? 1 : 0);
}
static void launch_prep_ab(rr_env *e, int sel, hipStream_t st) {
    hipLaunchKernelGGL(k_prep_ab16, prep16_grid(e, sel, true), dim3(128), 0, st, e->B, e->P, e->D, sel, collide_in_order(e, sel) ? e->P.N : 0);
}

// The solve of the heavy (sel 2) / very heavy (sel 3) envs on `st`, in the form the plan picked (StepPlan::coop_*): one env per
// wave, four waves per workgroup with one LDS region each (N waves: whatever the list's actual length, every entry has its
// wave; the others exit at once), or four envs to a wave.  beside_raster false: a step without camera.
static void launch_solve_class(rr_env *e, const StepPlan &pl, int sel, hipStream_t st, const RenderModel *fused_rm = nullptr, hipEvent_t done = nullptr, bool beside_raster = true) {
    const int N = e->P.N;
    const int ngroups = (N + SGRP - 1) / SGRP;
    const size_t lds64 = (size_t)SGRP * LF_TOTAL * sizeof(float);
    const bool coop = sel == 2 ? pl.coop_h : (beside_raster ? pl.coop_vh_beside : pl.coop_vh_alone);
    // (fused_rm: the step draws -- the kernel also sets up the render instances of its envs, as the light solve does)
    if (fused_rm) {
        if (coop) LAUNCH_EV(done, k_solve_rs, dim3((N + 3) / 4), dim3(256), lds64, st, e->B, e->P, e->D, sel, 1, fused_rm);
        else LAUNCH_EV(done, k_solve_rs, dim3((ngroups + 3) / 4), dim3(256), 4 * lds64, st, e->B, e->P, e->D, sel, 0, fused_rm);
    } else if (coop) LAUNCH_EV(done, k_solve, dim3((N + 3) / 4), dim3(256), lds64, st, e->B, e->P, e->D, sel, 1);
    else LAUNCH_EV(done, k_solve, dim3((ngroups + 3) / 4), dim3(256), 4 * lds64, st, e->B, e->P, e->D, sel, 0);
}

// The state part of a step for all envs on the main stream (k_prep_b16 beside k_collide on the side stream when `overlap`): at
// the start of a step whose look-ahead is missing or stale, or at the end of a step that has a single class.
static void state_part_all(rr_env *e, bool overlap) {
    if (overlap) {
        launch_prep_a(e, 0, 1, e->stream, e->ev_fork);
        HIPQ(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
        launch_prep_b(e, 0, e->aux, e->ev_dyn);
        launch_collide(e, 0, e->stream);
        HIPQ(hipStreamWaitEvent(e->stream, e->ev_dyn, 0));
    } else {
        TIMED(0, { launch_prep_a(e, 0, 1, e->stream); launch_prep_b(e, 0, e->stream); });
        TIMED(1, launch_collide(e, 0, e->stream));
    }
}

// Next slot of the pinned ring (allocated on first use: N * 37 bytes per slot = commands + render flags).
static int pin_acquire(rr_env *e, char **slot, int *idx) {
    const int i = e->pin_next;
    e->pin_next = (i + 1) & 3;
    if (!e->pin_buf[i]) {          // buffer and event together or neither
        e->pin_bytes = (size_t)e->P.N * 37;
        hipEvent_t ev = nullptr;
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        const int rc = mem_get(e, {mem_part(&e->pin_buf[i], e->pin_bytes, false, MEM_PINNED)}, "rr_step: allocating the pinned staging ring");
        if (rc != RR_OK) { hipEventDestroy(ev); return rc; }
        e->pin_ev[i] = ev;
    }
    if (e->pin_used[i]) HIPCHK(hipEventSynchronize(e->pin_ev[i]));
    *slot = e->pin_buf[i]; *idx = i;
    return RR_OK;
}

// ---- the schedule of one step --------------------------------------------------------------------------------------------------
// Which of the placements of DESIGN.md 5.2 a step takes, and every launch shape in it, is decided once by plan_step (rr_plan.inc);
// the functions below carry a StepPlan out and decide nothing themselves.

static void launch_light_solve(rr_env *e, const RenderModel *fused_rm, hipStream_t st, hipEvent_t done = nullptr) {
    const size_t lds64 = (size_t)SGRP * LF_TOTAL * sizeof(float);
    LAUNCH_EV(done, k_solve_light_ow, dim3((e->P.N + 15) / 16), dim3(LIGHT_OW_THREADS), 4 * lds64, st, e->B, e->P, e->D, fused_rm);
}

// The same launches as step_split(), one after the other on the main stream, each under its timer -- 2 / 3 / 4 / 6 what the main
// stream runs in an untimed step (the light envs), 7 / 8 what the side streams run beside it, 0 / 1 the look-ahead of the next step.
static int step_split_timed(rr_env *e, const StepPlan &pl, const DevPtrs &D, int restore, bool ahead, int render_mode) {
    TIMED(2, launch_light_solve(e, e->RM_dev, e->stream));
    TIMED(7, { launch_solve_class(e, pl, 2, e->stream, e->RM_dev); launch_solve_class(e, pl, 3, e->stream, e->RM_dev); });
    launch_render_timed(e, D, restore, 1, e->stream, true);
    TIMED(8, { launch_render(e, pl, D, restore, 2, e->stream, true); launch_render(e, pl, D, restore, 3, e->stream, true); });
    if (ahead) {
        TIMED(0, launch_prep_ab(e, 0, e->stream));
        TIMED(1, launch_collide(e, 0, e->stream));
        e->la_valid = true;
    }
    return launch_mirror(e, render_mode != 0);
}

// Placements 1 and 2: the few envs with generic contact rows take several times as long as the others (a solve kernel lasts as
// long as its longest Gauss-Seidel chain).  Main stream: light solve -> visibility -> shading of the light envs; heavy stream:
// heavy solve -> their render (-> the very heavy envs' render); very heavy stream: their solve (-> look-ahead).  Where the
// look-ahead and the very heavy envs' render go was settled by measurement (DESIGN.md 5.2, NOTEBOOK.md B).
// The solve kernels set up the render instances of their envs themselves.
static int step_split(rr_env *e, const StepPlan &pl, const DevPtrs &D, int restore, bool ahead, int render_mode) {
    // (the events that say "this class is solved" / "the collision pass is done" complete with those launches: LAUNCH_EV)
    HIPQ(hipEventRecord(e->ev_fork, e->stream));
    HIPQ(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
    launch_solve_class(e, pl, 2, e->aux, e->RM_dev, ahead ? e->ev_hsolved : nullptr);
    // (ev_join: the heavy stream's last launch -- the heavy lists' render, or the very heavy envs' behind it, or placement 2's collision pass)
    const hipEvent_t join_ev = pl.la_side ? nullptr : e->ev_join;
    launch_render(e, pl, D, restore, 2, e->aux, true, pl.vh_render_on_aux ? nullptr : join_ev);
    HIPQ(hipStreamWaitEvent(e->aux2, e->ev_fork, 0));
    launch_solve_class(e, pl, 3, e->aux2, e->RM_dev, ahead ? e->ev_vsolved : nullptr);
    if (pl.vh_render_on_aux) {
        HIPQ(hipStreamWaitEvent(e->aux, e->ev_vsolved, 0));
        launch_render(e, pl, D, restore, 3, e->aux, true, join_ev);
    } else if (!pl.la_on_vh) launch_render(e, pl, D, restore, 3, e->aux2, true);
    launch_light_solve(e, e->RM_dev, e->stream, ahead ? e->ev_dyn : nullptr);
    if (pl.la_side) {
        // the heavy stream is done with its envs' render long before the very heavy envs' is: the kinematics half of the preparation
        // and the collision pass go there once every solve is done, the dynamics half behind the very heavy envs' render
        HIPQ(hipStreamWaitEvent(e->aux, e->ev_dyn, 0));
        HIPQ(hipStreamWaitEvent(e->aux, e->ev_vsolved, 0));
        launch_prep_a(e, 0, 0, e->aux);
        launch_collide(e, 0, e->aux, e->ev_join);
        HIPQ(hipStreamWaitEvent(e->aux2, e->ev_dyn, 0));
        HIPQ(hipStreamWaitEvent(e->aux2, e->ev_hsolved, 0));
        launch_prep_b(e, 0, e->aux2, e->ev_join2);
    }
    if (pl.la_on_vh) {
        const ImageOut io = env_images(e);
        launch_raster(e, D, restore, 1, e->stream);
        HIPQ(hipEventRecord(e->ev_rast, e->stream));
        HIPQ(hipStreamWaitEvent(e->aux2, e->ev_rast, 0));          // (behind the light solve too: same stream)
        HIPQ(hipStreamWaitEvent(e->aux2, e->ev_hsolved, 0));
        launch_prep_ab(e, 0, e->aux2);
        launch_collide(e, 0, e->aux2, e->ev_join2);
        launch_shade(e, D, io, 1, e->stream);
    } else {
        if (!ahead) HIPQ(hipEventRecord(e->ev_join2, e->aux2));     // (with the look-ahead its last launch completes ev_join2)
        launch_render(e, pl, D, restore, 1, e->stream, true);
    }
    if (pl.vh_render_on_main) {
        HIPQ(hipStreamWaitEvent(e->stream, e->ev_vsolved, 0));
        launch_render(e, pl, D, restore, 3, e->stream, true);
    }
    if (ahead) e->la_valid = true;
    HIPQ(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    HIPQ(hipStreamWaitEvent(e->stream, e->ev_join2, 0));
    return launch_mirror(e, render_mode != 0);
}

// Placements 3, 4 and 5: one class (or a handful of envs).  A single env is solved by the kernel of its own class (a launch whose
// list is empty ends at once); a small batch with a wave for every env; otherwise four envs to a wave (StepPlan::single_solve).
static int step_single(rr_env *e, const StepPlan &pl, bool overlap, bool ahead, int render_mode) {
    const int N = e->P.N;
    const size_t lds64 = (size_t)SGRP * LF_TOTAL * sizeof(float);
    if (pl.single_solve == SOLVE_CHAIN_N1) {
        launch_light_solve(e, nullptr, e->stream);
        launch_solve_class(e, pl, 2, e->stream);
        launch_solve_class(e, pl, 3, e->stream);
    } else if (pl.single_solve == SOLVE_SIDE_BY_SIDE) {          // placement 3b
        HIPQ(hipEventRecord(e->ev_fork, e->stream));
        HIPQ(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
        launch_solve_class(e, pl, 2, e->aux, nullptr, nullptr, false);
        HIPQ(hipEventRecord(e->ev_join, e->aux));
        HIPQ(hipStreamWaitEvent(e->aux2, e->ev_fork, 0));
        launch_solve_class(e, pl, 3, e->aux2, nullptr, nullptr, false);
        HIPQ(hipEventRecord(e->ev_join2, e->aux2));
        launch_light_solve(e, nullptr, e->stream);
        HIPQ(hipStreamWaitEvent(e->stream, e->ev_join, 0));
        HIPQ(hipStreamWaitEvent(e->stream, e->ev_join2, 0));
    } else if (pl.single_solve == SOLVE_WAVE_PER_ENV)
        TIMED(2, hipLaunchKernelGGL(k_solve, dim3((N + 3) / 4), dim3(256), lds64, e->stream, e->B, e->P, e->D, 0, 1));
    else
        TIMED(2, hipLaunchKernelGGL(k_solve, dim3((N + SGRP - 1) / SGRP), dim3(SGRP * 16), lds64, e->stream, e->B, e->P, e->D, 0, 0));
    HIPCHK(hipGetLastError());
    int rc = RR_OK;
    if (pl.la_beside) {
        HIPQ(hipEventRecord(e->ev_fork, e->stream));
        HIPQ(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
        launch_prep_ab(e, 0, e->aux);
        launch_collide(e, 0, e->aux, e->ev_join);
    }
    if (render_mode) rc = do_render(e, render_mode == 2);
    if (pl.la_beside) {
        HIPQ(hipStreamWaitEvent(e->stream, e->ev_join, 0));
        e->la_valid = true;
    } else if (ahead) {
        // (a handful of envs: the observations of this step are complete here -- the mirror goes in front of the look-ahead, so that
        // a caller waiting for the observations alone (rr_sync_observations) gets them 45 us earlier and the state part of the next
        // step runs while the host computes its next action)
        if (pl.small_n) { const int rm = launch_mirror(e, render_mode != 0); if (rm != RR_OK) return rm; launch_prep_ab(e, 0, e->stream); launch_collide(e, 0, e->stream); }
        else state_part_all(e, overlap);
        e->la_valid = true;
    }
    if (!(pl.small_n && ahead && !pl.la_beside)) { const int rm = launch_mirror(e, render_mode != 0); if (rm != RR_OK) return rm; }
    return rc;
}

int rr_step(rr_env *e, const float *joint_cmd, int32_t cmd_on_device, int32_t render_mode, const uint8_t *render_flags_host) {
    if (!e) return fail(RR_EINVAL, "null env");
    if (render_mode < 0 || render_mode > 2 || (render_mode == 2 && !render_flags_host)) return fail(RR_EINVAL, "rr_step: bad render_mode");
    HIPCHK(hipSetDevice(e->cfg.device));
    const int N = e->P.N;
    const bool host_cmd = joint_cmd && !cmd_on_device, host_flags = render_mode == 2;
    char *pin = nullptr; int pin_idx = -1;
    if (host_cmd || host_flags) { const int rc = pin_acquire(e, &pin, &pin_idx); if (rc != RR_OK) return rc; }
    if (!joint_cmd) HIPCHK(hipMemsetAsync(e->D.cmd, 0, (size_t)N * 36, e->stream));      // env.py:333-334
    else if (host_cmd) {
        memcpy(pin, joint_cmd, (size_t)N * 36);
        HIPCHK(hipMemcpyAsync(e->D.cmd, pin, (size_t)N * 36, hipMemcpyHostToDevice, e->stream));
    }
    if (host_flags) {
        memcpy(pin + (size_t)N * 36, render_flags_host, N);
        HIPCHK(hipMemcpyAsync(e->D.render_flags, pin + (size_t)N * 36, N, hipMemcpyHostToDevice, e->stream));
    }
    if (pin_idx >= 0) { HIPCHK(hipEventRecord(e->pin_ev[pin_idx], e->stream)); e->pin_used[pin_idx] = true; }
    const bool overlap = !e->timing;      // side streams in use (timing leg: everything on the main stream)
    // ---- bounded run-ahead (a batch: a handful of envs is waited for every step by its caller anyway)
    const unsigned ahead_period = (unsigned)std::max(1, e->set.run_ahead / 2);
    const bool bounded = e->set.run_ahead > 0 && N > SMALL_N_MAX && e->step_no % ahead_period == 0;      // (a marker step)
    const int ahead_slot = (int)((e->step_no / ahead_period) & 1u);
    if (bounded) {
        if (!e->ahead_ev[ahead_slot]) HIPCHK(hipEventCreateWithFlags(&e->ahead_ev[ahead_slot], hipEventDisableTiming | hipEventDisableSystemFence));
        else HIPCHK(hipEventSynchronize(e->ahead_ev[ahead_slot]));       // (recorded two marker steps = run_ahead steps ago)
    }
    // ---- the state part of this step, unless the previous step already computed it (look-ahead) for exactly this state
    if (!e->la_valid) state_part_all(e, overlap);
    e->cur ^= 1; e->la_valid = false;           // the frame the collision pass filled is the one this step solves
    bind_frames(e);
    // ---- joint torques (rr_torque.inc): qd* += dt M^-1 tau in this step's preparation record.  Here the main stream is behind the
    // whole look-ahead (every step path ends with the main stream waiting for ev_join / ev_join2 or ev_dyn, or ran it on this stream;
    // state_part_all above likewise), and every solve below is on this stream or behind ev_fork recorded on it.  Under no timer.
    if (e->jt_on) hipLaunchKernelGGL(k_joint_torque, dim3((unsigned)((N * 16 + JT_THREADS - 1) / JT_THREADS)), dim3(JT_THREADS), 0, e->stream, e->P, e->D, (const float *)e->jt_table);
    // ---- external wrenches (rr_wrench.inc): their term in the same record, at the same point -- behind the torque term when both are on.
    if (e->xw_on) hipLaunchKernelGGL(k_ext_wrench, dim3((unsigned)((N * 16 + XW_THREADS - 1) / XW_THREADS)), dim3(XW_THREADS), 0, e->stream, e->P, e->D, (const float *)e->xw_table);
    // a device-resident command buffer is read in place by the solve kernels (stream order protects it like a copy would)
    e->D.cmd_in = (joint_cmd && cmd_on_device) ? joint_cmd : e->D.cmd;
    // ---- the plan of this step: the one reading of the lagged list lengths (behind the run-ahead wait: as fresh as it gets)
    PlanIn in;
    in.N = N; in.ntiles = e->RM.ntiles; in.render_mode = render_mode; in.timing = e->timing;
    in.split_heavy = e->set.split_heavy; in.lookahead = e->set.lookahead; in.coop_all = e->set.coop_all;
    in.split_max_pct = e->set.split_max_pct;
    in.counts = lagged_counts(e);
    const StepPlan pl = plan_step(in);
    const bool ahead = e->set.lookahead;            // this step ends with the state part of the next one
    int rc;
    if (pl.path != PATH_SINGLE) {
        DevPtrs D = e->D;
        if (render_mode != 2) D.render_flags = nullptr;
        const int restore = ensure_images(e, D);
        rc = pl.path == PATH_SPLIT_TIMED ? step_split_timed(e, pl, D, restore, ahead, render_mode) : step_split(e, pl, D, restore, ahead, render_mode);
    } else rc = step_single(e, pl, overlap, ahead, render_mode);
    if (rc != RR_OK) return rc;
    HIPCHK(hipGetLastError());
    if (bounded) HIPCHK(hipEventRecord(e->ahead_ev[ahead_slot], e->stream));
    e->step_no++;
    return step_status(e);
}

int rr_render(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    const int rc = do_render(e, false);
    const int rm = launch_mirror(e, true);
    return rc != RR_OK ? rc : rm;
}

int rr_pack_image_delta(rr_env *e, const uint32_t *offsets_dev, uint32_t *records_dev, uint32_t capacity) {
    if (!e || !offsets_dev || !records_dev) return fail(RR_EINVAL, "rr_pack_image_delta: null argument");
    if (!e->D.frag_list || !e->images_valid) return fail(RR_EINVAL, "rr_pack_image_delta: nothing rendered yet");
    if ((unsigned long long)e->P.N * e->RM.W * e->RM.H >= (1ull << 32)) return fail(RR_EINVAL, "rr_pack_image_delta: more than 2^32 pixels per handle (32-bit pixel addresses in the records)");
    HIPCHK(hipSetDevice(e->cfg.device));
    hipLaunchKernelGGL(k_pack_delta, dim3(e->P.N, e->RM.ntiles), dim3(256), 0, e->stream, e->RM_dev, e->D, env_images(e), offsets_dev, (uint3 *)records_dev, capacity);
    HIPCHK(hipGetLastError());
    return RR_OK;
}
int rr_apply_image_delta(const uint32_t *records_dev, const uint32_t *totals_dev, int32_t world, uint32_t capacity, size_t pixels_per_rank,
                         uint8_t *rgb_dev, float *depth_dev, void *stream) {
    if (!records_dev || !totals_dev || !rgb_dev || !depth_dev || world < 1) return fail(RR_EINVAL, "rr_apply_image_delta: bad argument");
    if (capacity == 0) return RR_OK;
    const size_t total = (size_t)world * capacity;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(k_apply_delta, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint3 *)records_dev, totals_dev, world, capacity, pixels_per_rank, rgb_dev, depth_dev);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// The three buffers of rr_contact_observations (RR_F_CONTACTS, RR_F_BODY_FORCE, RR_F_BODY_PARTNERS): allocated on first use -- by the
// call or by rr_get_buffer / rr_copy_to_host of one of the fields --, zero-filled.
static int ensure_contact_obs(rr_env *e) {
    if (e->co_contacts) return RR_OK;
    if (e->RM.nl + NOBJ != RR_CONTACT_ROWS) return fail(RR_EMODEL, "rr_contact_observations: the model's link count + 3 objects is not RR_CONTACT_ROWS");
    HIPCHK(hipSetDevice(e->cfg.device));
    RRCHK(mem_get(e, {mem_part(&e->co_contacts, e->field_bytes[RR_F_CONTACTS]), mem_part(&e->co_force, e->field_bytes[RR_F_BODY_FORCE]),
                      mem_part(&e->co_partners, e->field_bytes[RR_F_BODY_PARTNERS])}, "rr_contact_observations: allocating the observation buffers"));
    e->field_ptr[RR_F_CONTACTS] = e->co_contacts; e->field_ptr[RR_F_BODY_FORCE] = e->co_force; e->field_ptr[RR_F_BODY_PARTNERS] = e->co_partners;
    return RR_OK;
}
static inline bool contact_obs_field(int32_t field) { return field == RR_F_CONTACTS || field == RR_F_BODY_FORCE || field == RR_F_BODY_PARTNERS; }

// Kuka.get_contacts (robot.py:131-150) for the whole batch, on the device.  Ordered like rr_get_contacts' copies: on the main stream,
// which every rr_step has made wait for its side streams (ev_join / ev_join2) before it returns -- behind everything that wrote
// clist / cforce / ccount of the current frame; the look-ahead's frame (clist_next) is not read.
int rr_contact_observations(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "null env");
    const int rc = ensure_contact_obs(e);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    hipLaunchKernelGGL(k_contact_obs, dim3((e->P.N + CO_ENVS - 1) / CO_ENVS), dim3(64 * CO_ENVS), 0, e->stream, e->P, e->D, e->RM.nl,
                       e->co_contacts, e->co_force, e->co_partners);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// ---- the on-demand groups of the queries and step inputs ---------------------------------------------------------------------------------
// One group on first use: the buffers of a query family (family >= 0, while it has none), for its capacity and zero-filled, and
// every part of `more` whose pointer is still null (a null ptr: a part the call does not need) -- staging blocks, tables -- in ONE
// list, all or nothing.  `up`: a host table whose device copy is a part of the list goes up behind the allocation; if that fails the
// whole list is given back, every pointer null again.
struct GroupUpload { void **dst; const void *src; size_t bytes; const char *name; };
static int ensure_group(rr_env *e, int family, const char *who, const char *what, std::initializer_list<MemPart> more, const GroupUpload *up = nullptr) {
    MemPart parts[QUERY_MAX_BUFFERS + 4];
    size_t n = 0;
    if (family >= 0 && !e->qbuf[family][0]) {
        const QueryDims cap = query_capacity(family, (size_t)e->P.N, (size_t)e->P.nobj);
        for (int i = 0; i < QUERY_FAMILIES[family].count; i++) parts[n++] = mem_part(&e->qbuf[family][i], query_bytes(family, i, cap));
    }
    for (const MemPart &m : more)
        if (m.ptr && !*m.ptr) parts[n++] = m;
    if (!n) return RR_OK;
    const bool upload = up && !*up->dst;
    HIPCHK(hipSetDevice(e->cfg.device));
    RRCHK(mem_get(e, parts, n, (std::string(who) + ": allocating " + what).c_str()));
    if (!upload) return RR_OK;
    hipError_t rc = hipMemcpyAsync(*up->dst, up->src, up->bytes, hipMemcpyHostToDevice, e->stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(e->stream);      // (the source is the handle's own memory)
    if (rc == hipSuccess) return RR_OK;
    (void)hipStreamSynchronize(e->stream);
    for (size_t i = 0; i < n; i++) e->mem.release(*parts[i].ptr);
    (void)hipGetLastError();
    return fail(RR_EDEVICE, std::string(who) + ": uploading " + up->name + ": " + hipGetErrorString(rc));
}
static inline MemPart stage_part(float **ptr, size_t bytes, bool wanted = true) { return wanted ? mem_part(ptr, bytes, false) : MemPart{}; }
// the staging of a host caller's postures [N, RR_PC_MAX_POSTURES, 11], shared by every query that takes postures
static inline MemPart posture_stage(rr_env *e, bool wanted) { return stage_part(&e->pc_stage, (size_t)e->P.N * RR_PC_MAX_POSTURES * 44, wanted); }

// The model condition of the kernels that read the link table of rr_link_poses: 17 URDF links, every one on a body of the tree.
// `code`: the kinematic observations and the ray casts answer RR_EMODEL, the queries at candidate postures RR_EINVAL -- an
// inconsistency of the ABI, kept as it is.
static int check_link_table(const rr_env *e, const char *who, int code) {
    if (e->RM.nl != KIN_LINKS) return fail(code, std::string(who) + ": the model does not have the 17 URDF links of rr_link_poses");
    for (int l = 0; l < KIN_LINKS; l++)
        if (e->RM.link_body[l] >= NB) return fail(code, std::string(who) + ": link " + std::to_string(l) + " of the model is on a body outside the kinematic tree");
    return RR_OK;
}

// The group of a query family on first use -- by the query or by its buffer / copy_to_host --: its buffers, the device copy of the
// table it reads (the table in force goes up behind the allocation), and the staging blocks of `stages` the call still lacks.
static_assert(QRY_JOINTS == NB && QRY_LINKS == KIN_LINKS, "rr_query.inc restates the model's constants");
static int ensure_query(rr_env *e, int family, const char *who, std::initializer_list<MemPart> stages = {}) {
    static const char *const what[QF_COUNT] = {"the observation buffers", "the ray buffers", "the distance buffers", "the posture buffers", "the signed-distance buffers",
                                               "the signed-gradient buffers", "the sweep buffers", "the posture kinematics buffers", "the posture IK buffers",
                                               "the posture dynamics buffers"};
    MemPart more[3] = {};
    size_t n = 0;
    for (const MemPart &m : stages) more[n++] = m;
    GroupUpload up = {};
    switch (family) {
    case QF_KIN:
        RRCHK(check_link_table(e, who, RR_EMODEL));
        more[n] = mem_part(&e->kin_pts_dev, sizeof(KinPoints), false);
        up = {(void **)&e->kin_pts_dev, &e->kin_pts, sizeof(KinPoints), "the points"};
        break;
    case QF_RAY:
        RRCHK(check_link_table(e, who, RR_EMODEL));
        memcpy(e->ray_tab.uid, e->shape_uid, sizeof e->ray_tab.uid);
        more[n++] = stage_part(&e->ray_stage, (size_t)e->P.N * RR_RAY_MAX * 24);
        more[n] = mem_part(&e->ray_tab_dev, sizeof(RayTable), false);
        up = {(void **)&e->ray_tab_dev, &e->ray_tab, sizeof(RayTable), "the ray table"};
        break;
    case QF_DIST:
        more[n] = mem_part(&e->dist_tab_dev, sizeof(DistTable), false);
        up = {(void **)&e->dist_tab_dev, &e->dist_tab, sizeof(DistTable), "the pair table"};
        break;
    case QF_SW:
        more[n] = mem_part(&e->sw_reach_dev, sizeof(SweepReach), false);
        up = {(void **)&e->sw_reach_dev, &e->sweep_reach, sizeof(SweepReach), "the reach table"};
        break;
    case QF_PK: case QF_PIK:
        RRCHK(check_link_table(e, who, RR_EINVAL));
        break;
    }
    return ensure_group(e, family, who, what[family], {more[0], more[1], more[2]}, up.dst ? &up : nullptr);
}

// A host caller's tensors on their way to a kernel: each goes to the stage of its kind on the main stream, the kernel reads the
// stage, and the call waits at its end because the arguments are host memory.  host == false: device tensors, read in place.
struct HostStaging {
    rr_env *e; bool host;
    int in(const float *&tensor, float *stage, size_t bytes) const {
        if (!host || !tensor) return RR_OK;
        HIPCHK(hipMemcpyAsync(stage, tensor, bytes, hipMemcpyHostToDevice, e->stream));
        tensor = stage;
        return RR_OK;
    }
    int wait() const { if (host) HIPCHK(hipStreamSynchronize(e->stream)); return RR_OK; }
};

// The HIP side of the two accessors of rr_query.inc and the view of a handle they work on: the layout in force is the last call's K
// with the table's Q and the points' -- for the ray casts the rays' -- P.
static int hip_query_ensure(void *env, int family, const char *who) { return ensure_query((rr_env *)env, family, who); }
static int hip_query_copy(void *env, void *dst, const void *src, size_t bytes) {
    rr_env *e = (rr_env *)env;
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}
static const QueryBackend HIP_QUERY = {hip_query_ensure, hip_query_copy, fail};
static QueryView query_view(rr_env *e, int family) {
    if (!e) return QueryView{nullptr, family, nullptr, {}};
    return QueryView{e, family, e->qbuf[family],
                     {{(size_t)e->P.N, (size_t)e->qk[family], (size_t)e->dist_n, (size_t)(family == QF_RAY ? e->ray_n : e->kin_np), (size_t)e->P.nobj}}};
}
int rr_set_kinematic_points(rr_env *e, int32_t n_points, const int32_t *link, const float *local_pos) {
    if (!e) return fail(RR_EINVAL, "rr_set_kinematic_points: null env");
    if (n_points < 1 || n_points > RR_KIN_MAX_POINTS)
        return fail(RR_EINVAL, n_points < 1 ? "rr_set_kinematic_points: n_points " + std::to_string(n_points) + ": point 0 is missing (at least one point)"
                                            : "rr_set_kinematic_points: n_points " + std::to_string(n_points) + ": point " + std::to_string(RR_KIN_MAX_POINTS) +
                                                  " is beyond RR_KIN_MAX_POINTS (" + std::to_string(RR_KIN_MAX_POINTS) + ")");
    if (!link) return fail(RR_EINVAL, "rr_set_kinematic_points: null link array");
    KinPoints K = {};
    for (int j = 0; j < n_points; j++) {
        if (link[j] < 0 || link[j] >= KIN_LINKS)
            return fail(RR_EINVAL, "rr_set_kinematic_points: point " + std::to_string(j) + ": link " + std::to_string(link[j]) + " is not in [0, " + std::to_string(KIN_LINKS) + ")");
        K.link[j] = link[j];
        for (int k = 0; k < 3; k++) {
            const float v = local_pos ? local_pos[3 * j + k] : 0.0f;
            if (!std::isfinite(v)) return fail(RR_EINVAL, "rr_set_kinematic_points: point " + std::to_string(j) + ": local_pos is not finite");
            K.local[j][k] = v;
        }
    }
    if (e->kin_pts_dev) {      // (before the buffers exist the host copy is all there is: ensure_query uploads it)
        HIPCHK(hipSetDevice(e->cfg.device));
        HIPCHK(hipStreamSynchronize(e->stream));      // an observation call enqueued earlier still reads the earlier points
        HIPCHK(hipMemcpy(e->kin_pts_dev, &K, sizeof K, hipMemcpyHostToDevice));
    }
    e->kin_pts = K; e->kin_np = n_points;
    return RR_OK;
}

int rr_get_kinematic_points(rr_env *e, int32_t *n_points, int32_t *link_out, float *local_pos_out) {
    if (!e) return fail(RR_EINVAL, "rr_get_kinematic_points: null env");
    if (n_points) *n_points = e->kin_np;
    if (link_out) memcpy(link_out, e->kin_pts.link, (size_t)e->kin_np * 4);
    if (local_pos_out) memcpy(local_pos_out, e->kin_pts.local, (size_t)e->kin_np * 12);
    return RR_OK;
}

// getJointState / getLinkState / getBaseVelocity / calculateJacobian for the whole batch, on the device.  On the main stream like
// rr_contact_observations: behind every step, reset and state upload enqueued before it (every rr_step has made that stream wait for
// its side streams before it returns).  Reads D.state only -- never the scratch slab of the look-ahead -- and leaves la_valid alone.
int rr_kinematic_observations(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "rr_kinematic_observations: null env");
    RRCHK(ensure_query(e, QF_KIN, "rr_kinematic_observations"));
    HIPCHK(hipSetDevice(e->cfg.device));
    float *const *b = (float *const *)e->qbuf[QF_KIN];
    const KinOut O = {b[RR_KIN_JOINT_VEL], b[RR_KIN_LINK_POSE], b[RR_KIN_LINK_VEL], b[RR_KIN_OBJ_VEL], b[RR_KIN_POINT_POS], b[RR_KIN_POINT_VEL], b[RR_KIN_JACOBIAN]};
    hipLaunchKernelGGL(k_kinematics, dim3((e->P.N + KIN_ENVS - 1) / KIN_ENVS), dim3(KIN_THREADS), 0, e->stream, e->B, e->P, e->RM_dev, e->D, O,
                       e->kin_pts_dev, e->kin_np);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_kinematic_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_KIN), HIP_QUERY, which, dev_ptr, bytes); }
int rr_kinematic_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_KIN), HIP_QUERY, which, dst, bytes); }

// ---- ray casts against the collision hulls (rr_ray.inc) ---------------------------------------------------------------------------------
int rr_set_rays(rr_env *e, int32_t n_rays, const int32_t *link, const float *from_to) {
    if (!e) return fail(RR_EINVAL, "rr_set_rays: null env");
    if (n_rays < 0 || n_rays > RR_RAY_MAX)
        return fail(RR_EINVAL, n_rays < 0 ? "rr_set_rays: n_rays " + std::to_string(n_rays) + " is negative"
                                          : "rr_set_rays: n_rays " + std::to_string(n_rays) + ": ray " + std::to_string(RR_RAY_MAX) + " is beyond RR_RAY_MAX (" +
                                                std::to_string(RR_RAY_MAX) + ")");
    if (n_rays > 0 && !link) return fail(RR_EINVAL, "rr_set_rays: null link array");
    RayTable T = {};
    memcpy(T.uid, e->shape_uid, sizeof T.uid);
    for (int j = 0; j < n_rays; j++) {
        if (link[j] < -1 || link[j] >= KIN_LINKS)
            return fail(RR_EINVAL, "rr_set_rays: ray " + std::to_string(j) + ": link " + std::to_string(link[j]) + " is neither -1 (the world) nor in [0, " + std::to_string(KIN_LINKS) + ")");
        T.link[j] = link[j];
        for (int k = 0; k < 6; k++) {
            const float v = from_to ? from_to[6 * j + k] : 0.0f;
            if (!std::isfinite(v)) return fail(RR_EINVAL, "rr_set_rays: ray " + std::to_string(j) + ": from_to is not finite");
            T.seg[j][k] = v;
        }
    }
    for (int j = n_rays; j < RR_RAY_MAX; j++) T.link[j] = -1;
    if (e->ray_tab_dev) {      // (before the buffers exist the host copy is all there is: ensure_query uploads it)
        HIPCHK(hipSetDevice(e->cfg.device));
        HIPCHK(hipStreamSynchronize(e->stream));      // a cast enqueued earlier still reads the earlier table
        HIPCHK(hipMemcpy(e->ray_tab_dev, &T, sizeof T, hipMemcpyHostToDevice));
    }
    e->ray_tab = T; e->ray_n = n_rays;
    return RR_OK;
}

int rr_get_rays(rr_env *e, int32_t *n_rays, int32_t *link_out, float *from_to_out) {
    if (!e) return fail(RR_EINVAL, "rr_get_rays: null env");
    if (n_rays) *n_rays = e->ray_n;
    if (link_out) memcpy(link_out, e->ray_tab.link, (size_t)e->ray_n * 4);
    if (from_to_out) memcpy(from_to_out, e->ray_tab.seg, (size_t)e->ray_n * 24);
    return RR_OK;
}

// rayTestBatch for the whole batch, on the device.  On the main stream like rr_kinematic_observations: behind every step, reset and
// state write enqueued before it.  Reads D.state and the model only -- never the scratch slab of the look-ahead -- and leaves la_valid
// and the error flags alone.
int rr_ray_cast(rr_env *e, const float *rays, int32_t on_device) {
    if (!e) return fail(RR_EINVAL, "rr_ray_cast: null env");
    const int R = e->ray_n, N = e->P.N;
    if (R == 0) return fail(RR_EINVAL, "rr_ray_cast: the ray table is empty (rr_set_rays)");
    if (rays && !on_device)
        for (size_t i = 0; i < (size_t)N * R * 6; i++)
            if (!std::isfinite(rays[i]))
                return fail(RR_EINVAL, "rr_ray_cast: env " + std::to_string(i / ((size_t)R * 6)) + ", ray " + std::to_string(i / 6 % R) + ": the segment is not finite");
    RRCHK(ensure_query(e, QF_RAY, "rr_ray_cast"));
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, rays && !on_device};
    const float *seg = rays;
    RRCHK(st.in(seg, e->ray_stage, (size_t)N * R * 24));
    hipLaunchKernelGGL(k_ray_cast, dim3((N + RAY_ENVS - 1) / RAY_ENVS), dim3(RAY_THREADS), 0, e->stream, e->B, e->P, e->RM_dev, e->D, e->n_shapes,
                       e->ray_tab_dev, seg, R, (float4 *)e->qbuf[QF_RAY][RR_RAY_HIT], (int4 *)e->qbuf[QF_RAY][RR_RAY_ID]);
    HIPCHK(hipGetLastError());
    return st.wait();
}

int rr_ray_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_RAY), HIP_QUERY, which, dev_ptr, bytes); }
int rr_ray_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_RAY), HIP_QUERY, which, dst, bytes); }

// ---- closest points between collision hulls (rr_dist.inc) ------------------------------------------------------------------------------
int rr_set_distance_pairs(rr_env *e, int32_t n_pairs, const int32_t *shape_a, const int32_t *shape_b, float max_distance) {
    if (!e) return fail(RR_EINVAL, "rr_set_distance_pairs: null env");
    if (n_pairs < -1 || n_pairs > RR_DIST_MAX)
        return fail(RR_EINVAL, n_pairs < 0 ? "rr_set_distance_pairs: n_pairs " + std::to_string(n_pairs) + " is neither -1 (the step's collision pairs) nor a count"
                                           : "rr_set_distance_pairs: n_pairs " + std::to_string(n_pairs) + ": pair " + std::to_string(RR_DIST_MAX) +
                                                 " is beyond RR_DIST_MAX (" + std::to_string(RR_DIST_MAX) + ")");
    if (std::isnan(max_distance)) return fail(RR_EINVAL, "rr_set_distance_pairs: max_distance is NaN");
    static_assert(RR_DIST_MAX == MAXPAIRS, "the step's whole collision table fits the pair table");
    const bool own = n_pairs == -1;
    const int Q = own ? e->P.npairs : n_pairs;
    if (!own && Q > 0 && (!shape_a || !shape_b)) return fail(RR_EINVAL, "rr_set_distance_pairs: null shape array");
    DistTable T = {};
    T.max_distance = max_distance;
    for (int j = 0; j < Q; j++) {
        const int ab[2] = {own ? e->pair_shapes[2 * j] : shape_a[j], own ? e->pair_shapes[2 * j + 1] : shape_b[j]};
        for (int k = 0; k < 2; k++) {
            const std::string which = "rr_set_distance_pairs: pair " + std::to_string(j) + ": shape " + (k ? "b" : "a") + " = " + std::to_string(ab[k]);
            if (ab[k] < 0 || ab[k] >= e->n_shapes) return fail(RR_EINVAL, which + " is not in [0, " + std::to_string(e->n_shapes) + ")");
            if (e->shape_kind[ab[k]] == 2 && (e->shape_idx[ab[k]] < 0 || e->shape_idx[ab[k]] >= e->P.nobj))
                return fail(RR_EINVAL, which + " belongs to object " + std::to_string(e->shape_idx[ab[k]]) + ", which this handle (" + std::to_string(e->P.nobj) + " objects) does not have");
            if (e->shape_kind[ab[k]] == 1 && (e->shape_idx[ab[k]] < 0 || e->shape_idx[ab[k]] >= NB))
                return fail(RR_EMODEL, which + " is on a body outside the kinematic tree");
        }
        if (ab[0] == ab[1]) return fail(RR_EINVAL, "rr_set_distance_pairs: pair " + std::to_string(j) + ": a == b (shape " + std::to_string(ab[0]) + ")");
        T.a[j] = ab[0]; T.b[j] = ab[1];
    }
    if (e->dist_tab_dev) {     // (before the buffers exist the host copy is all there is: ensure_query uploads it)
        HIPCHK(hipSetDevice(e->cfg.device));
        HIPCHK(hipStreamSynchronize(e->stream));      // a query enqueued earlier still reads the earlier table
        HIPCHK(hipMemcpy(e->dist_tab_dev, &T, sizeof T, hipMemcpyHostToDevice));
    }
    e->dist_tab = T; e->dist_n = Q;
    return RR_OK;
}

int rr_get_distance_pairs(rr_env *e, int32_t *n_pairs, int32_t *shape_a_out, int32_t *shape_b_out, float *max_distance_out) {
    if (!e) return fail(RR_EINVAL, "rr_get_distance_pairs: null env");
    if (n_pairs) *n_pairs = e->dist_n;
    if (shape_a_out) memcpy(shape_a_out, e->dist_tab.a, (size_t)e->dist_n * 4);
    if (shape_b_out) memcpy(shape_b_out, e->dist_tab.b, (size_t)e->dist_n * 4);
    if (max_distance_out) *max_distance_out = e->dist_tab.max_distance;
    return RR_OK;
}

// getClosestPoints for the whole batch, on the device.  On the main stream like rr_ray_cast: behind every step, reset and state write
// enqueued before it.  Reads D.state and the model only -- never the scratch slab of the look-ahead -- and leaves la_valid and the
// error flags alone.
int rr_closest_points(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "rr_closest_points: null env");
    const int Q = e->dist_n, N = e->P.N;
    if (Q == 0) return fail(RR_EINVAL, "rr_closest_points: the pair table is empty (rr_set_distance_pairs)");
    RRCHK(ensure_query(e, QF_DIST, "rr_closest_points"));
    HIPCHK(hipSetDevice(e->cfg.device));
    hipLaunchKernelGGL(k_closest_points, dim3((N + DIST_ENVS - 1) / DIST_ENVS), dim3(DIST_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q,
                       (float4 *)e->qbuf[QF_DIST][RR_DIST_POINTS], (int4 *)e->qbuf[QF_DIST][RR_DIST_ID]);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_distance_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_DIST), HIP_QUERY, which, dev_ptr, bytes); }
int rr_distance_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_DIST), HIP_QUERY, which, dst, bytes); }

// ---- clearance at candidate postures (rr_posture.inc) ----------------------------------------------------------------------------------
// The clearance of K candidate postures per env, on the device.  On the main stream like rr_closest_points: behind every step, reset
// and state write enqueued before it.  Reads D.state (the objects), the model, the pair table and the tensor; writes the four buffers
// and nothing else -- not the state, the scratch slab of the look-ahead, la_valid, an error flag or an RR_DIST_* buffer.
int rr_posture_clearance(rr_env *e, const float *postures, int32_t n_postures, int32_t on_device) {
    if (!e) return fail(RR_EINVAL, "rr_posture_clearance: null env");
    if (!postures) return fail(RR_EINVAL, "rr_posture_clearance: null postures");
    if (n_postures < 1 || n_postures > RR_PC_MAX_POSTURES)
        return fail(RR_EINVAL, "rr_posture_clearance: n_postures " + std::to_string(n_postures) + " is not in [1, RR_PC_MAX_POSTURES = " +
                                   std::to_string(RR_PC_MAX_POSTURES) + "]");
    const int Q = e->dist_n, N = e->P.N, K = n_postures;
    if (Q == 0) return fail(RR_EINVAL, "rr_posture_clearance: the pair table is empty (rr_set_distance_pairs)");
    RRCHK(ensure_query(e, QF_DIST, "rr_posture_clearance"));     // (the device copy of the pair table)
    RRCHK(ensure_query(e, QF_PC, "rr_posture_clearance", {posture_stage(e, !on_device)}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, !on_device};
    const float *src = postures;
    RRCHK(st.in(src, e->pc_stage, (size_t)N * K * 44));
    void *const *b = e->qbuf[QF_PC];
    if (e->att_on)      // objects are attached to links (rr_set_attachments): the CARRY instantiation, the same buffers
        hipLaunchKernelGGL(k_posture_clearance<true>, dim3((unsigned)N * K), dim3(PC_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, src, K,
                           (float4 *)b[RR_PC_NEAREST], (int4 *)b[RR_PC_ID], (float *)b[RR_PC_DISTANCE], (int *)b[RR_PC_STATUS], (const float *)e->att_table);
    else
        hipLaunchKernelGGL(k_posture_clearance<false>, dim3((unsigned)N * K), dim3(PC_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, src, K,
                           (float4 *)b[RR_PC_NEAREST], (int4 *)b[RR_PC_ID], (float *)b[RR_PC_DISTANCE], (int *)b[RR_PC_STATUS], (const float *)nullptr);
    HIPCHK(hipGetLastError());
    e->qk[QF_PC] = K;
    return st.wait();
}

int rr_posture_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_PC), HIP_QUERY, which, dev_ptr, bytes); }
int rr_posture_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_PC), HIP_QUERY, which, dst, bytes); }

// ---- signed distance and penetration depth (rr_signed.inc) -----------------------------------------------------------------------------
// The signed distance of the pair table at the present state (postures == NULL) or at K candidate postures per env.  On the main stream
// like rr_posture_clearance: behind every step, reset and state write enqueued before it.  Reads D.state, the model, the pair table and
// the tensor; writes the five buffers (RR_SD_POINTS at the present state only) and nothing else -- not the state, the scratch slab of
// the look-ahead, la_valid, an error flag or an RR_DIST_* / RR_PC_* buffer.
int rr_signed_distance(rr_env *e, const float *postures, int32_t n_postures, int32_t on_device) {
    if (!e) return fail(RR_EINVAL, "rr_signed_distance: null env");
    if (!postures && n_postures != 0)
        return fail(RR_EINVAL, "rr_signed_distance: null postures with n_postures " + std::to_string(n_postures) + " (the present state is NULL with 0)");
    if (postures && (n_postures < 1 || n_postures > RR_PC_MAX_POSTURES))
        return fail(RR_EINVAL, "rr_signed_distance: n_postures " + std::to_string(n_postures) + " is not in [1, RR_PC_MAX_POSTURES = " +
                                   std::to_string(RR_PC_MAX_POSTURES) + "]");
    const int Q = e->dist_n, N = e->P.N, K = postures ? n_postures : 1;
    if (Q == 0) return fail(RR_EINVAL, "rr_signed_distance: the pair table is empty (rr_set_distance_pairs)");
    const HostStaging st = {e, postures && !on_device};
    RRCHK(ensure_query(e, QF_DIST, "rr_signed_distance"));       // (the device copy of the pair table)
    RRCHK(ensure_query(e, QF_SD, "rr_signed_distance", {posture_stage(e, st.host)}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const float *src = postures;
    RRCHK(st.in(src, e->pc_stage, (size_t)N * K * 44));
    void *const *b = e->qbuf[QF_SD];
    if (e->att_on)      // objects are attached to links (rr_set_attachments): the CARRY instantiation, the same buffers
        hipLaunchKernelGGL(k_signed_distance<true>, dim3((unsigned)N * K), dim3(SD_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, src, K,
                           (float4 *)b[RR_SD_DEEPEST], (int4 *)b[RR_SD_ID], (float *)b[RR_SD_SIGNED], (int *)b[RR_SD_STATUS],
                           postures ? (float4 *)nullptr : (float4 *)b[RR_SD_POINTS], (const float *)e->att_table);
    else
        hipLaunchKernelGGL(k_signed_distance<false>, dim3((unsigned)N * K), dim3(SD_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, src, K,
                           (float4 *)b[RR_SD_DEEPEST], (int4 *)b[RR_SD_ID], (float *)b[RR_SD_SIGNED], (int *)b[RR_SD_STATUS],
                           postures ? (float4 *)nullptr : (float4 *)b[RR_SD_POINTS], (const float *)nullptr);
    HIPCHK(hipGetLastError());
    e->qk[QF_SD] = K;
    return st.wait();
}

int rr_signed_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_SD), HIP_QUERY, which, dev_ptr, bytes); }
int rr_signed_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_SD), HIP_QUERY, which, dst, bytes); }

// ---- joint gradients of the signed distance (rr_grad.inc) ------------------------------------------------------------------------------
// rr_signed_distance with the joint gradients: the same launch shape on the main stream, the same reads, and the five RR_SD_* buffers
// written as that call writes them; the three RR_SG_* buffers (RR_SG_PAIR_GRADIENT at the present state only) in addition, and
// nothing else.
int rr_signed_gradient(rr_env *e, const float *postures, int32_t n_postures, int32_t on_device, float margin) {
    if (!e) return fail(RR_EINVAL, "rr_signed_gradient: null env");
    if (!postures && n_postures != 0)
        return fail(RR_EINVAL, "rr_signed_gradient: null postures with n_postures " + std::to_string(n_postures) + " (the present state is NULL with 0)");
    if (postures && (n_postures < 1 || n_postures > RR_PC_MAX_POSTURES))
        return fail(RR_EINVAL, "rr_signed_gradient: n_postures " + std::to_string(n_postures) + " is not in [1, RR_PC_MAX_POSTURES = " +
                                   std::to_string(RR_PC_MAX_POSTURES) + "]");
    if (!(margin >= 0.0f) || std::isinf(margin)) return fail(RR_EINVAL, "rr_signed_gradient: margin " + std::to_string(margin) + " is not a finite number >= 0");
    const int Q = e->dist_n, N = e->P.N, K = postures ? n_postures : 1;
    if (Q == 0) return fail(RR_EINVAL, "rr_signed_gradient: the pair table is empty (rr_set_distance_pairs)");
    const float maxd = e->dist_tab.max_distance;
    if (maxd > 0.0f && maxd < INFINITY && margin > maxd)
        return fail(RR_EINVAL, "rr_signed_gradient: margin " + std::to_string(margin) + " is above the pair table's max_distance " + std::to_string(maxd) +
                                   " (a culled pair's sphere gap would enter the hinge as a distance)");
    const HostStaging st = {e, postures && !on_device};
    RRCHK(ensure_query(e, QF_DIST, "rr_signed_gradient"));       // (the device copy of the pair table)
    RRCHK(ensure_query(e, QF_SD, "rr_signed_gradient"));
    RRCHK(ensure_query(e, QF_SG, "rr_signed_gradient", {posture_stage(e, st.host)}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const float *src = postures;
    RRCHK(st.in(src, e->pc_stage, (size_t)N * K * 44));
    void *const *b = e->qbuf[QF_SD], *const *g = e->qbuf[QF_SG];
    if (e->att_on)      // objects are attached to links (rr_set_attachments): the CARRY instantiation, the same buffers
        hipLaunchKernelGGL(k_signed_gradient<true>, dim3((unsigned)N * K), dim3(SD_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, src, K,
                           (float4 *)b[RR_SD_DEEPEST], (int4 *)b[RR_SD_ID], (float *)b[RR_SD_SIGNED], (int *)b[RR_SD_STATUS],
                           postures ? (float4 *)nullptr : (float4 *)b[RR_SD_POINTS], margin,
                           (float *)g[RR_SG_GRADIENT], (float *)g[RR_SG_COST], postures ? (float *)nullptr : (float *)g[RR_SG_PAIR_GRADIENT],
                           (const float *)e->att_table);
    else
        hipLaunchKernelGGL(k_signed_gradient<false>, dim3((unsigned)N * K), dim3(SD_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, src, K,
                           (float4 *)b[RR_SD_DEEPEST], (int4 *)b[RR_SD_ID], (float *)b[RR_SD_SIGNED], (int *)b[RR_SD_STATUS],
                           postures ? (float4 *)nullptr : (float4 *)b[RR_SD_POINTS], margin,
                           (float *)g[RR_SG_GRADIENT], (float *)g[RR_SG_COST], postures ? (float *)nullptr : (float *)g[RR_SG_PAIR_GRADIENT],
                           (const float *)nullptr);
    HIPCHK(hipGetLastError());
    e->qk[QF_SD] = e->qk[QF_SG] = K;
    return st.wait();
}

int rr_signed_gradient_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_SG), HIP_QUERY, which, dev_ptr, bytes); }
int rr_signed_gradient_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_SG), HIP_QUERY, which, dst, bytes); }

// ---- swept clearance along joint-space segments (rr_sweep.inc) -------------------------------------------------------------------------
// the refusals rr_swept_clearance and rr_carried_sweep share, each under the name of the entry point that was called
static int sweep_arguments(rr_env *e, const std::string &who, const float *segments, int32_t n_segments, float safety, float tolerance) {
    if (!segments) return fail(RR_EINVAL, who + ": null segments");
    if (n_segments < 1 || n_segments > RR_PC_MAX_POSTURES)
        return fail(RR_EINVAL, who + ": n_segments " + std::to_string(n_segments) + " is not in [1, RR_PC_MAX_POSTURES = " + std::to_string(RR_PC_MAX_POSTURES) + "]");
    if (e->dist_n == 0) return fail(RR_EINVAL, who + ": the pair table is empty (rr_set_distance_pairs)");
    if (!(safety >= 0.0f) || !std::isfinite(safety)) return fail(RR_EINVAL, who + ": safety " + std::to_string(safety) + " is not a finite number >= 0");
    if (!(tolerance >= 1e-6f) || !std::isfinite(tolerance)) return fail(RR_EINVAL, who + ": tolerance " + std::to_string(tolerance) + " is not a finite number >= 1e-6");
    const float maxd = e->dist_tab.max_distance;
    if (maxd > 0.0f && maxd < INFINITY && maxd < safety + tolerance)
        return fail(RR_EINVAL, who + ": the cull's max_distance " + std::to_string(maxd) + " is below safety + tolerance = " + std::to_string(safety + tolerance) +
                                   ": a culled pair's sphere gap could fake a hit");
    return RR_OK;
}
// Conservative advancement along K segments per env, on the device.  On the main stream like rr_posture_clearance: behind every step,
// reset and state write enqueued before it.  Reads D.state (the objects), the model, the pair table, the reach table and the tensor;
// writes the four buffers and nothing else -- not the state, the scratch slab of the look-ahead, la_valid, an error flag or a buffer of
// another query.
int rr_swept_clearance(rr_env *e, const float *segments, int32_t n_segments, int32_t on_device, float safety, float tolerance) {
    if (!e) return fail(RR_EINVAL, "rr_swept_clearance: null env");
    RRCHK(sweep_arguments(e, "rr_swept_clearance", segments, n_segments, safety, tolerance));
    const int Q = e->dist_n, N = e->P.N, K = n_segments;
    if (e->att_on)      // the proof's reach table is a constant of the model and the objects are staged once per row: a carried object would be swept past
        return fail(RR_EINVAL, "rr_swept_clearance: objects are attached to links (rr_set_attachments): the sweep does not move carried objects; "
                               "detach them (rr_set_attachments with link NULL and no mask) or use rr_carried_sweep, which does");
    RRCHK(ensure_query(e, QF_DIST, "rr_swept_clearance"));       // (the device copy of the pair table)
    RRCHK(ensure_query(e, QF_SW, "rr_swept_clearance", {stage_part(&e->sw_stage, (size_t)N * RR_PC_MAX_POSTURES * 88, !on_device)}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, !on_device};
    const float *src = segments;
    RRCHK(st.in(src, e->sw_stage, (size_t)N * K * 88));
    void *const *b = e->qbuf[QF_SW];
    hipLaunchKernelGGL(k_swept_clearance<false>, dim3((unsigned)N * K), dim3(SWEEP_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, e->sw_reach_dev, src, K,
                       safety, tolerance, (float *)b[RR_SW_STOP], (float4 *)b[RR_SW_HIT], (int4 *)b[RR_SW_ID], (float *)b[RR_SW_FREE],
                       (const float *)nullptr, (const SweepChain *)nullptr);
    HIPCHK(hipGetLastError());
    e->qk[QF_SW] = K;
    return st.wait();
}

int rr_sweep_reach(rr_env *e, float *out) {
    if (!e) return fail(RR_EINVAL, "rr_sweep_reach: null env");
    if (!out) return fail(RR_EINVAL, "rr_sweep_reach: null destination");
    for (int k = 0; k < NB; k++) memcpy(out + (size_t)k * e->n_shapes, e->sweep_reach.r[k], (size_t)e->n_shapes * 4);
    return RR_OK;
}

int rr_sweep_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_SW), HIP_QUERY, which, dev_ptr, bytes); }
int rr_sweep_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_SW), HIP_QUERY, which, dst, bytes); }

// ---- objects attached to robot links in the posture queries (rr_carry.inc) ---------------------------------------------------------------
// The table [N][NOBJ][ATT_ROW] and its staging block: on first use, all or nothing, the table zero-filled (every object free).
static int ensure_attachments(rr_env *e, const char *who) {
    const size_t bytes = (size_t)e->P.N * NOBJ * ATT_ROW * 4;
    return ensure_group(e, -1, who, "the attachment table", {mem_part(&e->att_table, bytes), stage_part(&e->att_stage, bytes)});
}

// The caller speaks of a URDF link's COM frame, the device table of the moving body b the link hangs on: with (L, l) = link_rot, link_pos
// of the link, T_body<-object = (L, l) o rel.  Both directions in float64; the quaternion of a row read back is the largest-of-four-squares
// root of its matrix, normalised (a captured matrix is orthonormal to float32 rounding only).
static void att_to_body(const RenderModel &RM, int l, const double *rel7, float *row) {
    const double x = rel7[3], y = rel7[4], z = rel7[5], w = rel7[6];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    const float *L = RM.link_rot[l], *lp = RM.link_pos[l];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) row[3 * i + j] = (float)((double)L[3 * i] * R[j] + (double)L[3 * i + 1] * R[3 + j] + (double)L[3 * i + 2] * R[6 + j]);
        row[9 + i] = (float)((double)lp[i] + (double)L[3 * i] * rel7[0] + (double)L[3 * i + 1] * rel7[1] + (double)L[3 * i + 2] * rel7[2]);
    }
}
static void att_from_body(const RenderModel &RM, int l, const float *row, float *rel7) {
    const float *L = RM.link_rot[l], *lp = RM.link_pos[l];
    double R[9], t[3];
    for (int i = 0; i < 3; i++) {      // L^T R_rel, L^T (t_rel - l)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (double)L[i] * row[j] + (double)L[3 + i] * row[3 + j] + (double)L[6 + i] * row[6 + j];
        t[i] = (double)L[i] * ((double)row[9] - lp[0]) + (double)L[3 + i] * ((double)row[10] - lp[1]) + (double)L[6 + i] * ((double)row[11] - lp[2]);
    }
    const double sq[4] = {1 + R[0] - R[4] - R[8], 1 - R[0] + R[4] - R[8], 1 - R[0] - R[4] + R[8], 1 + R[0] + R[4] + R[8]};    // 4 x^2, 4 y^2, 4 z^2, 4 w^2
    int big = 0;
    for (int a = 1; a < 4; a++) if (sq[a] > sq[big]) big = a;
    const double r = std::sqrt(std::max(sq[big], 0.0)) * 0.5, s = 0.25 / (r > 0 ? r : 1.0);
    double q[4];
    if (big == 0) { q[0] = r; q[1] = (R[1] + R[3]) * s; q[2] = (R[2] + R[6]) * s; q[3] = (R[7] - R[5]) * s; }
    else if (big == 1) { q[0] = (R[1] + R[3]) * s; q[1] = r; q[2] = (R[5] + R[7]) * s; q[3] = (R[2] - R[6]) * s; }
    else if (big == 2) { q[0] = (R[2] + R[6]) * s; q[1] = (R[5] + R[7]) * s; q[2] = r; q[3] = (R[3] - R[1]) * s; }
    else { q[0] = (R[7] - R[5]) * s; q[1] = (R[2] - R[6]) * s; q[2] = (R[3] - R[1]) * s; q[3] = r; }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 3; i++) rel7[i] = (float)t[i];
    for (int i = 0; i < 4; i++) rel7[3 + i] = (float)(n > 0 ? q[i] / n : (i == 3 ? 1.0 : 0.0));
}

// The rows of the masked envs, replaced whole, on the main stream behind every query enqueued before (which read the table on this
// stream).  With link and no rel_pose, k_attach_capture fills the poses from the present state behind whatever was enqueued -- no wait
// for the poses.  Everything is validated before anything changes.  A query-side setting: the state, the preparation record and
// la_valid are not touched, and no step reads the table.
int rr_set_attachments(rr_env *e, const int32_t *link, const float *rel_pose, const uint8_t *env_mask) {
    if (!e) return fail(RR_EINVAL, "rr_set_attachments: null env");
    if (!link && rel_pose) return fail(RR_EINVAL, "rr_set_attachments: rel_pose without link (link NULL detaches)");
    const int N = e->P.N, nobj = e->P.nobj;
    std::vector<float> rows((size_t)N * NOBJ * ATT_ROW, 0.0f);
    if (link) {
        RRCHK(check_link_table(e, "rr_set_attachments", RR_EINVAL));
        for (int i = 0; i < N; i++) {
            if (env_mask && !env_mask[i]) continue;
            for (int o = 0; o < nobj; o++) {
                const int l = link[(size_t)i * nobj + o];
                if (l == -1) continue;
                const std::string which = "rr_set_attachments: env " + std::to_string(i) + ", object " + std::to_string(o) + ": ";
                if (l < 0 || l >= KIN_LINKS) return fail(RR_EINVAL, which + "link " + std::to_string(l) + " is neither -1 (free) nor in [0, " + std::to_string(KIN_LINKS) + ")");
                if (e->RM.link_body[l] < 0) return fail(RR_EINVAL, which + "link " + std::to_string(l) + " is rigid with the world: nothing carries the object");
                float *row = &rows[((size_t)i * NOBJ + o) * ATT_ROW];
                const int att = e->RM.link_body[l] + 1;
                memcpy(row + ATT_BODY, &att, 4);
                if (!rel_pose) continue;      // k_attach_capture writes the pose
                double r[7], n2 = 0.0;
                for (int k = 0; k < 7; k++) {
                    r[k] = rel_pose[((size_t)i * nobj + o) * 7 + k];
                    if (!std::isfinite(r[k])) return fail(RR_EINVAL, which + "the rel pose is not finite");
                }
                for (int k = 3; k < 7; k++) n2 += r[k] * r[k];
                if (!(n2 > 0.0)) return fail(RR_EINVAL, which + "the rel pose's quaternion has norm zero");
                for (int k = 3; k < 7; k++) r[k] /= std::sqrt(n2);
                att_to_body(e->RM, l, r, row);
            }
        }
    }
    if (!link && !e->att_table) return RR_OK;      // detaching in a table that does not exist yet: every object is free, the feature off
    RRCHK(ensure_attachments(e, "rr_set_attachments"));
    HIPCHK(hipSetDevice(e->cfg.device));
    const unsigned char *m = nullptr;
    HIPCHK(hipMemcpyAsync(e->att_stage, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, e->stream));
    if (env_mask) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_attach_set, dim3((unsigned)((N * NOBJ * ATT_ROW + 255) / 256)), dim3(256), 0, e->stream, N, (const float *)e->att_stage, m, e->att_table);
    HIPCHK(hipGetLastError());
    if (link && !rel_pose) {
        hipLaunchKernelGGL(k_attach_capture, dim3((unsigned)N), dim3(64), 0, e->stream, e->B, e->P, e->D, m, e->att_table);
        HIPCHK(hipGetLastError());
    }
    if (e->att_link.empty()) e->att_link.assign((size_t)N * nobj, -1);
    for (int i = 0; i < N; i++) {
        if (env_mask && !env_mask[i]) continue;
        for (int o = 0; o < nobj; o++) e->att_link[(size_t)i * nobj + o] = link ? link[(size_t)i * nobj + o] : -1;
    }
    if (link) e->att_on = true;
    else if (!env_mask) e->att_on = false;      // the unmasked detach: the queries launch their original kernels until the next attach
    HIPCHK(hipStreamSynchronize(e->stream));    // the arguments and the staged rows are host memory
    return RR_OK;
}

int rr_get_attachments(rr_env *e, int32_t *link_out, float *rel_pose_out) {
    if (!e) return fail(RR_EINVAL, "rr_get_attachments: null env");
    const int N = e->P.N, nobj = e->P.nobj;
    for (size_t i = 0; link_out && i < (size_t)N * nobj; i++) link_out[i] = e->att_link.empty() ? -1 : e->att_link[i];
    if (!rel_pose_out) return RR_OK;
    std::vector<float> rows;
    if (e->att_table) {
        rows.resize((size_t)N * NOBJ * ATT_ROW);
        HIPCHK(hipSetDevice(e->cfg.device));
        HIPCHK(hipMemcpyAsync(rows.data(), e->att_table, rows.size() * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    for (int i = 0; i < N; i++)
        for (int o = 0; o < nobj; o++) {
            float *out = rel_pose_out + ((size_t)i * nobj + o) * 7;
            const int l = e->att_link.empty() ? -1 : e->att_link[(size_t)i * nobj + o];
            if (l < 0 || rows.empty()) { for (int k = 0; k < 7; k++) out[k] = k == 6 ? 1.0f : 0.0f; continue; }      // free: the identity
            att_from_body(e->RM, l, &rows[((size_t)i * NOBJ + o) * ATT_ROW], out);
        }
    return RR_OK;
}

// ---- swept clearance with carried objects (rr_sweep.inc, CARRY) -------------------------------------------------------------------------
// The chain table of k_swept_clearance<true> on first use, all or nothing: chain[k][b] = the sum of |jpos[m]| over the bodies m from b up to,
// but not including, k -- the term the reach loop of the model parse adds, in its order -- in float64 and rounded up; 0 where joint k is
// not an ancestor-or-self of body b.  A table of its own: SweepReach, which both instantiations read, keeps its size.
static int ensure_sweep_chain(rr_env *e, const char *who) {
    if (e->sw_chain_dev) return RR_OK;
    e->sw_chain = {};
    for (int b = 0; b < NB; b++) {
        double r = 0.0;
        for (int k = b; k >= 0; k = PARENT_HOST[k]) {
            float f = (float)r;
            if ((double)f < r) f = std::nextafterf(f, INFINITY);
            e->sw_chain.c[k][b] = f;
            const double j[3] = {e->B.jpos[k][0], e->B.jpos[k][1], e->B.jpos[k][2]};
            r += std::sqrt(j[0] * j[0] + j[1] * j[1] + j[2] * j[2]);
        }
    }
    const GroupUpload up = {(void **)&e->sw_chain_dev, &e->sw_chain, sizeof(SweepChain), "the chain table"};
    return ensure_group(e, -1, who, "the chain table", {mem_part(&e->sw_chain_dev, sizeof(SweepChain), false)}, &up);
}

// rr_swept_clearance with the carried objects moving.  Arguments, refusals, staging, buffers and the stream contract are that call's;
// with the attachments off it IS that call.  With them on, k_swept_clearance<true> reads in addition the attachment table and the chain table
// and writes the same four buffers and nothing else.
int rr_carried_sweep(rr_env *e, const float *segments, int32_t n_segments, int32_t on_device, float safety, float tolerance) {
    if (!e) return fail(RR_EINVAL, "rr_carried_sweep: null env");
    RRCHK(sweep_arguments(e, "rr_carried_sweep", segments, n_segments, safety, tolerance));
    // nothing is carried: the same kernel, the same bytes.  (rr_swept_clearance checks the arguments once more; the check above is
    // deliberate all the same: a refusal names the entry point that was called.)
    if (!e->att_on) return rr_swept_clearance(e, segments, n_segments, on_device, safety, tolerance);
    const int Q = e->dist_n, N = e->P.N, K = n_segments;
    RRCHK(ensure_query(e, QF_DIST, "rr_carried_sweep"));       // (the device copy of the pair table)
    RRCHK(ensure_query(e, QF_SW, "rr_carried_sweep", {stage_part(&e->sw_stage, (size_t)N * RR_PC_MAX_POSTURES * 88, !on_device)}));
    RRCHK(ensure_sweep_chain(e, "rr_carried_sweep"));       // (a group of its own, like the two above: a failure here leaves the sweep buffers allocated and zero-filled)
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, !on_device};
    const float *src = segments;
    RRCHK(st.in(src, e->sw_stage, (size_t)N * K * 88));
    void *const *b = e->qbuf[QF_SW];
    hipLaunchKernelGGL(k_swept_clearance<true>, dim3((unsigned)N * K), dim3(SWEEP_THREADS), 0, e->stream, e->B, e->P, e->D, e->dist_tab_dev, Q, e->sw_reach_dev, src, K,
                       safety, tolerance, (float *)b[RR_SW_STOP], (float4 *)b[RR_SW_HIT], (int4 *)b[RR_SW_ID], (float *)b[RR_SW_FREE],
                       (const float *)e->att_table, (const SweepChain *)e->sw_chain_dev);
    HIPCHK(hipGetLastError());
    e->qk[QF_SW] = K;
    return st.wait();
}

// ---- kinematics at candidate postures (rr_pkin.inc) -------------------------------------------------------------------------------------
// Link poses, point positions and Jacobians at K candidate postures per env, on the device.  On the main stream like
// rr_posture_clearance: behind every step, reset and state write enqueued before it.  Reads the tensor, the model and the points (the
// handle's host copy goes to the kernel by value: a call enqueued earlier keeps the points it was launched with); writes the three
// buffers and nothing else -- not the state, the scratch slab of the look-ahead, la_valid, an error flag or a buffer of another query.
int rr_posture_kinematics(rr_env *e, const float *postures, int32_t n_postures, int32_t on_device) {
    if (!e) return fail(RR_EINVAL, "rr_posture_kinematics: null env");
    if (!postures) return fail(RR_EINVAL, "rr_posture_kinematics: null postures");
    if (n_postures < 1 || n_postures > RR_PC_MAX_POSTURES)
        return fail(RR_EINVAL, "rr_posture_kinematics: n_postures " + std::to_string(n_postures) + " is not in [1, RR_PC_MAX_POSTURES = " +
                                   std::to_string(RR_PC_MAX_POSTURES) + "]");
    const int N = e->P.N, K = n_postures;
    RRCHK(ensure_query(e, QF_PK, "rr_posture_kinematics", {posture_stage(e, !on_device)}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, !on_device};
    const float *src = postures;
    RRCHK(st.in(src, e->pc_stage, (size_t)N * K * 44));
    const int rows = N * K;
    float *const *b = (float *const *)e->qbuf[QF_PK];
    const PkOut O = {b[RR_PK_LINK_POSE], b[RR_PK_POINT_POS], b[RR_PK_JACOBIAN]};
    hipLaunchKernelGGL(k_posture_kinematics, dim3((unsigned)((rows + PK_ROWS - 1) / PK_ROWS)), dim3(PK_THREADS), 0, e->stream, e->B, e->RM_dev, src, rows, O,
                       e->kin_pts, e->kin_np);
    HIPCHK(hipGetLastError());
    e->qk[QF_PK] = K;
    return st.wait();
}

int rr_posture_kinematics_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_PK), HIP_QUERY, which, dev_ptr, bytes); }
int rr_posture_kinematics_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_PK), HIP_QUERY, which, dst, bytes); }

// ---- inverse kinematics at candidate targets (rr_pik.inc) ------------------------------------------------------------------------------
// K target tool poses per env solved on the device.  On the main stream like rr_posture_clearance: behind every step, reset and
// state write enqueued before it.  Reads the two tensors (without seeds: the joint columns of the state), the model and the points
// (the handle's host copy goes to the kernel by value); writes the three buffers and nothing else -- not the state, the scratch slab
// of the look-ahead, la_valid, an error flag, the buffers of rr_ik / rr_plan_macro or a buffer of another query.
int rr_posture_ik(rr_env *e, const float *targets, const float *seeds, int32_t n_targets, int32_t on_device, const rr_ik_options *opt) {
    if (!e) return fail(RR_EINVAL, "rr_posture_ik: null env");
    if (!targets) return fail(RR_EINVAL, "rr_posture_ik: null targets");
    if (n_targets < 1 || n_targets > RR_PC_MAX_POSTURES)
        return fail(RR_EINVAL, "rr_posture_ik: n_targets " + std::to_string(n_targets) + " is not in [1, RR_PC_MAX_POSTURES = " + std::to_string(RR_PC_MAX_POSTURES) + "]");
    const rr_ik_options def = {0, 32, 1e-3f, 0.1f, 0.5f, RR_PIK_CLAMP_LIMITS};
    const rr_ik_options o = opt ? *opt : def;
    if (o.point < 0 || o.point >= e->kin_np)
        return fail(RR_EINVAL, "rr_posture_ik: point " + std::to_string(o.point) + " is not in [0, P = " + std::to_string(e->kin_np) + ") (rr_set_kinematic_points)");
    if (o.max_iterations < 1 || o.max_iterations > RR_PIK_MAX_ITERATIONS)
        return fail(RR_EINVAL, "rr_posture_ik: max_iterations " + std::to_string(o.max_iterations) + " is not in [1, RR_PIK_MAX_ITERATIONS = " +
                                   std::to_string(RR_PIK_MAX_ITERATIONS) + "]");
    if (!(o.tolerance > 0.0f) || !std::isfinite(o.tolerance)) return fail(RR_EINVAL, "rr_posture_ik: tolerance " + std::to_string(o.tolerance) + " is not a finite number > 0");
    if (!(o.damping > 0.0f) || !std::isfinite(o.damping)) return fail(RR_EINVAL, "rr_posture_ik: damping " + std::to_string(o.damping) + " is not a finite number > 0");
    if (!(o.max_step > 0.0f) || !std::isfinite(o.max_step)) return fail(RR_EINVAL, "rr_posture_ik: max_step " + std::to_string(o.max_step) + " is not a finite number > 0");
    if (o.flags & ~(uint32_t)(RR_PIK_POSITION_ONLY | RR_PIK_CLAMP_LIMITS)) return fail(RR_EINVAL, "rr_posture_ik: unknown flag bits in " + std::to_string(o.flags));
    const int N = e->P.N, K = n_targets;
    RRCHK(ensure_query(e, QF_PIK, "rr_posture_ik", {posture_stage(e, !on_device && seeds), stage_part(&e->pik_stage, (size_t)N * RR_PC_MAX_POSTURES * 28, !on_device)}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, !on_device};
    const float *tsrc = targets, *ssrc = seeds;
    RRCHK(st.in(tsrc, e->pik_stage, (size_t)N * K * 28));
    RRCHK(st.in(ssrc, e->pc_stage, (size_t)N * K * 44));
    const int rows = N * K;
    void *const *b = e->qbuf[QF_PIK];
    const PikOut O = {(float *)b[RR_PIK_POSTURE], (float *)b[RR_PIK_RESULT], (int *)b[RR_PIK_INFO]};
    const PikOpt po = {o.point, o.max_iterations, o.tolerance, o.damping * o.damping, o.max_step, o.flags};
    // (one instantiation per system size: 6 x 6 full pose, 3 x 3 position only)
    if (o.flags & RR_PIK_POSITION_ONLY)
        hipLaunchKernelGGL(k_posture_ik<1>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, e->stream, e->B, e->RM_dev, tsrc, ssrc, (const float *)e->D.state, N, K,
                           O, e->kin_pts, po);
    else
        hipLaunchKernelGGL(k_posture_ik<0>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, e->stream, e->B, e->RM_dev, tsrc, ssrc, (const float *)e->D.state, N, K,
                           O, e->kin_pts, po);
    HIPCHK(hipGetLastError());
    e->qk[QF_PIK] = K;
    return st.wait();
}

int rr_posture_ik_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_PIK), HIP_QUERY, which, dev_ptr, bytes); }
int rr_posture_ik_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_PIK), HIP_QUERY, which, dst, bytes); }

// ---- joint-space dynamics at candidate postures (rr_pdyn.inc) ---------------------------------------------------------------------------
// M, G, G + C, M qdd + C + G and on request M^-1 at K rows per env, on the device.  On the main stream like rr_posture_clearance:
// behind every step, reset and state write enqueued before it.  Reads the tensors (without postures: the joint columns of the
// state), the model and the handle's body table -- the one the preparation reads --; writes the five buffers and nothing else: not
// the state, the scratch slab of the look-ahead, la_valid, an error flag or a buffer of another query.
int rr_posture_dynamics(rr_env *e, const float *postures, const float *velocities, const float *accelerations, int32_t n_postures, int32_t on_device,
                        uint32_t flags) {
    if (!e) return fail(RR_EINVAL, "rr_posture_dynamics: null env");
    if (n_postures < 1 || n_postures > RR_PC_MAX_POSTURES)
        return fail(RR_EINVAL, "rr_posture_dynamics: n_postures " + std::to_string(n_postures) + " is not in [1, RR_PC_MAX_POSTURES = " +
                                   std::to_string(RR_PC_MAX_POSTURES) + "]");
    if (!postures && velocities) return fail(RR_EINVAL, "rr_posture_dynamics: velocities without postures (the present-state form takes the state's joint velocities)");
    if (!postures && n_postures != 1) return fail(RR_EINVAL, "rr_posture_dynamics: n_postures " + std::to_string(n_postures) + " without postures (the present-state form has K = 1)");
    if (flags & ~(uint32_t)RR_PD_INVERSE) return fail(RR_EINVAL, "rr_posture_dynamics: unknown flag bits in " + std::to_string(flags));
    const int N = e->P.N, K = n_postures;
    const size_t tensor = (size_t)N * K * 44;
    RRCHK(ensure_query(e, QF_PD, "rr_posture_dynamics", {posture_stage(e, !on_device && postures),
                                                         stage_part(&e->pd_stage, (size_t)2 * N * RR_PC_MAX_POSTURES * 44, !on_device && (velocities || accelerations))}));
    HIPCHK(hipSetDevice(e->cfg.device));
    const HostStaging st = {e, !on_device};      // (the wait also without a tensor: one rule for the host path)
    PdIn in = {postures, velocities, accelerations, NB, 1};
    RRCHK(st.in(in.q, e->pc_stage, tensor));
    RRCHK(st.in(in.qd, e->pd_stage, tensor));
    RRCHK(st.in(in.qdd, e->pd_stage + (size_t)N * RR_PC_MAX_POSTURES * NB, tensor));
    if (!postures) {      // the present state: row e is env e, q and qd the columns ST_Q.. and ST_QD.. of the [61][N] state
        in.q = (const float *)e->D.state + (size_t)ST_Q * N;
        in.qd = (const float *)e->D.state + (size_t)ST_QD * N;
        in.rs = 1; in.cs = (size_t)N;
    }
    const int rows = N * K;
    float *const *b = (float *const *)e->qbuf[QF_PD];
    const PdOut O = {b[RR_PD_MASS_MATRIX], b[RR_PD_GRAVITY], b[RR_PD_BIAS], b[RR_PD_TORQUE], b[RR_PD_MASS_INVERSE]};
    const dim3 grid((unsigned)((rows + PD_ROWS - 1) / PD_ROWS));
    if (flags & RR_PD_INVERSE)
        hipLaunchKernelGGL(k_posture_dynamics<true>, grid, dim3(PD_THREADS), 0, e->stream, e->B, (const float *)e->D.body_tab, e->P.gravity, in, rows, O);
    else
        hipLaunchKernelGGL(k_posture_dynamics<false>, grid, dim3(PD_THREADS), 0, e->stream, e->B, (const float *)e->D.body_tab, e->P.gravity, in, rows, O);
    HIPCHK(hipGetLastError());
    e->qk[QF_PD] = K;
    return st.wait();
}

int rr_posture_dynamics_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) { return query_buffer(query_view(e, QF_PD), HIP_QUERY, which, dev_ptr, bytes); }
int rr_posture_dynamics_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) { return query_copy_to_host(query_view(e, QF_PD), HIP_QUERY, which, dst, bytes); }

// ---- joint torque inputs of the step (rr_torque.inc) ------------------------------------------------------------------------------------
// The table tau [N][11] and, for a host caller, its staging block: on first use, all or nothing, the table zero-filled.
static int ensure_torques(rr_env *e, const char *who, bool stage = false) {
    const size_t bytes = (size_t)e->P.N * NB * 4;
    return ensure_group(e, -1, who, "the joint torque table", {mem_part(&e->jt_table, bytes), stage_part(&e->jt_stage, bytes, stage)});
}

// The rows of the masked envs into the handle's table, one launch on the main stream: behind every step enqueued before it (whose
// k_joint_torque read the table on this stream), in front of the next one.  A command-side setting like the motor targets: the
// state, the preparation record and la_valid are not touched -- the step applies the table behind the look-ahead, whatever it holds.
int rr_set_joint_torques(rr_env *e, const float *torques, int32_t torques_on_device, const uint8_t *env_mask, int32_t mask_on_device) {
    if (!e) return fail(RR_EINVAL, "rr_set_joint_torques: null env");
    if (torques && env_mask && !torques_on_device != !mask_on_device)
        return fail(RR_EINVAL, std::string("rr_set_joint_torques: torques and env_mask must live on the same side (torques on the ") +
                                   (torques_on_device ? "device" : "host") + ", env_mask on the " + (mask_on_device ? "device" : "host") + ")");
    const int N = e->P.N;
    if (torques && !torques_on_device) {      // host rows are validated before anything changes
        for (int i = 0; i < N; i++) {
            if (env_mask && !env_mask[i]) continue;
            for (int j = 0; j < NB; j++)
                if (!std::isfinite(torques[(size_t)i * NB + j]))
                    return fail(RR_EINVAL, "rr_set_joint_torques: env " + std::to_string(i) + ", joint " + std::to_string(j) + ": the torque is not finite");
        }
    }
    if (!torques && !e->jt_table) return RR_OK;      // zeroing rows of a table that does not exist yet: it is all zero, the feature off
    RRCHK(ensure_torques(e, "rr_set_joint_torques", torques && !torques_on_device));
    HIPCHK(hipSetDevice(e->cfg.device));
    const float *src = torques;
    const unsigned char *m = env_mask;
    if (torques && !torques_on_device) { HIPCHK(hipMemcpyAsync(e->jt_stage, torques, (size_t)N * NB * 4, hipMemcpyHostToDevice, e->stream)); src = e->jt_stage; }
    const bool host_mask = env_mask && !mask_on_device;
    if (host_mask) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_joint_torque_set, dim3((unsigned)((N * NB + 255) / 256)), dim3(256), 0, e->stream, N, src, m, e->jt_table);
    HIPCHK(hipGetLastError());
    if (torques) e->jt_on = true;
    else if (!env_mask) e->jt_on = false;      // the clearing call: the steps launch no torque kernel until the next table
    if ((torques && !torques_on_device) || host_mask) HIPCHK(hipStreamSynchronize(e->stream));   // the arguments are host memory
    return RR_OK;
}

int rr_joint_torque_buffer(rr_env *e, void **dev_ptr, size_t *bytes) {
    if (!e) return fail(RR_EINVAL, "rr_joint_torque_buffer: null env");
    RRCHK(ensure_torques(e, "rr_joint_torque_buffer"));
    if (dev_ptr) *dev_ptr = e->jt_table;
    if (bytes) *bytes = (size_t)e->P.N * NB * 4;
    return RR_OK;
}

int rr_get_joint_torques(rr_env *e, float *out_host) {
    if (!e) return fail(RR_EINVAL, "rr_get_joint_torques: null env");
    if (!out_host) return fail(RR_EINVAL, "rr_get_joint_torques: null destination");
    RRCHK(ensure_torques(e, "rr_get_joint_torques"));
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(out_host, e->jt_table, (size_t)e->P.N * NB * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

// ---- external wrenches of the step (rr_wrench.inc) ---------------------------------------------------------------------------------------
// The table w [N][14][6] and, for a host caller, its staging block: on first use, all or nothing, the table zero-filled.
static int ensure_wrenches(rr_env *e, const char *who, bool stage = false) {
    const size_t bytes = (size_t)e->P.N * RR_XW_BODIES * 6 * 4;
    return ensure_group(e, -1, who, "the external wrench table", {mem_part(&e->xw_table, bytes), stage_part(&e->xw_stage, bytes, stage)});
}

// The rows of the masked envs into the handle's table, one launch on the main stream: behind every step enqueued before it (whose
// k_ext_wrench read the table on this stream), in front of the next one.  A command-side setting like the joint torques: the state,
// the preparation record and the look-ahead's validity are not touched -- the step applies the table behind the look-ahead.
int rr_set_external_wrenches(rr_env *e, const float *wrenches, int32_t wrenches_on_device, const uint8_t *env_mask, int32_t mask_on_device) {
    if (!e) return fail(RR_EINVAL, "rr_set_external_wrenches: null env");
    if (wrenches && env_mask && !wrenches_on_device != !mask_on_device)
        return fail(RR_EINVAL, std::string("rr_set_external_wrenches: wrenches and env_mask must live on the same side (wrenches on the ") +
                                   (wrenches_on_device ? "device" : "host") + ", env_mask on the " + (mask_on_device ? "device" : "host") + ")");
    const int N = e->P.N;
    const int ROW = RR_XW_BODIES * 6;
    if (wrenches && !wrenches_on_device) {      // host rows are validated before anything changes
        for (int i = 0; i < N; i++) {
            if (env_mask && !env_mask[i]) continue;
            for (int j = 0; j < ROW; j++)
                if (!std::isfinite(wrenches[(size_t)i * ROW + j]))
                    return fail(RR_EINVAL, "rr_set_external_wrenches: env " + std::to_string(i) + ", row " + std::to_string(j / 6) + ", entry " + std::to_string(j % 6) +
                                               ": the wrench is not finite");
        }
    }
    if (!wrenches && !e->xw_table) return RR_OK;      // zeroing rows of a table that does not exist yet: it is all zero, the feature off
    RRCHK(ensure_wrenches(e, "rr_set_external_wrenches", wrenches && !wrenches_on_device));
    HIPCHK(hipSetDevice(e->cfg.device));
    const float *src = wrenches;
    const unsigned char *m = env_mask;
    if (wrenches && !wrenches_on_device) { HIPCHK(hipMemcpyAsync(e->xw_stage, wrenches, (size_t)N * ROW * 4, hipMemcpyHostToDevice, e->stream)); src = e->xw_stage; }
    const bool host_mask = env_mask && !mask_on_device;
    if (host_mask) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_ext_wrench_set, dim3((unsigned)((N * ROW + 255) / 256)), dim3(256), 0, e->stream, N, src, m, e->xw_table);
    HIPCHK(hipGetLastError());
    if (wrenches) e->xw_on = true;
    else if (!env_mask) e->xw_on = false;      // the clearing call: the steps launch no wrench kernel until the next table
    if ((wrenches && !wrenches_on_device) || host_mask) HIPCHK(hipStreamSynchronize(e->stream));   // the arguments are host memory
    return RR_OK;
}

int rr_external_wrench_buffer(rr_env *e, void **dev_ptr, size_t *bytes) {
    if (!e) return fail(RR_EINVAL, "rr_external_wrench_buffer: null env");
    RRCHK(ensure_wrenches(e, "rr_external_wrench_buffer"));
    if (dev_ptr) *dev_ptr = e->xw_table;
    if (bytes) *bytes = (size_t)e->P.N * RR_XW_BODIES * 6 * 4;
    return RR_OK;
}

int rr_get_external_wrenches(rr_env *e, float *out_host) {
    if (!e) return fail(RR_EINVAL, "rr_get_external_wrenches: null env");
    if (!out_host) return fail(RR_EINVAL, "rr_get_external_wrenches: null destination");
    RRCHK(ensure_wrenches(e, "rr_get_external_wrenches"));
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(out_host, e->xw_table, (size_t)e->P.N * RR_XW_BODIES * 6 * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_get_buffer(rr_env *e, int32_t field, void **dev_ptr, size_t *bytes) {
    if (!e || field < 0 || field >= RR_F_COUNT) return fail(RR_EINVAL, "rr_get_buffer: bad field");
    refresh_frame_fields(e);
    if (contact_obs_field(field)) { const int rc = ensure_contact_obs(e); if (rc != RR_OK) return rc; }
    if (dev_ptr) *dev_ptr = e->field_ptr[field];
    if (bytes) *bytes = e->field_bytes[field];
    return RR_OK;
}

int rr_copy_to_host(rr_env *e, int32_t field, void *dst, size_t bytes) {
    if (!e || !dst || field < 0 || field >= RR_F_COUNT) return fail(RR_EINVAL, "rr_copy_to_host: bad argument");
    refresh_frame_fields(e);
    if (contact_obs_field(field)) { const int rc = ensure_contact_obs(e); if (rc != RR_OK) return rc; }
    if (!e->field_ptr[field]) return fail(RR_EINVAL, "rr_copy_to_host: field not available (RR_FLAG_NO_MASK)");
    if (bytes != e->field_bytes[field]) return fail(RR_EINVAL, "rr_copy_to_host: size mismatch");
    HIPCHK(hipSetDevice(e->cfg.device));
    if (field == RR_F_STATE)
        hipLaunchKernelGGL(k_state_io, dim3((e->P.N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, e->state_aos, 1);
    HIPCHK(hipMemcpyAsync(dst, e->field_ptr[field], bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_set_state(rr_env *e, const float *state_host) {
    if (!e || !state_host) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;
    HIPCHK(hipMemcpyAsync(e->state_aos, state_host, e->field_bytes[RR_F_STATE], hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_state_io, dim3((e->P.N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, e->state_aos, 0);
    launch_obs(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

// ---- checkpoint: everything a later restore needs to continue bit for bit ----------------------------------------------------
// {header, state slab [72][N] (incl. motor targets), contact count [N], contact list [N][48][3] float4, normal forces [N][48],
//  timestep [N], errflags [N], touch [N][4], object home poses [21][N], object dynamics [N][nobj][8], pair materials
//  [N][npairs][4], actuators [N][11][4] (version 5)}: the 61-float state of RR_F_STATE plus the contact history of the warm start (Bullet: the persistent manifolds
// with their cached impulses), the episode clocks and the per-env object data.
// The header also carries every parameter the continuation depends on: a blob restored into a handle that steps differently
// (other dt / ERP / margin / sweeps / warm-start factor / motor gains and force / damping / rate-limit switch / object-lane
// capacity / inertia source / edge contacts) is rejected
// instead of silently diverging.
struct CkptHeader { char magic[8]; int32_t version, N, nobj, iters; float dt, erp, margin, warmstart; int32_t os_cap, edge_contacts, urdf_inertia, no_rate_limit;
                    float kp, kd, max_impulse, lin_damp, ang_damp, rest_thresh, gravity; int32_t reserved; };
static CkptHeader ckpt_header(const rr_env *e) {
    CkptHeader hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, "RRCKPT05", 8); hd.version = 5; hd.N = e->P.N; hd.nobj = e->P.nobj; hd.iters = e->P.iters;
    hd.dt = e->P.dt; hd.erp = e->P.erp; hd.margin = e->P.margin; hd.warmstart = e->P.warmstart;
    hd.os_cap = e->P.os_cap; hd.edge_contacts = e->P.edge_contacts; hd.urdf_inertia = e->cfg.use_urdf_inertia;
    hd.no_rate_limit = (e->cfg.solver_flags & RR_SOLVER_NO_RATE_LIMIT) ? 1 : 0;
    hd.kp = e->P.kp; hd.kd = e->P.kd; hd.max_impulse = e->P.max_impulse; hd.lin_damp = e->P.lin_damp; hd.ang_damp = e->P.ang_damp;
    hd.rest_thresh = e->P.rest_thresh; hd.gravity = e->P.gravity;
    return hd;
}
static size_t ckpt_bytes(const rr_env *e) {
    const size_t N = e->P.N;
    return sizeof(CkptHeader) + 4 * (ST_TOTAL * N + N + N * MAXC * 12 + N * MAXC + N + N + N * 4 + NOBJ * 7 * N) + 4 * (e->dyn.size() + e->pair_host.size() + e->act.size());
}
int rr_checkpoint_bytes(rr_env *e, size_t *bytes) {
    if (!e || !bytes) return fail(RR_EINVAL, "null argument");
    *bytes = ckpt_bytes(e);
    return RR_OK;
}
static int ckpt_copy(rr_env *e, char *host, bool save) {
    const size_t N = e->P.N;
    struct Part { void *dev; size_t bytes; } parts[] = {
        {e->D.state, 4 * ST_TOTAL * N}, {e->D.ccount, 4 * N}, {e->D.clist, 4 * N * MAXC * 12}, {e->D.cforce, 4 * N * MAXC},
        {e->D.timestep, 4 * N}, {e->D.errflags, 4 * N}, {e->D.touch, 4 * N * 4}, {e->D.obj_home, 4 * NOBJ * 7 * N}};
    char *h = host + sizeof(CkptHeader);
    for (const Part &p : parts) {
        if (save) HIPCHK(hipMemcpyAsync(h, p.dev, p.bytes, hipMemcpyDeviceToHost, e->stream));
        else HIPCHK(hipMemcpyAsync(p.dev, h, p.bytes, hipMemcpyHostToDevice, e->stream));
        h += p.bytes;
    }
    // the object dynamics and the actuators: from the host copies (a restore uploads them again)
    for (std::vector<float> *v : {&e->dyn, &e->pair_host, &e->act}) {
        if (save) memcpy(h, v->data(), v->size() * 4);
        else memcpy(v->data(), h, v->size() * 4);
        h += v->size() * 4;
    }
    if (save) return RR_OK;
    const int rc = upload_dynamics(e);
    return rc != RR_OK ? rc : upload_actuators(e);
}
int rr_checkpoint_save(rr_env *e, void *dst_host, size_t bytes) {
    if (!e || !dst_host) return fail(RR_EINVAL, "null argument");
    if (bytes != ckpt_bytes(e)) return fail(RR_EINVAL, "rr_checkpoint_save: size mismatch (rr_checkpoint_bytes)");
    HIPCHK(hipSetDevice(e->cfg.device));
    const CkptHeader hd = ckpt_header(e);
    memcpy(dst_host, &hd, sizeof hd);
    const int rc = ckpt_copy(e, (char *)dst_host, true);
    if (rc != RR_OK) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}
int rr_checkpoint_restore(rr_env *e, const void *src_host, size_t bytes) {
    if (!e || !src_host) return fail(RR_EINVAL, "null argument");
    if (bytes != ckpt_bytes(e)) return fail(RR_EINVAL, "rr_checkpoint_restore: size mismatch (rr_checkpoint_bytes)");
    CkptHeader hd;
    memcpy(&hd, src_host, sizeof hd);
    const CkptHeader mine = ckpt_header(e);
    if (memcmp(hd.magic, mine.magic, 8) != 0 || hd.version != mine.version || hd.N != mine.N || hd.nobj != mine.nobj)
        return fail(RR_EINVAL, "rr_checkpoint_restore: not a checkpoint of an env handle of this shape");
    if (memcmp(&hd, &mine, sizeof hd) != 0)
        return fail(RR_EINVAL, "rr_checkpoint_restore: the checkpoint was taken with other step parameters (dt / erp / margin / solver_iters / warm start / motor gains / motor force / damping / rate limit / object-lane capacity / inertia source / edge contacts)");
    HIPCHK(hipSetDevice(e->cfg.device));
    e->la_valid = false;
    const int rc = ckpt_copy(e, (char *)const_cast<void *>(src_host), false);
    if (rc != RR_OK) return rc;
    // the published count follows the restored list; the class diagnostic and k_collide's launch order start clean (the lists of
    // the handle's own run say nothing about the restored one)
    const size_t N = e->P.N;
    HIPCHK(hipMemcpyAsync(e->D.ccount_pub, e->D.ccount, 4 * N, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemsetAsync(e->D.class_pub, 0, 4 * N, e->stream));
    HIPCHK(hipMemsetAsync(e->D.hgflag, 0, 4 * N, e->stream));
    HIPCHK(hipMemsetAsync(e->D.hcount, 0, 16, e->stream)); HIPCHK(hipMemsetAsync(e->D.hcount2, 0, 16, e->stream));
    launch_obs(e);
    HIPCHK(hipStreamSynchronize(e->stream));   // the source is host memory
    return RR_OK;
}

// ---- env forks and snapshot slots on the device (rr_fork.inc) -------------------------------------------------------------------
// A slot is one block of the nine arrays of a ForkRec for all N envs, every array on a 256-byte boundary; the slots of a handle
// are one allocation (rr_env::snap), the staging slot of the in-place copies another (rr_env::fork_stage, kept until rr_destroy).
static const size_t FORK_PART_BYTES[9] = {4 * ST_TOTAL, 4, 4 * MAXC * 12, 4 * MAXC, 4, 4, 16, 4, 4};      // per env, in ForkRec's order
static size_t fork_slot_bytes(size_t N) {
    size_t total = 0;
    for (size_t b : FORK_PART_BYTES) total += (b * N + 255) & ~(size_t)255;
    return total;
}
static ForkRec fork_rec_at(char *base, size_t N) {
    char *p[9];
    for (int k = 0; k < 9; k++) { p[k] = base; base += (FORK_PART_BYTES[k] * N + 255) & ~(size_t)255; }
    ForkRec r;
    r.state = (float *)p[0]; r.ccount = (int *)p[1]; r.clist = (float4 *)p[2]; r.cforce = (float *)p[3]; r.timestep = (int *)p[4];
    r.errflags = (unsigned *)p[5]; r.touch = (float *)p[6]; r.ccount_pub = (int *)p[7]; r.class_pub = (int *)p[8];
    return r;
}
// The records of the running envs: the contact list, its count and the forces of the frame of the LAST SOLVED step, as bind_frames
// left them (the look-ahead's frame, clist_next, is not part of a record: a copy into the running envs drops it, la_valid).
static ForkRec fork_rec_live(const rr_env *e) {
    const DevPtrs &D = e->D;
    ForkRec r;
    r.state = D.state; r.ccount = D.ccount; r.clist = D.clist; r.cforce = D.cforce; r.timestep = D.timestep;
    r.errflags = D.errflags; r.touch = D.touch; r.ccount_pub = D.ccount_pub; r.class_pub = D.class_pub;
    return r;
}
static ForkRec fork_rec(const rr_env *e, int slot) {
    return slot == RR_SLOT_LIVE ? fork_rec_live(e) : fork_rec_at(e->snap + (size_t)slot * fork_slot_bytes(e->P.N), e->P.N);
}
// into a running env: the source's error bits 1, 2 and 4 (a frozen env forks frozen); bit 8 is cleared -- it describes the
// destination's own last rendered frame (rr_set_state clears it as well)
static inline unsigned fork_err_mask(int dst_slot) { return dst_slot == RR_SLOT_LIVE ? 7u : 0xffffffffu; }
static void launch_fork(rr_env *e, const ForkRec &src, const ForkRec &dst, const int *idx_dev, int identity, unsigned err_mask) {
    hipLaunchKernelGGL(k_fork, dim3((e->P.N + FK_GROUP - 1) / FK_GROUP, 5), dim3(256), 0, e->stream, e->P.N, src, dst, idx_dev, identity, err_mask);
}
// The first entry of a host index that is neither -1 nor an env, or -1 when there is none (no HIP type: plain host arithmetic).
static int fork_bad_index(const int32_t *idx, int N) {
    for (int i = 0; i < N; i++) if (idx[i] < -1 || idx[i] >= N) return i;
    return -1;
}

int rr_snapshot_slots(rr_env *e, int32_t n_slots) {
    if (!e) return fail(RR_EINVAL, "null env");
    if (n_slots < 0 || n_slots > RR_MAX_SLOTS) return fail(RR_EINVAL, "rr_snapshot_slots: n_slots " + std::to_string(n_slots) + " is not in [0, " + std::to_string(RR_MAX_SLOTS) + "]");
    HIPCHK(hipSetDevice(e->cfg.device));
    const size_t N = e->P.N, sb = fork_slot_bytes(N);
    char *blk = nullptr;
    if (n_slots > 0) {
        // the new slots exist before the old ones are given up; every one starts as a copy of the running envs
        RRCHK(mem_get(e, {mem_part(&blk, (size_t)n_slots * sb, false)}, "rr_snapshot_slots: allocating the slots"));
        const ForkRec live = fork_rec_live(e);
        for (int k = 0; k < n_slots; k++) launch_fork(e, live, fork_rec_at(blk + (size_t)k * sb, N), nullptr, 0, 0xffffffffu);
        const hipError_t lrc = hipGetLastError();
        if (lrc != hipSuccess) { (void)hipStreamSynchronize(e->stream); e->mem.release(blk); return fail(RR_EDEVICE, std::string("rr_snapshot_slots: ") + hipGetErrorString(lrc)); }
    }
    if (e->snap) {
        HIPCHK(hipStreamSynchronize(e->stream));      // (ends every queued copy that reads or writes the old slots)
        e->mem.release(e->snap);
    }
    e->snap = blk; e->n_slots = n_slots;
    return RR_OK;
}

// On the library's stream, like rr_contact_observations: every rr_step has made that stream wait for its side streams (ev_join /
// ev_join2 in step_split and step_single; the timed leg runs on it alone) before it returns, so the launch is ordered behind every
// kernel that reads or writes the records of the running envs -- the look-ahead included -- without a wait of its own.
int rr_copy_envs(rr_env *e, int32_t src_slot, int32_t dst_slot, const int32_t *src_index, int32_t index_on_device) {
    if (!e) return fail(RR_EINVAL, "null env");
    for (int32_t s : {src_slot, dst_slot})
        if (s < RR_SLOT_LIVE || s >= e->n_slots)
            return fail(RR_EINVAL, "rr_copy_envs: slot " + std::to_string(s) + " is not RR_SLOT_LIVE or in [0, " + std::to_string(e->n_slots) + ") (rr_snapshot_slots)");
    const int N = e->P.N;
    const bool host_index = src_index && !index_on_device;
    if (host_index) {
        const int bad = fork_bad_index(src_index, N);
        if (bad >= 0) return fail(RR_EINVAL, "rr_copy_envs: env " + std::to_string(bad) + ": source index " + std::to_string(src_index[bad]) + " is not -1 or in [0, " + std::to_string(N) + ")");
    }
    if (src_slot == dst_slot && !src_index) return RR_OK;      // every record onto itself
    HIPCHK(hipSetDevice(e->cfg.device));
    // whatever has to be allocated is allocated before anything is launched: a failure leaves the handle as it was
    const bool staged = src_slot == dst_slot;                  // (with an index: the map may read envs that it also writes)
    if (staged && !e->fork_stage) RRCHK(mem_get(e, {mem_part(&e->fork_stage, fork_slot_bytes(N), false)}, "rr_copy_envs: allocating the staging slot"));
    const int *idx_dev = src_index;
    if (host_index) {
        if (!e->fork_index) RRCHK(mem_get(e, {mem_part(&e->fork_index, (size_t)N * 4, false)}, "rr_copy_envs: allocating the index staging"));
        // through the pinned ring, as rr_step's commands: the caller may reuse its array at once and nobody waits for the device
        char *pin = nullptr; int pin_idx = -1;
        const int rc = pin_acquire(e, &pin, &pin_idx);
        if (rc != RR_OK) return rc;
        memcpy(pin, src_index, (size_t)N * 4);
        HIPCHK(hipMemcpyAsync(e->fork_index, pin, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipEventRecord(e->pin_ev[pin_idx], e->stream)); e->pin_used[pin_idx] = true;
        idx_dev = e->fork_index;
    }
    const bool to_live = dst_slot == RR_SLOT_LIVE;
    if (to_live) e->la_valid = false;      // the state changes from outside: the next step prepares itself in line (as rr_reset)
    const ForkRec src = fork_rec(e, src_slot), dst = fork_rec(e, dst_slot);
    if (staged) {
        // as if every source were read before any destination is written: staging[i] = src[idx[i]], then dst[i] = staging[i] for the
        // envs with a valid index -- two launches of the same kernel, ordered by the stream
        const ForkRec stage = fork_rec_at(e->fork_stage, N);
        launch_fork(e, src, stage, idx_dev, 0, 0xffffffffu);
        launch_fork(e, stage, dst, idx_dev, 1, fork_err_mask(dst_slot));
    } else launch_fork(e, src, dst, idx_dev, 0, fork_err_mask(dst_slot));
    if (to_live) launch_obs(e);            // the observation buffers and a mapped host mirror follow
    HIPCHK(hipGetLastError());
    return RR_OK;
}


// ---- state writes and reads on the device (rr_write.inc) --------------------------------------------------------------------------------
// On the library's stream, like rr_copy_envs: every rr_step has made that stream wait for its side streams before it returns, so the
// launch is ordered behind every kernel that reads or writes the state -- the look-ahead included -- without a wait of its own.
static void launch_state_rw(rr_env *e, float *aos, const unsigned char *mask_dev, unsigned parts, int to_aos) {
    hipLaunchKernelGGL(k_state_rw, dim3((e->P.N + SW_ENVS - 1) / SW_ENVS), dim3(SW_THREADS), 0, e->stream, e->P, e->D, aos, mask_dev, parts, to_aos);
}

int rr_write_state(rr_env *e, const float *state, const uint8_t *env_mask, uint32_t parts, int32_t on_device) {
    if (!e) return fail(RR_EINVAL, "rr_write_state: null env");
    const uint32_t cols = RR_W_JOINT_POS | RR_W_JOINT_VEL | RR_W_OBJ_POSE | RR_W_OBJ_VEL, all = cols | RR_W_RESET | RR_W_FRESH;
    if (parts & ~all) return fail(RR_EINVAL, "rr_write_state: parts " + std::to_string(parts) + " has a bit outside the six RR_W_* (" + std::to_string(all) + ")");
    if (parts == 0) return fail(RR_EINVAL, "rr_write_state: parts == 0 (nothing to write)");
    if (!state && (parts & cols)) return fail(RR_EINVAL, "rr_write_state: a column group (parts & 15 = " + std::to_string(parts & cols) + ") needs a state tensor");
    HIPCHK(hipSetDevice(e->cfg.device));
    const int N = e->P.N;
    const float *aos = (parts & cols) ? state : nullptr;      // (without a column bit the tensor is not looked at)
    const unsigned char *m = env_mask;
    if (!on_device) {
        if (aos) { HIPCHK(hipMemcpyAsync(e->state_aos, aos, (size_t)N * NSTATE * 4, hipMemcpyHostToDevice, e->stream)); aos = e->state_aos; }
        if (m) { HIPCHK(hipMemcpyAsync(e->mask_dev, m, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    }
    e->la_valid = false;          // the state changes from outside: the next step prepares itself in line (as rr_reset)
    launch_state_rw(e, const_cast<float *>(aos), m, parts, 0);
    launch_obs(e);                // the observation buffers and a mapped host mirror follow
    HIPCHK(hipGetLastError());
    if (!on_device) HIPCHK(hipStreamSynchronize(e->stream));   // the arguments are host memory
    return RR_OK;
}

int rr_read_state(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "rr_read_state: null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    launch_state_rw(e, e->state_aos, nullptr, 0u, 1);
    HIPCHK(hipGetLastError());
    return RR_OK;
}


// ---- device micro-benchmarks for bench.py's roofline (SURVEY 8(d): "achievable" measured in the same run) -------------------
// kind 0: HBM copy (read + write), 1: HBM triad a = b + s c (2 reads + 1 write), 256 MiB per array, float4 per lane, grid-stride;
// kind 2: VALU issue rate of a sample-test-like mix (sub, mul, fma, cmp, cndmask with real dependencies) at the raster kernel's
// shape -- 512-thread workgroups, 39 KB of LDS each, four per CU = eight waves per SIMD (tools/ubench/valu_issue.hip sweeps
// waves per SIMD and instruction kinds; profiles/r04_valu_issue.txt).  Result: GB/s (0, 1) or G wave64-instructions/s (2).
__global__ void __launch_bounds__(256) k_ub_copy(const float4 *__restrict__ a, float4 *__restrict__ b, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) b[i] = a[i];
}
__global__ void __launch_bounds__(256) k_ub_triad(float4 *__restrict__ a, const float4 *__restrict__ b, const float4 *__restrict__ c, float s, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float4 x = b[i], y = c[i];
        a[i] = make_float4(fmaf(s, y.x, x.x), fmaf(s, y.y, x.y), fmaf(s, y.z, x.z), fmaf(s, y.w, x.w));
    }
}
#define UB_S8(x) x x x x x x x x
__global__ void __launch_bounds__(512) k_ub_valu(float *out, int iters, float a, float b) {
    extern __shared__ float ub_lds[];
    float x0 = threadIdx.x * a, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
    for (int it = 0; it < iters; it++) {
        asm volatile(UB_S8("v_sub_f32 %0, %1, %8\n v_mul_f32 %2, %0, %9\n v_fma_f32 %3, %2, %8, %0\n v_cmp_lt_f32 vcc, %3, %9\n"
                           "v_cndmask_b32 %4, %5, %6, vcc\n v_sub_f32 %5, %7, %9\n v_fma_f32 %6, %4, %8, %5\n v_mul_f32 %7, %6, %8\n")
                     : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a), "v"(b) : "vcc");
    }
    const float r = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
    if (r == 12345.678f) ub_lds[threadIdx.x] = r;
    out[(size_t)blockIdx.x * 512 + threadIdx.x] = r;
}
int rr_device_microbench(int32_t device, int32_t kind, double *result) {
    if (!result || kind < 0 || kind > 2) return fail(RR_EINVAL, "rr_device_microbench: bad argument");
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail(RR_EDEVICE, "rr_device_microbench: no such HIP device (no CPU fallback)"); }
    // (everything the measurement allocates is released on every path, it runs on a stream of its own, and the caller's current
    // device is put back)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st = nullptr;
    void *buf[3] = {nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    float best_ms = 1e30f;
    double units = 0.0;
#define UB(call) do { if (err == hipSuccess) err = (call); } while (0)
    hipDeviceProp_t prop;
    UB(hipGetDeviceProperties(&prop, device));
    const int ncu = err == hipSuccess ? prop.multiProcessorCount : 1;
    UB(hipEventCreate(&e0)); UB(hipEventCreate(&e1)); UB(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (kind <= 1) {
        const size_t bytes = (size_t)256 << 20, n4 = bytes / 16;
        for (int i = 0; i < (kind == 0 ? 2 : 3); i++) { UB(hipMalloc(&buf[i], bytes)); UB(hipMemsetAsync(buf[i], 0, bytes, st)); }
        for (int rep = 0; rep < 6 && err == hipSuccess; rep++) {
            UB(hipEventRecord(e0, st));
            if (kind == 0) hipLaunchKernelGGL(k_ub_copy, dim3(ncu * 16), dim3(256), 0, st, (const float4 *)buf[0], (float4 *)buf[1], n4);
            else hipLaunchKernelGGL(k_ub_triad, dim3(ncu * 16), dim3(256), 0, st, (float4 *)buf[0], (const float4 *)buf[1], (const float4 *)buf[2], 0.5f, n4);
            UB(hipEventRecord(e1, st));
            UB(hipEventSynchronize(e1));
            float ms = 0; UB(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && err == hipSuccess) best_ms = std::min(best_ms, ms);
        }
        units = (double)bytes * (kind == 0 ? 2 : 3) / 1e9;                 // GB moved per launch
    } else {
        const int iters = 800, blocks = 4 * ncu;
        UB(hipMalloc(&buf[0], (size_t)blocks * 512 * 4));
        UB(hipFuncSetAttribute((const void *)k_ub_valu, hipFuncAttributeMaxDynamicSharedMemorySize, 39 * 1024));
        for (int rep = 0; rep < 4 && err == hipSuccess; rep++) {
            UB(hipEventRecord(e0, st));
            hipLaunchKernelGGL(k_ub_valu, dim3(blocks), dim3(512), 39 * 1024, st, (float *)buf[0], iters, 1.0001f, 0.5f);
            UB(hipEventRecord(e1, st));
            UB(hipEventSynchronize(e1));
            float ms = 0; UB(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && err == hipSuccess) best_ms = std::min(best_ms, ms);
        }
        units = (double)iters * 64 * blocks * 8 / 1e9;                     // G wave-instructions per launch
    }
    UB(hipGetLastError());
#undef UB
    for (int i = 0; i < 3; i++) if (buf[i]) (void)hipFree(buf[i]);
    if (st) (void)hipStreamDestroy(st);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    if (err != hipSuccess) { (void)hipGetLastError(); return fail(RR_EDEVICE, std::string("rr_device_microbench: ") + hipGetErrorString(err)); }
    *result = units / (best_ms * 1e-3);
    return RR_OK;
}

int rr_map_observations(rr_env *e, void **host_ptr, size_t *bytes) {
    if (!e || !host_ptr) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    const size_t N = e->P.N, nobj = e->P.nobj;
    const size_t nb = 4 * (N * 9 + N * 4 + N * nobj * 7 + N + N);
    if (!e->obs_host) {
        void *h = nullptr, *d = nullptr;
        RRCHK(mem_get(e, {mem_part(&h, nb, true, MEM_PINNED_MAPPED)}, "rr_map_observations: allocating the mapped block"));
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { e->mem.release(h); (void)hipGetLastError(); return fail(RR_EDEVICE, "rr_map_observations: pinned host memory is not device-mapped on this system"); }
        float *f = (float *)d;
        e->obs_dev.joints = f; e->obs_dev.touch = f + N * 9; e->obs_dev.objpose = f + N * 13;
        e->obs_dev.timestep = (int *)(f + N * (13 + nobj * 7)); e->obs_dev.errflags = (unsigned *)(f + N * (14 + nobj * 7));
        e->obs_host = h;
        launch_mirror(e);
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    *host_ptr = e->obs_host;
    if (bytes) *bytes = nb;
    return RR_OK;
}

int rr_sync_observations(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    if (e->ev_obs_set) HIPCHK(hipEventSynchronize(e->ev_obs)); else HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_map_images(rr_env *e, void **rgb_host, void **depth_host, void **mask_host) {
    if (!e) return fail(RR_EINVAL, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    void **out[3] = {rgb_host, depth_host, mask_host};
    const int f[3] = {RR_F_RGB, RR_F_DEPTH, RR_F_MASK};
    size_t total = 0;
    for (int i = 0; i < 3; i++) if (out[i]) total += e->field_bytes[f[i]];
    if (total > ((size_t)256 << 20)) return fail(RR_EINVAL, "rr_map_images: more than 256 MiB of images per step (meant for a handful of envs; batches read the device buffers)");
    for (int i = 0; i < 3; i++) {
        if (!out[i]) continue;
        if (!e->field_ptr[f[i]]) return fail(RR_EINVAL, "rr_map_images: field not available (RR_FLAG_NO_MASK)");
        if (!e->img_host[i]) {
            RRCHK(mem_get(e, {mem_part(&e->img_host[i], e->field_bytes[f[i]], false, MEM_PINNED)}, "rr_map_images: allocating the pinned copy"));
            HIPCHK(hipMemcpyAsync(e->img_host[i], e->field_ptr[f[i]], e->field_bytes[f[i]], hipMemcpyDeviceToHost, e->stream));
        }
        *out[i] = e->img_host[i];
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_select_image_mirror(rr_env *e, int32_t fields) {
    if (!e) return fail(RR_EINVAL, "null env");
    if (fields < 0 || fields > 7) return fail(RR_EINVAL, "rr_select_image_mirror: fields is a mask of 1 (RGB), 2 (depth), 4 (mask)");
    HIPCHK(hipSetDevice(e->cfg.device));
    const int f[3] = {RR_F_RGB, RR_F_DEPTH, RR_F_MASK};
    const int fresh = fields & ~e->img_sel;          // selected again: the block is brought up to date with the device buffer at once
    e->img_sel = fields;
    bool copied = false;
    for (int i = 0; i < 3; i++)
        if (((fresh >> i) & 1) && e->img_host[i] && e->field_ptr[f[i]]) {
            HIPCHK(hipMemcpyAsync(e->img_host[i], e->field_ptr[f[i]], e->field_bytes[f[i]], hipMemcpyDeviceToHost, e->stream));
            copied = true;
        }
    if (copied) {
        if (!e->ev_obs) HIPCHK(hipEventCreateWithFlags(&e->ev_obs, hipEventDisableTiming));
        HIPCHK(hipEventRecord(e->ev_obs, e->stream));
        e->ev_obs_set = true;
    }
    return RR_OK;
}

int rr_sync(rr_env *e) {
    if (!e) return fail(RR_EINVAL, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_link_poses(rr_env *e, float *out_host) {
    if (!e || !out_host) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    hipLaunchKernelGGL(k_link_poses, dim3((e->P.N + 63) / 64), dim3(64), 0, e->stream, e->B, e->P, e->RM_dev, e->D, e->link_out);
    HIPCHK(hipMemcpyAsync(out_host, e->link_out, (size_t)e->P.N * e->RM.nl * 28, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_get_contacts(rr_env *e, int32_t env_index, float *out_host, int32_t max_contacts, int32_t *count) {
    if (!e || !out_host || !count) return fail(RR_EINVAL, "null argument");
    if (env_index < 0 || env_index >= e->P.N) return fail(RR_EINVAL, "rr_get_contacts: env out of range");
    HIPCHK(hipSetDevice(e->cfg.device));
    int nc = 0;
    float rec[MAXC * 12], force[MAXC];
    HIPCHK(hipMemcpyAsync(&nc, e->D.ccount + env_index, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(rec, e->D.clist + (size_t)env_index * MAXC * 3, sizeof rec, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(force, e->D.cforce + (size_t)env_index * MAXC, sizeof force, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    nc = std::max(0, std::min(nc, std::min((int)MAXC, (int)max_contacts)));
    for (int c = 0; c < nc; c++) {      // device record {x y z nx | ny nz dist meta | mu rest roll spin} -> {bodyA, bodyB, linkA, x, n, dist, force, mu}
        const float *r = rec + 12 * c;
        int meta;
        memcpy(&meta, r + 7, 4);
        float *o = out_host + 12 * c;
        o[0] = (float)(signed char)(meta & 255); o[1] = (float)(signed char)((meta >> 8) & 255); o[2] = (float)(signed char)((meta >> 16) & 255);
        o[3] = r[0]; o[4] = r[1]; o[5] = r[2]; o[6] = r[3]; o[7] = r[4]; o[8] = r[5]; o[9] = r[6]; o[10] = force[c]; o[11] = r[8];
    }
    *count = nc;
    return RR_OK;
}

int rr_evaluate_goals(rr_env *e, const float *goal_pos_host, const uint8_t *goal_mask_host, float *score_out_host) {
    if (!e || !goal_pos_host || !score_out_host) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    const size_t N = e->P.N, nobj = e->P.nobj;
    if (!e->score_out) RRCHK(mem_get(e, {mem_part(&e->score_out, N * 4), mem_part(&e->score_mask, N * NOBJ)}, "rr_evaluate_goals: allocating the score buffers"));
    static_assert(NSTATE >= NOBJ * 3, "the state staging buffer doubles as goal-position staging");
    HIPCHK(hipMemcpyAsync(e->state_aos, goal_pos_host, N * nobj * 12, hipMemcpyHostToDevice, e->stream));
    if (goal_mask_host) HIPCHK(hipMemcpyAsync(e->score_mask, goal_mask_host, N * nobj, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_goal_score, dim3((e->P.N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, e->state_aos, goal_mask_host ? e->score_mask : nullptr, e->score_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(score_out_host, e->score_out, N * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

static int ensure_plan_buffers(rr_env *e, const char *who) {
    if (e->plan) return RR_OK;
    const size_t N = e->P.N;
    return mem_get(e, {mem_part(&e->plan, N * PLAN_LEN * 36), mem_part(&e->plan_step, N * 4), mem_part(&e->ik_in, N * 28), mem_part(&e->ik_out, N * 44),
                       mem_part(&e->ik_err, N * 4)}, who);
}

int rr_ik(rr_env *e, const float *targets_host, float *q_out_host, float *err_out_host) {
    if (!e || !targets_host || !q_out_host) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    int rc = ensure_plan_buffers(e, "rr_ik: allocating the plan and IK buffers");
    if (rc != RR_OK) return rc;
    const int N = e->P.N;
    HIPCHK(hipMemcpyAsync(e->ik_in, targets_host, (size_t)N * 28, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_ik, dim3((N + 63) / 64), dim3(64), 0, e->stream, e->IK, e->P, e->D, e->ik_in, e->ik_out, e->ik_err);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q_out_host, e->ik_out, (size_t)N * 44, hipMemcpyDeviceToHost, e->stream));
    if (err_out_host) HIPCHK(hipMemcpyAsync(err_out_host, e->ik_err, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_plan_macro(rr_env *e, const float *macro_host, const uint8_t *env_mask_host) {
    if (!e || !macro_host) return fail(RR_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->cfg.device));
    int rc = ensure_plan_buffers(e, "rr_plan_macro: allocating the plan and IK buffers");
    if (rc != RR_OK) return rc;
    const int N = e->P.N;
    // the macro targets travel through the (otherwise idle) ik_out staging buffer: [N][4]
    HIPCHK(hipMemcpyAsync(e->ik_out, macro_host, (size_t)N * 16, hipMemcpyHostToDevice, e->stream));
    const unsigned char *m = nullptr;
    if (env_mask_host) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask_host, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_plan_macro, dim3((N + 63) / 64), dim3(64), 0, e->stream, e->IK, e->P, e->D, e->ik_out, m, e->plan, e->plan_step);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_get_plan(rr_env *e, int32_t env_index, float *plan_host) {
    if (!e || !plan_host) return fail(RR_EINVAL, "null argument");
    if (!e->plan) return fail(RR_EINVAL, "rr_get_plan: no plan was generated");
    if (env_index < 0 || env_index >= e->P.N) return fail(RR_EINVAL, "rr_get_plan: env out of range");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(plan_host, e->plan + (size_t)env_index * PLAN_LEN * 9, PLAN_LEN * 36, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_step_plan_masked(rr_env *e, const uint8_t *idle_mask_host, int32_t render_mode, const uint8_t *render_flags_host) {
    if (!e) return fail(RR_EINVAL, "null env");
    if (!e->plan) return fail(RR_EINVAL, "rr_step_plan: call rr_plan_macro first");
    // (checked here as well: k_plan_fetch advances the plan positions, which must not happen for a step rr_step then rejects)
    if (render_mode < 0 || render_mode > 2 || (render_mode == 2 && !render_flags_host)) return fail(RR_EINVAL, "rr_step_plan: bad render_mode");
    HIPCHK(hipSetDevice(e->cfg.device));
    const unsigned char *idle = nullptr;
    if (idle_mask_host) { HIPCHK(hipMemcpyAsync(e->mask_dev, idle_mask_host, e->P.N, hipMemcpyHostToDevice, e->stream)); idle = e->mask_dev; }
    hipLaunchKernelGGL(k_plan_fetch, dim3((e->P.N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, e->plan, e->plan_step, idle);
    return rr_step(e, e->D.cmd, 1, render_mode, render_flags_host);
}

int rr_step_plan(rr_env *e, int32_t render_mode, const uint8_t *render_flags_host) {
    return rr_step_plan_masked(e, nullptr, render_mode, render_flags_host);
}

// ---- device-resident macro actions (rr_macro.inc) -----------------------------------------------------------------------------------------
// The record, the need list and the `replanned` bytes on first use, with the plan and IK buffers where the handle has none yet: one
// group, all or nothing.  The record starts all NaN (one launch behind the allocation): no request equals it.
static int ensure_macro(rr_env *e, const char *who) {
    if (e->macro_req) return RR_OK;
    const size_t N = e->P.N;
    RRCHK(ensure_group(e, -1, who, "the macro record and the plan buffers",
                       {mem_part(&e->macro_req, N * 16), mem_part(&e->macro_list, (N + 1) * 4), mem_part(&e->macro_replanned, N),
                        mem_part(&e->plan, N * PLAN_LEN * 36), mem_part(&e->plan_step, N * 4), mem_part(&e->ik_in, N * 28), mem_part(&e->ik_out, N * 44),
                        mem_part(&e->ik_err, N * 4)}));
    hipLaunchKernelGGL(k_macro_invalidate, dim3((unsigned)((N * 4 + 255) / 256)), dim3(256), 0, e->stream, (int)N, (const unsigned char *)nullptr, e->macro_req);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// One step of macro actions decided on the device.  Launch order on the main stream: staging (host arguments only), k_macro_decide,
// k_macro_replan, k_plan_fetch, rr_step.  Device arguments are read in place and nothing waits; host arguments go through the staging
// helper, whose wait stands at the end because they are host memory.  The grid of k_macro_replan is sized from N (up to MR_WAVES
// listed envs a workgroup each, beyond that ceil(count / MR_WAVES) envs per workgroup, at most MR_SLOTS): the list's length stays on the
// device.
int rr_step_macro(rr_env *e, const float *macro, int32_t macro_on_device, const uint8_t *idle, int32_t idle_on_device, int32_t render_mode,
                  const uint8_t *render_flags_host) {
    if (!e) return fail(RR_EINVAL, "rr_step_macro: null env");
    if (!macro) return fail(RR_EINVAL, "rr_step_macro: null macro");
    // (checked here as well: the decision moves records and plan positions, which must not happen for a step rr_step then rejects)
    if (render_mode < 0 || render_mode > 2 || (render_mode == 2 && !render_flags_host)) return fail(RR_EINVAL, "rr_step_macro: bad render_mode");
    if (idle && !macro_on_device != !idle_on_device)
        return fail(RR_EINVAL, std::string("rr_step_macro: macro and idle must live on the same side (macro on the ") + (macro_on_device ? "device" : "host") +
                                   ", idle on the " + (idle_on_device ? "device" : "host") + ")");
    HIPCHK(hipSetDevice(e->cfg.device));
    RRCHK(ensure_macro(e, "rr_step_macro"));
    const int N = e->P.N;
    const HostStaging st = {e, !macro_on_device};
    // (a host request travels through the otherwise idle ik_out staging buffer, as in rr_plan_macro; a host idle mask through mask_dev)
    RRCHK(st.in(macro, e->ik_out, (size_t)N * 16));
    const unsigned char *idle_dev = idle;
    if (idle && !idle_on_device) { HIPCHK(hipMemcpyAsync(e->mask_dev, idle, N, hipMemcpyHostToDevice, e->stream)); idle_dev = e->mask_dev; }
    hipLaunchKernelGGL(k_macro_decide, dim3(1), dim3(MD_THREADS), 0, e->stream, N, macro, idle_dev, e->macro_req, e->plan_step, e->macro_replanned, e->macro_list);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_macro_replan, dim3((unsigned)std::min(N, std::max(MR_WAVES, (N + MR_SLOTS - 1) / MR_SLOTS))), dim3(64), 0, e->stream, e->IK, e->P, e->D, (const float *)e->macro_req, (const int *)e->macro_list, e->plan);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_plan_fetch, dim3((N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, e->plan, e->plan_step, idle_dev);
    HIPCHK(hipGetLastError());
    const int rc = rr_step(e, e->D.cmd, 1, render_mode, render_flags_host);
    const int rw = st.wait();
    return rc != RR_OK ? rc : rw;
}

int rr_macro_invalidate(rr_env *e, const uint8_t *env_mask, int32_t mask_on_device) {
    if (!e) return fail(RR_EINVAL, "rr_macro_invalidate: null env");
    if (!e->macro_req) return RR_OK;      // no record yet: it is created all NaN
    HIPCHK(hipSetDevice(e->cfg.device));
    const int N = e->P.N;
    const unsigned char *m = env_mask;
    const bool host_mask = env_mask && !mask_on_device;
    if (host_mask) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_macro_invalidate, dim3((unsigned)((N * 4 + 255) / 256)), dim3(256), 0, e->stream, N, m, e->macro_req);
    HIPCHK(hipGetLastError());
    if (host_mask) HIPCHK(hipStreamSynchronize(e->stream));   // the argument is host memory
    return RR_OK;
}

static int macro_field(rr_env *e, int32_t which, void **ptr, size_t *bytes, const char *who) {
    if (!e || which < 0 || which >= RR_MACRO_COUNT) return fail(RR_EINVAL, std::string(who) + ": bad buffer");
    HIPCHK(hipSetDevice(e->cfg.device));
    RRCHK(ensure_macro(e, who));
    const size_t N = e->P.N;
    void *const p[RR_MACRO_COUNT] = {e->macro_req, e->plan_step, e->macro_replanned, e->plan};
    const size_t b[RR_MACRO_COUNT] = {N * 16, N * 4, N, N * PLAN_LEN * 36};
    *ptr = p[which]; *bytes = b[which];
    return RR_OK;
}

int rr_macro_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) {
    void *p = nullptr; size_t b = 0;
    RRCHK(macro_field(e, which, &p, &b, "rr_macro_buffer"));
    if (dev_ptr) *dev_ptr = p;
    if (bytes) *bytes = b;
    return RR_OK;
}

int rr_macro_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) {
    if (!dst) return fail(RR_EINVAL, "rr_macro_copy_to_host: null destination");
    void *p = nullptr; size_t b = 0;
    RRCHK(macro_field(e, which, &p, &b, "rr_macro_copy_to_host"));
    if (bytes != b) return fail(RR_EINVAL, "rr_macro_copy_to_host: size mismatch");
    HIPCHK(hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

// ---- device-resident cartesian actions (rr_cart.inc) ------------------------------------------------------------------------------------
// The record, its solution and residual, the `solved` bytes, the need list and the staging of a host caller's targets and gripper
// commands on first use: one group, all or nothing.  The record starts all NaN (one launch behind the allocation): no request equals it.
static int ensure_cartesian(rr_env *e, const char *who) {
    if (e->cart_req) return RR_OK;
    const size_t N = e->P.N;
    RRCHK(ensure_group(e, -1, who, "the cartesian record, solution and list",
                       {mem_part(&e->cart_req, N * 28), mem_part(&e->cart_sol, N * 28), mem_part(&e->cart_res, N * 4), mem_part(&e->cart_solved, N),
                        mem_part(&e->cart_list, (N + 1) * 4), stage_part(&e->cart_stage, N * 36)}));
    hipLaunchKernelGGL(k_cart_invalidate, dim3((unsigned)((N * 7 + 255) / 256)), dim3(256), 0, e->stream, (int)N, (const unsigned char *)nullptr, e->cart_req);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// Whether the runtime knows `p` to live on the other side than the flag says: pageable host memory under on_device (a kernel could not
// read it), device memory under !on_device.  Pinned and managed memory serve either side.  A host-side table lookup: no wait.
static bool cart_other_side(const void *p, bool on_device) {
    hipPointerAttribute_t a = {};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return on_device; }      // (unknown to the runtime: pageable host memory)
    return on_device ? a.type == hipMemoryTypeUnregistered : a.type == hipMemoryTypeDevice;
}

// One step of cartesian actions decided on the device.  Launch order on the main stream: staging (host arguments only), k_cart_decide,
// k_cart_solve, k_cart_fetch, rr_step.  Device arguments are read in place and nothing waits; host arguments go through the staging
// helper, whose wait stands at the end because they are host memory.  The grid of k_cart_solve is sized from N (up to CS_WAVES listed
// envs a workgroup each, beyond that ceil(count / CS_WAVES) envs per workgroup, at most CS_SLOTS): the list's length stays on the device.
int rr_step_cartesian(rr_env *e, const float *cartesian, const float *gripper, const uint8_t *idle, int32_t on_device, int32_t render_mode,
                      const uint8_t *render_flags_host) {
    if (!e) return fail(RR_EINVAL, "rr_step_cartesian: null env");
    if (!cartesian) return fail(RR_EINVAL, "rr_step_cartesian: null cartesian");
    if (!gripper) return fail(RR_EINVAL, "rr_step_cartesian: null gripper");
    // (checked here as well: the decision moves records, which must not happen for a step rr_step then rejects)
    if (render_mode < 0 || render_mode > 2 || (render_mode == 2 && !render_flags_host)) return fail(RR_EINVAL, "rr_step_cartesian: bad render_mode");
    HIPCHK(hipSetDevice(e->cfg.device));
    // one flag covers the three arrays: an array the runtime knows to live on the other side makes the set a mixed one
    const void *const arrays[3] = {cartesian, gripper, idle};
    static const char *const names[3] = {"cartesian", "gripper", "idle"};
    for (int i = 0; i < 3; i++)
        if (arrays[i] && cart_other_side(arrays[i], on_device != 0))
            return fail(RR_EINVAL, std::string("rr_step_cartesian: cartesian, gripper and idle must live on the same side (on_device says the ") +
                                       (on_device ? "device" : "host") + ", " + names[i] + " is on the " + (on_device ? "host" : "device") + ")");
    RRCHK(ensure_cartesian(e, "rr_step_cartesian"));
    const int N = e->P.N;
    const HostStaging st = {e, !on_device};
    // (host targets and gripper commands travel through the group's own staging block, [N][7] then [N][2]; a host idle mask through mask_dev)
    RRCHK(st.in(cartesian, e->cart_stage, (size_t)N * 28));
    RRCHK(st.in(gripper, e->cart_stage + (size_t)N * 7, (size_t)N * 8));
    const unsigned char *idle_dev = idle;
    if (idle && !on_device) { HIPCHK(hipMemcpyAsync(e->mask_dev, idle, N, hipMemcpyHostToDevice, e->stream)); idle_dev = e->mask_dev; }
    hipLaunchKernelGGL(k_cart_decide, dim3(1), dim3(MD_THREADS), 0, e->stream, N, cartesian, idle_dev, e->cart_req, e->cart_solved, e->cart_list);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cart_solve, dim3((unsigned)std::min(N, std::max(CS_WAVES, (N + CS_SLOTS - 1) / CS_SLOTS))), dim3(64), 0, e->stream, e->IK, e->P, e->D, (const float *)e->cart_req, (const int *)e->cart_list, e->cart_sol, e->cart_res);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cart_fetch, dim3((N + 255) / 256), dim3(256), 0, e->stream, e->P, e->D, (const float *)e->cart_sol, gripper, idle_dev);
    HIPCHK(hipGetLastError());
    const int rc = rr_step(e, e->D.cmd, 1, render_mode, render_flags_host);
    const int rw = st.wait();
    return rc != RR_OK ? rc : rw;
}

int rr_cartesian_invalidate(rr_env *e, const uint8_t *env_mask, int32_t mask_on_device) {
    if (!e) return fail(RR_EINVAL, "rr_cartesian_invalidate: null env");
    if (!e->cart_req) return RR_OK;      // no record yet: it is created all NaN
    HIPCHK(hipSetDevice(e->cfg.device));
    const int N = e->P.N;
    const unsigned char *m = env_mask;
    const bool host_mask = env_mask && !mask_on_device;
    if (host_mask) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    hipLaunchKernelGGL(k_cart_invalidate, dim3((unsigned)((N * 7 + 255) / 256)), dim3(256), 0, e->stream, N, m, e->cart_req);
    HIPCHK(hipGetLastError());
    if (host_mask) HIPCHK(hipStreamSynchronize(e->stream));   // the argument is host memory
    return RR_OK;
}

static int cartesian_field(rr_env *e, int32_t which, void **ptr, size_t *bytes, const char *who) {
    if (!e || which < 0 || which >= RR_CART_COUNT) return fail(RR_EINVAL, std::string(who) + ": bad buffer");
    HIPCHK(hipSetDevice(e->cfg.device));
    RRCHK(ensure_cartesian(e, who));
    const size_t N = e->P.N;
    void *const p[RR_CART_COUNT] = {e->cart_req, e->cart_sol, e->cart_res, e->cart_solved};
    const size_t b[RR_CART_COUNT] = {N * 28, N * 28, N * 4, N};
    *ptr = p[which]; *bytes = b[which];
    return RR_OK;
}

int rr_cartesian_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) {
    void *p = nullptr; size_t b = 0;
    RRCHK(cartesian_field(e, which, &p, &b, "rr_cartesian_buffer"));
    if (dev_ptr) *dev_ptr = p;
    if (bytes) *bytes = b;
    return RR_OK;
}

int rr_cartesian_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) {
    if (!dst) return fail(RR_EINVAL, "rr_cartesian_copy_to_host: null destination");
    void *p = nullptr; size_t b = 0;
    RRCHK(cartesian_field(e, which, &p, &b, "rr_cartesian_copy_to_host"));
    if (bytes != b) return fail(RR_EINVAL, "rr_cartesian_copy_to_host: size mismatch");
    HIPCHK(hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

// ---- per-env static layers: per-env cameras (rr_set_env_cameras) and per-env appearance (rr_set_env_appearance) -------------
// Both need an env's own static layer -- its camera projects the never-moving instances, its light shades them, its colours
// paint them -- and share one mode: the buffers below (19 bytes per pixel per env, allocated by whichever call comes first), a
// camera record per env (the handle's camera for every env while only the appearance is per env), and one rebuild.  The handle
// remembers which of the two settings is in force (cam_per_env, app_per_env); the mode lasts while either holds.
static int ensure_env_layers(rr_env *e, const char *who) {
    if (e->cam_dev) return RR_OK;
    const int N = e->P.N, CF = cam_floats(e->RM.ntiles);
    const size_t px = (size_t)e->RM.W * e->RM.H;
    RRCHK(mem_get(e, {mem_part(&e->cam_dev, (size_t)N * CF * 4), mem_part(&e->cam_sel, (size_t)N * 4),
                      mem_part(&e->env_static_vis, N * px * 8, false), mem_part(&e->env_static_rgb, N * px * 3, false),
                      mem_part(&e->env_static_depth, N * px * 4, false), mem_part(&e->env_static_mask, N * px * 4, false)}, who));
    e->cam_host.assign((size_t)N * CF, 0.0f);
    return RR_OK;
}
static dim3 env_layer_copy_grid(const rr_env *e) {
    const size_t px = (size_t)e->RM.W * e->RM.H;
    return dim3(std::min(16, (int)((px / 4 + COPY_THREADS - 1) / COPY_THREADS)), std::min(e->P.N, 65535));
}
// the handle's camera as the record of env i
static void env_camera_from_handle(rr_env *e, int i) {
    const RenderModel &RM = e->RM;
    float *rec = e->cam_host.data() + (size_t)i * cam_floats(RM.ntiles);
    memcpy(rec + CAM_VP, RM.VP, sizeof RM.VP);
    memcpy(rec + CAM_PN, RM.plane_norm, sizeof RM.plane_norm);
    memcpy(rec + CAM_TP, RM.tile_plane, sizeof(float) * 8 * RM.ntiles);
}
// Entering the mode (no-op inside it): every env has the handle's camera and a copy of the shared static layer.
static int enter_env_layers(rr_env *e) {
    if (e->D.env_cam) return RR_OK;
    const int N = e->P.N;
    const size_t px = (size_t)e->RM.W * e->RM.H;
    for (int i = 0; i < N; i++) env_camera_from_handle(e, i);
    ImageOut layers;
    layers.rgb = e->env_static_rgb; layers.depth = e->env_static_depth; layers.mask = e->env_static_mask; layers.env_stride = px;
    const dim3 copy_grid = env_layer_copy_grid(e);
    hipLaunchKernelGGL(k_static_copy, copy_grid, dim3(COPY_THREADS), 0, e->stream, e->RM_dev, e->D, layers, 0, N, (const unsigned char *)nullptr);
    hipLaunchKernelGGL(k_static_vis_spread, copy_grid, dim3(COPY_THREADS), 0, e->stream, (const unsigned long long *)e->shared_static_vis, e->env_static_vis, px, N);
    HIPCHK(hipGetLastError());
    e->D.env_cam = e->cam_dev; e->D.static_stride = px;
    e->D.static_vis = e->D.static_vis_out = e->env_static_vis; e->D.static_rgb = e->env_static_rgb;
    e->D.static_depth = e->env_static_depth; e->D.static_mask = e->env_static_mask;
    return RR_OK;
}
// Leaving it: every env shares the handle's camera and static layer again (the caller rebuilds that layer).
static void leave_env_layers(rr_env *e) {
    e->D.env_cam = nullptr; e->D.static_stride = 0;
    e->D.static_vis = e->D.static_vis_out = e->shared_static_vis; e->D.static_rgb = e->shared_static_rgb;
    e->D.static_depth = e->shared_static_depth; e->D.static_mask = e->shared_static_mask;
}
// The rebuild of the static layers of the envs whose mask byte is set (nullptr: all), from the host's camera records and whatever
// appearance e->D points at: build_static_layer's launches over a grid of all envs, of which only the masked ones stay (class
// array cam_sel, sel 1) -- background, instance set-up, pass-1 visibility with the env's own fragment list as scratch, shading
// into its layer.  Their lists are emptied and, once images exist, they become stale (a full copy of their own layer at their
// next render).  The other envs are not touched.
static int rebuild_env_layers(rr_env *e, const uint8_t *env_mask_host, const char *who) {
    const RenderModel &RM = e->RM;
    const int N = e->P.N, CF = cam_floats(RM.ntiles);
    const size_t px = (size_t)RM.W * RM.H;
    std::vector<int> sel(N, 1);
    std::vector<uint8_t> mask(N, 0);
    for (int i = 0; i < N; i++)
        if (!env_mask_host || env_mask_host[i]) { sel[i] = 0; mask[i] = 1; }
    HIPCHK(hipMemcpyAsync(e->cam_dev, e->cam_host.data(), sizeof(float) * N * CF, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->cam_sel, sel.data(), sizeof(int) * N, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->mask_dev, mask.data(), N, hipMemcpyHostToDevice, e->stream));
    DevPtrs Db = e->D;
    Db.static_vis = nullptr; Db.hgflag = e->cam_sel;
    ImageOut layers;
    layers.rgb = Db.static_rgb; layers.depth = Db.static_depth; layers.mask = Db.static_mask; layers.env_stride = px;
    hipLaunchKernelGGL(k_background, env_layer_copy_grid(e), dim3(256), 0, e->stream, e->RM_dev, Db, N, (const unsigned char *)e->mask_dev);
    hipLaunchKernelGGL(k_render_setup, dim3((N * MAXINST + 63) / 64), dim3(64), 0, e->stream, e->B, e->P, e->RM_dev, Db, 1);
    hipLaunchKernelGGL(k_raster, dim3(N, RM.ntiles), dim3(RASTER_THREADS), 0, e->stream, e->P, e->RM_dev, Db, e->n_inst_used, 1, 0, 0, 1);
    hipLaunchKernelGGL(k_shade, dim3(N, RM.ntiles, SHADE_SPLIT), dim3(SHADE_THREADS), 0, e->stream, e->RM_dev, Db, layers, 0, 0, 1, 0, (unsigned *)nullptr);
    hipLaunchKernelGGL(k_camera_changed, dim3((N + 255) / 256), dim3(256), 0, e->stream, e->RM_dev, e->D, N, (const unsigned char *)e->mask_dev,
                       e->images_valid ? e->stale_dev : (unsigned char *)nullptr);
    HIPCHK(hipGetLastError());
    if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(RR_EDEVICE, std::string(who) + ": static layer pass failed");
    if (e->images_valid) e->stale_any = true;
    return RR_OK;
}

// Replaces the fixed eye camera by an arbitrary one (row-major 4x4 view and projection, OpenGL conventions) and rebuilds
// the static layer. Used for the debug camera of render('rgb_array') (EnvCamera, env.py:470-513).  Ends per-env cameras; with a
// per-env appearance in force the per-env layers stay: every env gets this camera and its layer is rebuilt.
int rr_set_camera(rr_env *e, const float *view16, const float *proj16) {
    if (!e || (!view16) != (!proj16)) return fail(RR_EINVAL, "rr_set_camera: null argument (both matrices, or neither for the default eye)");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->cam_per_env = false;
    if (e->D.env_cam && !e->app_per_env) leave_env_layers(e);
    if (!view16) look_at_persp(e->RM.VP, e->table_pos, e->RM.W, e->RM.H);       // back to the reference's eye camera (env.py:136-141, 253-255)
    else camera_vp(view16, proj16, e->RM.VP);
    frustum_plane_norms(e->RM, e->RM.VP, e->RM.plane_norm, e->RM.tile_plane);
    HIPCHK(hipMemcpy(e->RM_dev, &e->RM, sizeof e->RM, hipMemcpyHostToDevice));
    if (e->D.env_cam) {
        for (int i = 0; i < e->P.N; i++) env_camera_from_handle(e, i);
        return rebuild_env_layers(e, nullptr, "rr_set_camera");
    }
    return build_static_layer(e);
}

// Per-env cameras.  Entering per-env mode starts every env from the handle's camera and a copy of its static layer.  The masked
// envs then get their record (camera_vp and frustum_plane_norms, as rr_set_camera) and their layer is rebuilt
// (rebuild_env_layers).  The other envs are not touched.
int rr_set_env_cameras(rr_env *e, const float *views16, const float *projs16, const uint8_t *env_mask_host) {
    if (!e || !views16 || !projs16) return fail(RR_EINVAL, "rr_set_env_cameras: null argument");
    const int N = e->P.N;
    for (int i = 0; i < N; i++) {
        if (env_mask_host && !env_mask_host[i]) continue;
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(views16[16 * (size_t)i + k]) || !std::isfinite(projs16[16 * (size_t)i + k]))
                return fail(RR_EINVAL, "rr_set_env_cameras: non-finite matrix of env " + std::to_string(i) + " (no env changed)");
    }
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const RenderModel &RM = e->RM;
    const int CF = cam_floats(RM.ntiles);
    int rc;
    if ((rc = ensure_env_layers(e, "rr_set_env_cameras: allocating the per-env static layers")) != RR_OK || (rc = enter_env_layers(e)) != RR_OK) return rc;
    e->cam_per_env = true;
    for (int i = 0; i < N; i++) {
        if (env_mask_host && !env_mask_host[i]) continue;
        float *rec = e->cam_host.data() + (size_t)i * CF;
        camera_vp(views16 + 16 * (size_t)i, projs16 + 16 * (size_t)i, rec + CAM_VP);
        frustum_plane_norms(RM, rec + CAM_VP, rec + CAM_PN, (float (*)[8])(rec + CAM_TP));
    }
    return rebuild_env_layers(e, env_mask_host, "rr_set_env_cameras");
}

// ---- per-env appearance ----------------------------------------------------------------------------------------------------
// The light every env has until it is given one: shade_light's literals, in the same float32 operations (the sum of the
// squares is an integer, the square root and the quotient are correctly rounded on both sides): the same bits.
static void unit_light(const float *l, float *out4) {
#pragma clang fp contract(off)
    const float linv = 1.0f / sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    out4[0] = l[0] * linv; out4[1] = l[1] * linv; out4[2] = l[2] * linv; out4[3] = 0.0f;
}
static void default_light(float *out4) {
    const float l[3] = {-50.0f, 30.0f, 100.0f};
    unit_light(l, out4);
}
static void default_appearance(rr_env *e) {
    const int N = e->P.N;
    e->colour_host.assign((size_t)N * MAXINST * 3, 0.0f);
    e->light_host.assign((size_t)N * 4, 0.0f);
    for (int i = 0; i < N; i++) {
        memcpy(e->colour_host.data() + (size_t)i * MAXINST * 3, e->RM.in_color, sizeof e->RM.in_color);
        default_light(e->light_host.data() + (size_t)i * 4);
    }
}

int rr_set_env_appearance(rr_env *e, const float *colours, const float *light_dirs, const uint8_t *env_mask_host) {
    if (!e) return fail(RR_EINVAL, "null env");
    if (!colours && !light_dirs && env_mask_host) return fail(RR_EINVAL, "rr_set_env_appearance: an env mask without colours or light directions");
    const int N = e->P.N, ni = e->RM.ni;
    for (int i = 0; i < N; i++) {
        if (env_mask_host && !env_mask_host[i]) continue;
        if (colours)
            for (int k = 0; k < ni * 3; k++) {
                const float c = colours[(size_t)i * ni * 3 + k];
                if (!std::isfinite(c) || c < 0.0f)
                    return fail(RR_EINVAL, "rr_set_env_appearance: negative or non-finite colour of env " + std::to_string(i) + " (no env changed)");
            }
        if (light_dirs) {
            const float *l = light_dirs + 3 * (size_t)i;
            const float n2 = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];      // (float32, as the normalisation: an overflow is refused here)
            if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !std::isfinite(n2) || !(sqrtf(n2) > 1e-6f))
                return fail(RR_EINVAL, "rr_set_env_appearance: light direction of env " + std::to_string(i) + " is not finite or shorter than 1e-6 (no env changed)");
        }
    }
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipStreamSynchronize(e->stream));
    int rc;
    if (!colours && !light_dirs) {          // back to the model's appearance for every env
        if (!e->app_per_env) return RR_OK;
        e->app_per_env = false;
        e->D.env_colour = nullptr; e->D.env_light = nullptr;
        default_appearance(e);
        if (e->cam_per_env) return rebuild_env_layers(e, nullptr, "rr_set_env_appearance");      // the cameras stay per env
        leave_env_layers(e);
        return build_static_layer(e);
    }
    if (!e->colour_dev) {
        RRCHK(mem_get(e, {mem_part(&e->colour_dev, (size_t)N * MAXINST * 12, false), mem_part(&e->light_dev, (size_t)N * 16, false)},
                      "rr_set_env_appearance: allocating the appearance tables"));
        default_appearance(e);
    }
    if ((rc = ensure_env_layers(e, "rr_set_env_appearance: allocating the per-env static layers")) != RR_OK || (rc = enter_env_layers(e)) != RR_OK) return rc;
    e->app_per_env = true;
    for (int i = 0; i < N; i++) {
        if (env_mask_host && !env_mask_host[i]) continue;
        if (colours) memcpy(e->colour_host.data() + (size_t)i * MAXINST * 3, colours + (size_t)i * ni * 3, sizeof(float) * ni * 3);
        if (light_dirs) unit_light(light_dirs + 3 * (size_t)i, e->light_host.data() + (size_t)i * 4);
    }
    HIPCHK(hipMemcpyAsync(e->colour_dev, e->colour_host.data(), sizeof(float) * e->colour_host.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->light_dev, e->light_host.data(), sizeof(float) * e->light_host.size(), hipMemcpyHostToDevice, e->stream));
    e->D.env_colour = e->colour_dev; e->D.env_light = e->light_dev;
    return rebuild_env_layers(e, env_mask_host, "rr_set_env_appearance");
}

int rr_get_env_appearance(rr_env *e, float *colours_out, float *light_dirs_out) {
    if (!e) return fail(RR_EINVAL, "null env");
    const int N = e->P.N, ni = e->RM.ni;
    float l4[4];
    default_light(l4);
    const bool own = !e->colour_host.empty();
    for (int i = 0; i < N; i++) {
        if (colours_out) memcpy(colours_out + (size_t)i * ni * 3, own ? e->colour_host.data() + (size_t)i * MAXINST * 3 : &e->RM.in_color[0][0], sizeof(float) * ni * 3);
        if (light_dirs_out) memcpy(light_dirs_out + 3 * (size_t)i, own ? e->light_host.data() + (size_t)i * 4 : l4, sizeof(float) * 3);
    }
    return RR_OK;
}

int rr_render_instances(rr_env *e, int32_t *n_inst, int32_t *owner_out) {
    if (!e || !n_inst) return fail(RR_EINVAL, "null argument");
    const RenderModel &RM = e->RM;
    *n_inst = RM.ni;
    if (owner_out)
        for (int i = 0; i < RM.ni; i++) {
            owner_out[4 * i] = RM.in_otype[i]; owner_out[4 * i + 1] = RM.in_oidx[i]; owner_out[4 * i + 2] = RM.in_uid[i]; owner_out[4 * i + 3] = RM.in_tex[i];
        }
    return RR_OK;
}

// ---- goals and episodes on the device (rr_episode.inc) ------------------------------------------------------------------------
static inline size_t image_bytes(const rr_env *e) { return (size_t)e->RM.W * e->RM.H * 3; }
static inline dim3 ep_grid(const rr_env *e) { return dim3((e->P.N + 255) / 256); }

// RR_EP_GOAL_RGB of the envs whose "goal changed" byte the last k_episode / k_env_goals launch set
static void launch_goal_image(rr_env *e) {
    if (!e->ep_goal_rgb) return;
    const size_t B = image_bytes(e);
    const int N = e->P.N, G = e->goals_rgb ? e->goals.G : 0;
    if (B % 16 == 0) {
        const unsigned units = (unsigned)(B / 16), chunks = (units + GI_CHUNK - 1) / GI_CHUNK;
        hipLaunchKernelGGL(k_goal_image<uint4>, dim3((unsigned)N * chunks), dim3(GI_THREADS), 0, e->stream, N, G, units, chunks, e->ep.goal_index, e->ep.changed,
                           (const uint4 *)e->goals_rgb, (uint4 *)e->ep_goal_rgb);
    } else {
        const unsigned units = (unsigned)(B / 4), chunks = (units + GI_CHUNK - 1) / GI_CHUNK;
        hipLaunchKernelGGL(k_goal_image<unsigned>, dim3((unsigned)N * chunks), dim3(GI_THREADS), 0, e->stream, N, G, units, chunks, e->ep.goal_index, e->ep.changed,
                           (const unsigned *)e->goals_rgb, (unsigned *)e->ep_goal_rgb);
    }
}

// every env of the mask (nullptr: all) to the goal index_dev[env] (nullptr: no goal), on the library's stream
static void launch_env_goals(rr_env *e, const int *index_dev, const unsigned char *mask_dev) {
    hipLaunchKernelGGL(k_env_goals, ep_grid(e), dim3(256), 0, e->stream, e->P, e->D, e->goals, e->ep, index_dev, mask_dev);
    launch_goal_image(e);
}

// The episode record: allocated on first use, zero-filled, every env without a goal (index -1, RR_EP_GOAL_POS all NaN).
static int ensure_episode(rr_env *e) {
    if (e->ep.score) return RR_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    const size_t N = e->P.N, nobj = e->P.nobj;
    static_assert(RR_EP_GOAL_RGB == RR_EP_COUNT - 1, "the image buffer is the last one and not part of the record");
    size_t *b = e->ep_bytes;
    b[RR_EP_SCORE] = b[RR_EP_REWARD] = b[RR_EP_DONE] = b[RR_EP_GOAL_INDEX] = b[RR_EP_EPISODE] = N * 4;
    b[RR_EP_FINAL_OBS] = N * (13 + 7 * nobj + 1) * 4;
    b[RR_EP_GOAL_POS] = N * nobj * 12;
    b[RR_EP_GOAL_RGB] = N * image_bytes(e);
    EpisodeRec &E = e->ep;
    RRCHK(mem_get(e, {mem_part(&E.score, b[RR_EP_SCORE]), mem_part(&E.reward, b[RR_EP_REWARD]), mem_part(&E.done, b[RR_EP_DONE]),
                      mem_part(&E.goal_index, b[RR_EP_GOAL_INDEX]), mem_part(&E.episode, b[RR_EP_EPISODE]),
                      mem_part(&E.final_obs, b[RR_EP_FINAL_OBS]), mem_part(&E.goal_pos, b[RR_EP_GOAL_POS]),
                      mem_part(&E.prev, N * 4), mem_part(&e->ep_index_stage, N * 4), mem_part(&E.changed, N * 4)},      // previous score, index staging, "goal changed" bytes
                  "rr_episode: allocating the episode record"));
    launch_env_goals(e, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_set_goals(rr_env *e, int32_t n_goals, const float *start_poses, const float *final_pos, const uint8_t *flags, const uint8_t *goal_rgb) {
    if (!e || n_goals < 0 || (n_goals > 0 && (!start_poses || !final_pos || !flags))) return fail(RR_EINVAL, "rr_set_goals: bad argument");
    const size_t G = (size_t)n_goals, nobj = e->P.nobj, B = image_bytes(e);
    for (size_t g = 0; g < G; g++)
        for (size_t i = 0; i < nobj; i++) {
            const unsigned f = flags[g * nobj + i];
            bool ok = true;
            if (f & 1u) for (int k = 0; k < 3; k++) ok = ok && std::isfinite(final_pos[(g * nobj + i) * 3 + k]);
            if (f & 2u) for (int k = 0; k < 7; k++) ok = ok && std::isfinite(start_poses[(g * nobj + i) * 7 + k]);
            if (!ok) return fail(RR_EINVAL, "rr_set_goals: goal " + std::to_string(g) + ", object " + std::to_string(i) + ": a value that is read is not finite");
        }
    int rc = ensure_episode(e);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    const bool images = G > 0 && goal_rgb != nullptr;
    // everything the new table needs is allocated before anything of the old one is given up
    GoalTable T = {};
    unsigned char *rgb = nullptr, *env_rgb = nullptr;
    MemPart parts[5];
    size_t np = 0;
    if (G > 0) { parts[np++] = mem_part(&T.start, G * nobj * 28, false); parts[np++] = mem_part(&T.final_pos, G * nobj * 12, false); parts[np++] = mem_part(&T.flags, G * nobj, false); }
    if (images) parts[np++] = mem_part(&rgb, G * B, false);
    if (images && !e->ep_goal_rgb) parts[np++] = mem_part(&env_rgb, (size_t)e->P.N * B);
    const char *err = e->mem.acquire(parts, np);
    if (err) return fail(RR_EDEVICE, std::string("rr_set_goals: allocating the goal table: ") + err);
    T.G = (int)G;
    hipError_t hrc = hipSuccess;
    if (G > 0) {
        hrc = hipMemcpyAsync((void *)T.start, start_poses, G * nobj * 28, hipMemcpyHostToDevice, e->stream);
        if (hrc == hipSuccess) hrc = hipMemcpyAsync((void *)T.final_pos, final_pos, G * nobj * 12, hipMemcpyHostToDevice, e->stream);
        if (hrc == hipSuccess) hrc = hipMemcpyAsync((void *)T.flags, flags, G * nobj, hipMemcpyHostToDevice, e->stream);
        if (hrc == hipSuccess && images) hrc = hipMemcpyAsync(rgb, goal_rgb, G * B, hipMemcpyHostToDevice, e->stream);
    }
    // (the wait also ends every queued kernel that reads the old table)
    if (hrc == hipSuccess) hrc = hipStreamSynchronize(e->stream);
    if (hrc != hipSuccess) {
        (void)hipStreamSynchronize(e->stream);
        e->mem.release(T.start); e->mem.release(T.final_pos); e->mem.release(T.flags); e->mem.release(rgb); e->mem.release(env_rgb);
        (void)hipGetLastError();
        return fail(RR_EDEVICE, std::string("rr_set_goals: uploading the goal table: ") + hipGetErrorString(hrc));
    }
    e->mem.release(e->goals.start); e->mem.release(e->goals.final_pos); e->mem.release(e->goals.flags); e->mem.release(e->goals_rgb);
    e->goals = T; e->goals_rgb = rgb;
    if (env_rgb) e->ep_goal_rgb = env_rgb;
    else if (!images) e->mem.release(e->ep_goal_rgb);
    // indices into the old table mean nothing in the new one: every env is without a goal until rr_set_env_goals
    launch_env_goals(e, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_set_env_goals(rr_env *e, const int32_t *goal_index, const uint8_t *env_mask_host) {
    if (!e || !goal_index) return fail(RR_EINVAL, "null argument");
    const int N = e->P.N;
    for (int i = 0; i < N; i++)
        if ((!env_mask_host || env_mask_host[i]) && (goal_index[i] < -1 || goal_index[i] >= e->goals.G))
            return fail(RR_EINVAL, "rr_set_env_goals: env " + std::to_string(i) + ": goal index " + std::to_string(goal_index[i]) + " is not -1 or in [0, " + std::to_string(e->goals.G) + ")");
    const int rc = ensure_episode(e);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(e->ep_index_stage, goal_index, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    const unsigned char *m = nullptr;
    if (env_mask_host) { HIPCHK(hipMemcpyAsync(e->mask_dev, env_mask_host, N, hipMemcpyHostToDevice, e->stream)); m = e->mask_dev; }
    launch_env_goals(e, e->ep_index_stage, m);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));   // the arguments are host memory
    return RR_OK;
}

int rr_set_episode(rr_env *e, int32_t horizon, int32_t goal_stride) {
    if (!e) return fail(RR_EINVAL, "null env");
    e->ep_horizon = horizon; e->ep_stride = goal_stride;
    return RR_OK;
}

int rr_episode_update(rr_env *e, int32_t reset_done) {
    if (!e) return fail(RR_EINVAL, "null env");
    const int rc = ensure_episode(e);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(e->cfg.device));
    const int G = e->goals.G;
    const int stride = G > 0 ? (int)((((long long)e->ep_stride % G) + G) % G) : 0;
    hipLaunchKernelGGL(k_episode, ep_grid(e), dim3(256), 0, e->stream, e->P, e->D, e->goals, e->ep, e->ep_horizon, stride, reset_done ? 1 : 0);
    if (reset_done) {
        launch_goal_image(e);
        e->la_valid = false;      // the device may have reset envs the look-ahead prepared for (as rr_reset)
        launch_obs(e);
    }
    HIPCHK(hipGetLastError());
    return RR_OK;
}

static int episode_field(rr_env *e, int32_t which, void **ptr, const char *who) {
    if (!e || which < 0 || which >= RR_EP_COUNT) return fail(RR_EINVAL, std::string(who) + ": bad buffer");
    const int rc = ensure_episode(e);
    if (rc != RR_OK) return rc;
    if (which == RR_EP_GOAL_RGB && !e->ep_goal_rgb) return fail(RR_EINVAL, std::string(who) + ": RR_EP_GOAL_RGB exists only while the goal table has images");
    void *const p[RR_EP_COUNT] = {e->ep.score, e->ep.reward, e->ep.done, e->ep.goal_index, e->ep.episode, e->ep.final_obs, e->ep.goal_pos, e->ep_goal_rgb};
    *ptr = p[which];
    return RR_OK;
}

int rr_episode_buffer(rr_env *e, int32_t which, void **dev_ptr, size_t *bytes) {
    void *p = nullptr;
    const int rc = episode_field(e, which, &p, "rr_episode_buffer");
    if (rc != RR_OK) return rc;
    if (dev_ptr) *dev_ptr = p;
    if (bytes) *bytes = e->ep_bytes[which];
    return RR_OK;
}

int rr_episode_copy_to_host(rr_env *e, int32_t which, void *dst, size_t bytes) {
    if (!dst) return fail(RR_EINVAL, "rr_episode_copy_to_host: null destination");
    void *p = nullptr;
    const int rc = episode_field(e, which, &p, "rr_episode_copy_to_host");
    if (rc != RR_OK) return rc;
    if (bytes != e->ep_bytes[which]) return fail(RR_EINVAL, "rr_episode_copy_to_host: size mismatch");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return RR_OK;
}

int rr_set_timing(rr_env *e, int32_t enable) {
    if (!e) return fail(RR_EINVAL, "null env");
    e->timing = enable != 0;
    memset(e->t_ms, 0, sizeof e->t_ms); memset(e->t_n, 0, sizeof e->t_n);
    return RR_OK;
}

int rr_get_timing(rr_env *e, float *ms_out, int32_t *launches_out) {
    if (!e || !ms_out || !launches_out) return fail(RR_EINVAL, "null argument");
    for (int i = 0; i < RR_NUM_KERNELS; i++) { ms_out[i] = e->t_ms[i]; launches_out[i] = e->t_n[i]; e->t_ms[i] = 0; e->t_n[i] = 0; }
    return RR_OK;
}

}  // extern "C"

