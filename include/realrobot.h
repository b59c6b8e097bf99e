/* realrobot.h -- C ABI of librealrobot_hip.so: batched REALRobot env.step() on MI355X (gfx950).
 *
 * Drop-in boundary.  The reference has no FFI for this path: its boundary is the duck-typed gym API
 * `gym.make(id) -> REALRobotEnv` with reset()/step()/render() (real_robots/__init__.py:22-28,
 * real_robots/envs/env.py:206-219,326-356) and, underneath, ~50 pybullet C-API calls per step
 * (SURVEY.md 3.3).  This header is what a maintainer binds instead of `import pybullet` for the step path;
 * every entry point cites the reference call(s) it replaces.  The ctypes binding is
 * real_robots_amd/_native.py; INTEGRATION.md shows the stub to add to the reference.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on success or a
 * negative RR_E* code and never throws/aborts; rr_last_error() gives the message of the last failure on the
 * calling thread.  The library owns all device memory; the caller owns host buffers.  One rr_env may be
 * used from one thread at a time.  Work is enqueued on the stream given at creation (or rr_set_stream) and
 * is asynchronous until rr_sync / rr_copy_to_host.
 * Layouts: every buffer is row-major with the env index outermost ([N, ...]).
 */
#ifndef REALROBOT_H
#define REALROBOT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 7   /* 3: RR_F_CONTACT_COUNT, RR_F_ENV_CLASS, rr_checkpoint_*, rr_evaluate_goals; 4: rr_map_observations, rr_map_images,
                              rr_sync_observations, rr_device_microbench; checkpoint blobs carry the step parameters (version 2 header);
                              5: rr_select_image_mirror; 6: rr_config carries the motor / solver constants the reference leaves to
                              pybullet's defaults (motor_kp .. solver_flags, in the place of reserved[7]: same struct size); checkpoint
                              header version 3 carries them too; RR_F_PREP; rr_pack_image_delta, rr_apply_image_delta;
                              7: rr_set_object_dynamics, rr_get_object_dynamics (per-env mass, inertia and contact materials of the
                              objects); checkpoint header version 4 carries them; rr_set_env_cameras, rr_set_env_appearance; rr_set_env_actuators,
                              rr_get_env_actuators (per-env motor gains, motor force and joint damping; checkpoint header version 5 carries them); rr_contact_observations;
                              rr_set_goals, rr_set_env_goals, rr_set_episode, rr_episode_update, rr_episode_buffer (goal table and episode
                              record on the device; checkpoints do not carry them); rr_snapshot_slots, rr_copy_envs (env forks and
                              snapshot slots on the device); rr_set_kinematic_points, rr_get_kinematic_points, rr_kinematic_observations,
                              rr_kinematic_buffer, rr_kinematic_copy_to_host (link states and Jacobians of the whole batch); rr_write_state,
                              rr_read_state (masked state writes by column groups -- resets, teleports, postures, velocity kicks -- and state
                              reads on the device); rr_set_rays, rr_get_rays, rr_ray_cast, rr_ray_buffer, rr_ray_copy_to_host (segments of
                              the whole batch against the collision hulls); rr_set_distance_pairs, rr_get_distance_pairs, rr_closest_points,
                              rr_distance_buffer, rr_distance_copy_to_host (distance and closest points of pairs of collision hulls);
                              rr_posture_clearance, rr_posture_buffer, rr_posture_copy_to_host (clearance of the pair table at candidate
                              joint postures, the nearest pair reduced on the device); rr_signed_distance, rr_signed_buffer,
                              rr_signed_copy_to_host (signed distance of the pair table: penetration depth, direction and witness points
                              where hulls overlap, at the present state or at candidate postures); rr_signed_gradient,
                              rr_signed_gradient_buffer, rr_signed_gradient_copy_to_host (that query plus the joint gradients of the
                              deepest pair's signed distance and of a hinge collision cost, reduced on the device);
                              rr_swept_clearance, rr_sweep_reach, rr_sweep_buffer, rr_sweep_copy_to_host (first contact of the pair
                              table along joint-space segments, by conservative advancement); rr_set_attachments,
                              rr_get_attachments (objects attached to robot links in the posture queries); rr_carried_sweep (the
                              swept clearance with those objects moving) */

enum {
    RR_OK = 0,
    RR_EINVAL = -1,     /* bad argument */
    RR_EDEVICE = -2,    /* HIP runtime error (no GPU, out of memory, launch failure).  Memory that a call allocates on first use
                           (contact and kinematic observations, ray casts, closest points, posture clearance, goal scores, plans and IK, per-env cameras and appearance, goal table and episode
                           record, snapshot slots and fork staging, mapped host blocks, the staging ring) is allocated all or nothing:
                           when that fails the call returns RR_EDEVICE, nothing has changed -- what the call would replace is kept --
                           and the handle stays usable; a later call tries again. */
    RR_EMODEL = -3,     /* malformed model blob */
    RR_EACTION = -4     /* non-finite action (the reference asserts, robot.py:189) */
};

/* fields of rr_get_buffer / rr_copy_to_host */
enum {
    RR_F_JOINTS = 0,    /* f32 [N, 9]        Kuka.calc_state()            robot.py:203-211 */
    RR_F_TOUCH = 1,     /* f32 [N, 4]        Kuka.get_touch_sensors()     robot.py:152-163 */
    RR_F_OBJ_POSE = 2,  /* f32 [N, n_obj, 7] object_bodies[..].get_pose() env.py:236-244 (xyz + xyzw quat) */
    RR_F_RGB = 3,       /* u8  [N, H, W, 3]  retina                       env.py:249-255,560-562 */
    RR_F_DEPTH = 4,     /* f32 [N, H, W]     GL depth in [0,1]            env.py:564-565 */
    RR_F_MASK = 5,      /* i32 [N, H, W]     body unique id, -1 background  env.py:552-558 */
    RR_F_TIMESTEP = 6,  /* i32 [N]           env.timestep                 env.py:217,346 */
    RR_F_ERRFLAGS = 7,  /* u32 [N]           1: non-finite state detected (env frozen until reset / set_state); 2: this step's command was
                                             not finite (env not stepped, robot.py:189: its state, clock and observations stay as they
                                             are; its contact list is dropped -- RR_F_CONTACT_COUNT 0, rr_get_contacts empty -- and the
                                             next accepted step starts its contact solve cold, like a step after rr_set_state);
                                             4: internal consistency of the solver (never expected; the env stops stepping until reset / set_state);
                                             8: RENDER status only -- more than 2048 near-plane-crossing triangles met one raster tile of the last
                                             rendered frame and the surplus was dropped (a camera inside a mesh); the physics ignores this bit,
                                             it stays set until rr_reset / rr_set_state of the env */
    RR_F_STATE = 8,     /* f32 [N, 61]       q[11] qd[11] 3x(pos3 quat4 lin3 ang3)  (checkpoint / parity) */
    RR_F_FRAG_COUNT = 9,/* u32 [N, tiles]    diagnostic: entries of k_shade's work list in the last render (pixels won by moving geometry + pixels vacated since the frame before) */
    RR_F_CONTACT_COUNT = 10, /* i32 [N]      contacts of the last solved step (rr_get_contacts returns them one env at a time); 0 after
                                             rr_reset / rr_set_state of that env */
    RR_F_ENV_CLASS = 11,     /* i32 [N]      diagnostic: 0 light, 1 heavy, 2 very heavy -- which launch solved / rendered the env in the last
                                             step.  Both fields live in fixed buffers written by the solve kernels: a pointer
                                             from rr_get_buffer stays valid over steps like every other field's */
    RR_F_PREP = 12,          /* f32 [N, 378]  diagnostic: the preparation's record of every env, as the last preparation launch left it -- frames of the
                                             eleven bodies (R 99, position 33, joint axis 33), M^-1 (121), unconstrained joint velocities (11), the objects'
                                             rotation / world inverse inertia / unconstrained velocities / collision position (27 + 27 + 9 + 9 + 9); after a
                                             step with the look-ahead it describes the state the step LEFT (tests compare the kernel's forms through it) */
    RR_F_CONTACTS = 13,      /* f32 [N, 48, 12]  the three fields of rr_contact_observations (additive in ABI 7), which see: as its LAST CALL */
    RR_F_BODY_FORCE = 14,    /* f32 [N, RR_CONTACT_ROWS, 2]   left them -- steps do not refresh them; allocated on first use, all zero */
    RR_F_BODY_PARTNERS = 15, /* u32 [N, RR_CONTACT_ROWS]      before the first call */
    RR_F_COUNT = 16
};
#define RR_CONTACT_ROWS 20   /* body rows of RR_F_BODY_FORCE / RR_F_BODY_PARTNERS: the 17 URDF links, then objects 0..2 */

/* rr_config.flags */
#define RR_FLAG_NO_MASK 1   /* R2 environments have no `mask` observation (robot.py:99-112): do not produce RR_F_MASK */

typedef struct rr_config {
    int32_t abi_version;    /* RR_ABI_VERSION */
    int32_t num_envs;       /* N envs on this device */
    int32_t n_objects;      /* 1..3: cube, tomato, mustard      robot.py:49-50 */
    int32_t width, height;  /* eye camera; reference default 320x240 (robot.py:30-31).  width: a multiple of 4 in [4, 1024], height in
                               [1, 1024], at most 255 raster tiles of 4096 pixels (1024 x 960 fits, 1024 x 961 does not): RR_EINVAL otherwise */
    int32_t device;         /* HIP device ordinal */
    int32_t solver_iters;   /* PGS iterations; <=0 -> 50        SURVEY A.1.2 */
    int32_t envs_per_block; /* accepted and ignored: no launch shape depends on it (the field stays for the ABI); pass 0 */
    float dt;               /* <=0 -> 0.005                     env.py:203-204 */
    float erp;              /* <=0 -> 0.2 */
    float margin;           /* <=0 -> 0.02 */
    int32_t use_urdf_inertia; /* 0: Bullet AABB inertia for robot links (default); 1: URDF <inertia> */
    int32_t flags;          /* RR_FLAG_* */
    /* The constants below are NOT in the reference tree: robot.py:196-201 calls Joint.set_position -> setJointMotorControl2(
     * POSITION_CONTROL, targetPosition) and leaves positionGain / velocityGain / force to pybullet's defaults, env.py:202-204 leaves
     * the solver to Bullet's (unverifiable here).  They are parameters of the handle, reach every
     * kernel as scalar arguments and are part of a checkpoint's header; 0 selects the documented default, a NEGATIVE value a
     * literal zero (gain off / cold start / no damping).  The reference's own tracking script (tests/test_actions.py:62-71,
     * 147-152) is met at every check point by motor_kp >= 0.5 and not by 0.1 (tests/golden/macro_sensitivity.json). */
    float motor_kp;         /* 0 -> 0.1      positionGain: v_target = kp (target - q) / dt + (1 - kd) qd */
    float motor_kd;         /* 0 -> 1.0      velocityGain */
    float motor_max_force;  /* 0 -> 100000   |motor impulse| <= force dt */
    float warmstart;        /* 0 -> 0.85     Bullet's m_warmstartingFactor on the matched normal impulses; < 0: cold start every step */
    float lin_damping;      /* 0 -> 0.04     btMultiBody base damping of the free objects; < 0: none */
    float ang_damping;      /* 0 -> 0.04 */
    int32_t solver_flags;   /* RR_SOLVER_* */
} rr_config;
#define RR_SOLVER_NO_RATE_LIMIT 1   /* limitActionByJoint (env.py:314-321) is skipped: the clipped command itself is the motor target */
#define RR_SOLVER_IK_SINGLE_SEED 2  /* rr_ik / rr_plan_macro: ONE damped-least-squares solve per target, seeded with the env's current joints --
                                       the literal call pattern of the reference (env.py:372-375, 421-427: one calculateInverseKinematics per
                                       way point, no stepping in between).  Default (0): the best of several seeds -- current joints, an
                                       elbow-up posture, the previous way point -- by convergence, then elbow height / continuity: which branch
                                       pybullet's own solver lands on from one seed is not specified by the reference */

typedef struct rr_env rr_env;

/* Replaces REALRobotEnv.__init__ + the lazy bullet client/world creation in reset()
 * (env.py:36-122,202-219; robot.py:44-118,165-185: loadURDF of robot + table + objects).
 * `model_blob` is the compiled model (tools/compile_model.py). `stream` is a hipStream_t or NULL (default stream). */
int rr_create(const rr_config *cfg, const void *model_blob, size_t blob_bytes, void *stream, rr_env **out);
int rr_destroy(rr_env *env);
int rr_set_stream(rr_env *env, void *stream);

/* Replaces env.reset() (env.py:206-219; robot.py:120-129,165-185) for the envs whose mask byte is non-zero
 * (env_mask == NULL: all envs). Device-side state copy from the template; does not render. */
int rr_reset(rr_env *env, const uint8_t *env_mask_host);

/* Replaces BodyPart.reset_pose via robot.object_bodies[name].reset_pose (env.py:159-162; zeroes velocity). */
int rr_set_object_pose(rr_env *env, int32_t env_index, int32_t obj, const float *pose7);
/* Batched rr_set_object_pose: poses f32 [N, n_obj, 7] (host) for the envs whose mask byte is non-zero (NULL: all envs).
 * Replaces the per-object loop of REALRobotEnv.set_goal (env.py:159-162) for a whole batch with one upload. */
int rr_set_object_poses(rr_env *env, const float *poses_host, const uint8_t *env_mask_host);
/* The pose (xyz + xyzw quaternion, host) object `obj` of env `env_index` (< 0: every env) returns to on rr_reset and when the
 * out-of-bounds rule fires (env.py:257-264). Replaces in-place edits of Kuka.object_poses (robot.py:19-24; the reference's
 * tests/test_actions.py:95-98 parks the objects on the shelf that way). Defaults: the poses of the model blob. */
int rr_set_object_home(rr_env *env, int32_t env_index, int32_t obj, const float *pose7);

/* Per-env dynamics of the free objects: f32 [N, n_obj, 8] host, one row per (env, object) =
 *   {mass, ixx, iyy, izz (principal inertia, object frame), lateral friction, restitution, rolling friction, spinning friction}.
 * Replaces pybullet.changeDynamics(uid, -1, mass=, localInertiaDiagonal=, lateralFriction=, restitution=, rollingFriction=,
 * spinningFriction=) of an object for the envs whose mask byte is non-zero (NULL: all envs; the rows of the other envs are not read).
 * Mass and inertias must be finite and > 0, the four materials finite and >= 0: on any violation the call returns RR_EINVAL and
 * changes no env.  Defaults: the values of the model blob.  The values are part of the env, not of its state: they outlive rr_reset,
 * rr_set_state and rr_set_object_pose(s), and checkpoints carry them.  An object's materials apply to all of its collision shapes; a
 * contact between two shapes gets the materials combined by Bullet's rule (products of friction and restitution, r_a mu_b + r_b mu_a
 * at most 10 for rolling / spinning -- rr_get_contacts shows the combined friction); the table and the robot keep the blob's values.
 * Synchronous (the source is host memory). */
int rr_set_object_dynamics(rr_env *env, const float *dyn_host, const uint8_t *env_mask_host);
/* Replaces pybullet.getDynamicsInfo(uid, -1) of the objects: every env's rows, same layout, f32 [N, n_obj, 8] host. */
int rr_get_object_dynamics(rr_env *env, float *dyn_out_host);

/* Per-env actuators (additive in ABI 7): f32 [N][11][4] host, one row per (env, movable joint) in the order of q[11] of RR_F_STATE (the
 * seven arm joints, then the four finger joints) =
 *   {kp (positionGain), kd (velocityGain), max_force, joint damping}.
 * Replaces pybullet.setJointMotorControl2(POSITION_CONTROL, positionGain=, velocityGain=, force=) and changeDynamics(jointDamping=) of
 * a joint for the envs whose mask byte is non-zero (NULL: all envs; the rows of the other envs are not read).  For that env and joint
 * the row takes the place of the handle's motor_kp, motor_kd, motor_max_force (rr_config) and of the model blob's body_damping in
 *   v_target = kp (target - q) / dt + (1 - kd) qd,   |motor impulse| <= max_force dt,   rhs = -bias - damping qd.
 * act_host == NULL: the masked envs return to the handle's values.  All four values must be finite and >= 0 (max_force dt finite too);
 * 0 is a LITERAL zero here (gain off, motor off, no damping) -- unlike rr_config, where 0 selects the default.  On any violation the
 * call returns RR_EINVAL, the message names the env and the joint, and no env changes.  Defaults on a fresh handle: the handle's
 * motor_kp, motor_kd, motor_max_force in every row and the blob's body_damping.  The values are part of the env, not of its state:
 * they outlive rr_reset, rr_set_state and rr_set_object_pose(s), and checkpoints carry them (a continuation is only bit for bit with
 * the same actuators; a restore puts the checkpoint's table in force; the handle's scalars are still compared).  The next step
 * prepares itself again (the look-ahead ran with the old damping).  Neither rr_ik nor rr_plan_macro depend on the table.
 * Ranges are the caller's responsibility: a velocity gain below 1, or large position gains without the rate limit, can diverge under
 * full-range commands (in the float64 oracle as on the device); RR_F_ERRFLAGS tells.  Synchronous (the source is host memory).
 * Out of scope: per-env rate limits and joint ranges (act_maxdiff, act_min / act_max, body_limits), per-env link masses / inertias
 * of the robot (M^-1 is per env already, the body table of the preparation is not), per-env erp / warm start / object damping,
 * action latency.  The handle's motor constants (rr_config) keep working exactly as they do. */
int rr_set_env_actuators(rr_env *env, const float *act_host, const uint8_t *env_mask_host);
/* What is in force for every env, same layout, f32 [N][11][4] host. */
int rr_get_env_actuators(rr_env *env, float *act_out_host);

/* Replaces one REALRobotEnv.step_joints() (env.py:326-356) for all N envs:
 *   limitActionByJoint (env.py:314-321), control_objects_limits (env.py:257-264), Kuka.apply_action
 *   (robot.py:188-201), scene.global_step() -> stepSimulation (env.py:340), calc_state/get_touch_sensors
 *   (robot.py:203-211,152-163) and, when render_mode != 0, get_retina (env.py:249-255).
 * joint_cmd: f32 [N, 9] (device pointer if cmd_on_device, else host; NULL -> zeros as env.py:333-334).
 *   Host commands / flags are copied into a pinned staging ring before the call returns (the caller may reuse its
 *   buffer at once; the call does not wait for the device).
 *   STREAM CONTRACT for cmd_on_device: the buffer is read IN PLACE by the first kernel of the step, on the library's
 *   stream (rr_create / rr_set_stream).  The caller must (1) have produced it on that same stream, or have made that
 *   stream wait for the producer (event / synchronise), and (2) not overwrite it before the step has consumed it --
 *   i.e. not before later work on the same stream, or rr_sync.  The zero-copy views of rr_get_buffer carry no stream
 *   either: readers on another stream must order themselves after the step the same way.
 * render_mode: 0 none, 1 all envs, 2 per-env flags in render_flags_host (u8 [N]). */
int rr_step(rr_env *env, const float *joint_cmd, int32_t cmd_on_device, int32_t render_mode,
            const uint8_t *render_flags_host);

/* Replaces EyeCamera.render (env.py:536-567) for all envs at the current state (used by reset()/set_goal()). */
int rr_render(rr_env *env);

/* Replaces the camera of this env handle (row-major 4x4 OpenGL view and projection matrices, host). The default is the
 * reference's eye camera; the facade uses a second env handle with EnvCamera's matrices for render('rgb_array')
 * (computeViewMatrixFromYawPitchRoll / computeProjectionMatrixFOV, env.py:480-499).  Both pointers NULL: back to the default
 * eye camera (eye (0.01, 0, 1.2) -> table position, up (0, 0, 1), fov 80, near 0.1, far 100; env.py:136-141, 253-255, 548-551).
 * Does not render: every env keeps its last frame until it is rendered again, and that frame is the first one of the new camera. */
int rr_set_camera(rr_env *env, const float *view16, const float *proj16);
/* Per-env cameras (additive in ABI 7): the envs whose mask byte is non-zero (NULL: all) get their own row-major 4x4 OpenGL view and
 * projection (views16 / projs16: f32 [N][16] host, rows of unmasked envs not read) -- the conventions and limits of rr_set_camera:
 * any view, a perspective projection whose near plane is 0.1 (geometry nearer than w = 0.1 is clipped).  A null or non-finite
 * matrix of a masked env returns RR_EINVAL and changes no env.  The envs outside the mask are not touched (camera, image, fragment
 * lists).  Does not render: a masked env keeps its last frame until its own next render, the first frame of its new camera.
 * The first call allocates a static layer per env (19 bytes per pixel per env: 1.27 GB at 4096 envs of 128 x 128); rr_set_camera
 * returns the handle to one camera for all envs.  Cameras are settings of the handle, not env state: rr_reset, rr_set_state,
 * rr_set_object_pose(s) and rr_checkpoint_restore keep them, checkpoints do not carry them.  Synchronous. */
int rr_set_env_cameras(rr_env *env, const float *views16, const float *projs16, const uint8_t *env_mask_host);
/* Per-env appearance (additive in ABI 7; pybullet's changeVisualShape(rgbaColor=...) and getCameraImage(lightDirection=...)):
 * the envs whose mask byte is non-zero (NULL: all) get their own colour for every render instance and / or their own light
 * direction.  colours: f32 [N][n_inst][3] host or NULL (keep); light_dirs: f32 [N][3] host or NULL (keep); rows of unmasked envs
 * are not read.  n_inst and what each instance belongs to: rr_render_instances.  A colour replaces the model's colour of that
 * instance for that env: the pixel stays floor(texel * colour * shade), clamped to 255.  A light direction replaces
 * l = (-50, 30, 100) / |.| in shade = 0.6 + 0.35 max(n.l, 0) + 0.05 max(r_z, 0)^2; it points from the scene towards the light and
 * is normalised in float32 on the host, once.  Colours of a masked env must be finite and >= 0, its light finite with a float32
 * norm that is finite and > 1e-6; otherwise RR_EINVAL (the message names the env) and no env changes.  All three pointers NULL:
 * back to the model's appearance for every env (a mask alone is RR_EINVAL).
 * Does not render: a masked env keeps its last frame until its own next render, which shows the whole env in its new appearance --
 * static instances and movable instances that did not move included.  The envs outside the mask are not touched.
 * Appearance needs an env's own static layer, as rr_set_env_cameras does: the same buffers (19 bytes per pixel per env), allocated
 * by whichever of the two calls comes first.  With an appearance in force rr_set_camera gives every env that one camera and keeps
 * the per-env layers; rr_set_env_appearance(env, NULL, NULL, NULL) with no per-env cameras in force returns to the shared layer.
 * A setting of the handle like the cameras: rr_reset, rr_set_state, rr_set_object_pose(s) and rr_checkpoint_restore keep it,
 * checkpoints do not carry it.  Synchronous.
 * Out of scope: the ambient / diffuse / specular coefficients (0.6, 0.35, 0.05 stay literals), a light colour of its own (a common
 * factor on the colours does it), the background colour, per-env textures, transparency (there is no alpha). */
int rr_set_env_appearance(rr_env *env, const float *colours, const float *light_dirs, const uint8_t *env_mask_host);
/* What is in force: colours_out f32 [N][n_inst][3], light_dirs_out f32 [N][3] (unit vectors), either may be NULL.  On a fresh handle:
 * the model's instance colours and the default light. */
int rr_get_env_appearance(rr_env *env, float *colours_out, float *light_dirs_out);
/* The render instances of the model: *n_inst of them; owner_out (i32 [n_inst][4] or NULL) gets {owner type 0 static / 1 robot body /
 * 2 object, index of that body or object, uid (the value in RR_F_MASK), texture index or -1} of each.  The trailing instances of
 * the objects that a handle with n_objects < 3 does not draw have a row too (their colours are stored, never read). */
int rr_render_instances(rr_env *env, int32_t *n_inst, int32_t *owner_out);

/* Device pointer + size of an observation/state buffer (valid until rr_destroy). */
int rr_get_buffer(rr_env *env, int32_t field, void **dev_ptr, size_t *bytes);
/* The buffers are owned by the library and READ-ONLY for the caller: observations are rewritten by every step, and the
 * image buffers (RGB, DEPTH, MASK) persist from frame to frame -- a render only rewrites the pixels that differ from the
 * previous frame of that env, so a caller that scribbles into them would see its marks survive. */
/* Synchronising copy of a whole field to host memory. */
int rr_copy_to_host(rr_env *env, int32_t field, void *dst, size_t bytes);
/* Overwrites the simulation state from host memory (f32 [N, 61]); parity tests, goal set-up.  The contact history of the warm
 * start (the previous step's contact list, see rr_get_contacts) is not part of the 61 floats: the step after rr_set_state /
 * rr_reset starts cold, as after pybullet's resetSimulation.  To continue a run exactly, use rr_checkpoint_save / _restore.
 * (rr_set_object_pose(s) keeps the history, like resetBasePositionAndOrientation keeps Bullet's manifolds: cached points of a
 * teleported body are farther than the contact margin from its new contacts and match nothing.) */
int rr_set_state(rr_env *env, const float *state_host);
/* ---- State writes and reads on the device (additive in ABI 7) ------------------------------------------------------------------------
 * Replaces resetJointState, resetBasePositionAndOrientation and resetBaseVelocity of pybullet for ALL envs at once, with the tensor and
 * the mask in device memory if the caller wishes: a device program decides which envs restart and where they start -- a curriculum
 * over start poses, randomised postures, early termination on its own criterion, objects put where a sampled plan says -- with no
 * host round trip (the set_*_state_tensor_indexed of batched simulators).  rr_reset, rr_set_object_poses and rr_set_state take host
 * memory, and the last one has no mask.  A read-modify-write of the object twists (rr_read_state, arithmetic, RR_W_OBJ_VEL) is an
 * impulse, dv = J / m, applied between two steps.
 * state: f32 [N, 61], the rows of RR_F_STATE; env_mask: u8 [N], an env takes part when its byte is non-zero (a one-byte bool array
 * is a valid mask), NULL: all envs.  parts: which column groups of the row are written, and what happens around them: */
#define RR_W_JOINT_POS 1   /* columns 0..10 of the RR_F_STATE row: q[11] */
#define RR_W_JOINT_VEL 2   /* columns 11..21: qd[11] */
#define RR_W_OBJ_POSE  4   /* per object o < n_objects, columns 22+13o .. +6: pos3 quat4 */
#define RR_W_OBJ_VEL   8   /* per object, columns 22+13o+7 .. +12: lin3 ang3 */
#define RR_W_RESET     16  /* the env is first reset exactly as by rr_reset */
#define RR_W_FRESH     32  /* afterwards: error flags 0, touch 0, contact history dropped (what rr_set_state does behind its write) */
/* Order per masked env: (1) the reset, if RR_W_RESET is set; (2) the selected column groups are copied from the env's row of `state`;
 * (3) the fresh-start clean-up, if RR_W_FRESH is set.  Columns outside the selected groups, rows of unmasked envs and the columns of
 * objects >= n_objects are never used: a NaN there does not reach the state.
 * RR_W_OBJ_POSE without RR_W_OBJ_VEL zeroes the object's twist -- resetBasePositionAndOrientation, as rr_set_object_poses does --;
 * with both bits both come from the tensor; RR_W_OBJ_VEL alone leaves the pose in place: the velocity kick.
 * Without RR_W_RESET or RR_W_FRESH these are KEPT, as rr_set_object_poses keeps them: the contact history of the warm start,
 * RR_F_TIMESTEP, the error flags, the touch sensors and the motor-target rows of the state slab.  So an env frozen by error flag 1
 * stays frozen unless RR_W_FRESH (or RR_W_RESET) is given.
 * Equivalences, each bit for bit (tested):
 *   parts == RR_W_RESET (state may be NULL)                  rr_reset(mask)
 *   RR_W_OBJ_POSE                                            rr_set_object_poses(poses, mask), the poses in their columns of the rows
 *   15 | RR_W_FRESH with a NULL mask                         rr_set_state (on a handle with three objects: rr_set_state also writes the
 *                                                            columns of the objects the handle does not have)
 *   RR_W_RESET | RR_W_OBJ_POSE                               steps 2 and 4 of the auto-reset of rr_episode_update
 * on_device != 0: both pointers are device memory, read IN PLACE on the library's stream under the STREAM CONTRACT of rr_step's
 * cmd_on_device (produced on that stream or ordered before it; not overwritten before later work on that stream, or rr_sync); the
 * call allocates nothing, checks the launch and returns without waiting.  on_device == 0: both are host memory; the call stages them
 * and is synchronous, like rr_set_state.
 * Values are not validated, as in rr_set_state and rr_set_object_poses: a non-finite value is caught by the next step's guard (error
 * flag 1).  RR_EINVAL, with nothing changed: a null env; a bit outside the six; parts == 0; state == NULL while any of the four
 * column bits is set.
 * Like every change of state from outside, the next step prepares itself again; the observation buffers and a mapped host mirror
 * are refreshed behind the write; images are left alone (an env keeps its last frame until its next render).  The episode record,
 * macro plans in flight, settings and the fields of the observation calls are not touched: after a write into running envs the
 * caller re-bases the previous score with rr_set_env_goals, as after rr_reset.
 * Out of scope: writing the clock or the motor targets; per-env object sets; writes into snapshot slots (go through rr_copy_envs);
 * validation on the device; an indexed form (a list of env ids instead of a mask); options of the gym vector env, whose episode
 * clocks live on the host. */
int rr_write_state(rr_env *env, const float *state, const uint8_t *env_mask, uint32_t parts, int32_t on_device);
/* One launch on the library's stream gathers the PRESENT state of every env into the device buffer of RR_F_STATE (rr_get_buffer):
 * f32 [N, 61], the rows rr_copy_to_host(RR_F_STATE) returns.  The call checks the launch and returns without waiting; the buffer is
 * valid for readers ordered behind it (STREAM CONTRACT as for the other zero-copy views, rr_step) and holds what the last such call
 * -- or rr_copy_to_host(RR_F_STATE) -- computed: steps do not refresh it.  The same buffer is the STAGING AREA of rr_set_state,
 * rr_set_object_poses, rr_evaluate_goals and the host path of rr_write_state: those calls overwrite it.  (It may be passed to
 * rr_write_state with on_device != 0 as it is: that path reads in place and stages nothing.) */
int rr_read_state(rr_env *env);

/* Checkpoint = everything a restore needs to continue BIT FOR BIT where the save left off: the state (with the motor targets),
 * the contact history of the warm start (contact list + normal forces of the last solved step -- Bullet's persistent manifolds
 * with their cached impulses, which pybullet.saveState / restoreState carry too), episode clocks, error flags, touch sensors,
 * the per-env object home poses, the per-env object dynamics (rr_set_object_dynamics) and the per-env actuators (rr_set_env_actuators).  Opaque host blob of
 * rr_checkpoint_bytes() bytes, valid for env handles of the same num_envs / n_objects.  (Macro plans in flight are host-side policy state and not part of it.)  save + restore + step == step, tested. */
int rr_checkpoint_bytes(rr_env *env, size_t *bytes);
int rr_checkpoint_save(rr_env *env, void *dst_host, size_t bytes);
int rr_checkpoint_restore(rr_env *env, const void *src_host, size_t bytes);
int rr_sync(rr_env *env);

/* ---- Env forks and snapshot slots on the device (additive in ABI 7) ----------------------------------------------------------------
 * Replaces pybullet.saveState() / restoreState(stateId) -- the IN-MEMORY variant, which the host-side rr_checkpoint_* calls do not
 * cover -- and adds what a batched simulator needs for planning with itself as the model (MPPI / CEM rollouts, branching search):
 * "env j becomes an exact copy of env i", for any map, and a whole batch put aside and brought back, all without the host.
 * The RECORD of an env is what a checkpoint carries for it minus its settings:
 *   rows 0..71 of the state slab (the 61 floats of RR_F_STATE and the motor targets); the contact count of the last solved step; the
 *   live rows of that step's contact list and of its normal forces -- the rows below min(count, 48), the contact history of the warm
 *   start --; RR_F_TIMESTEP; RR_F_ERRFLAGS; the four RR_F_TOUCH values; the published count and class (RR_F_CONTACT_COUNT,
 *   RR_F_ENV_CLASS).
 * The rows of the list and of the forces from the count on are NOT copied and are unspecified in a destination: every reader of
 * the list (the collision pass's warm-start matching, the solve, rr_contact_observations, rr_get_contacts) stops at the count.
 * NOT part of a record, and left with the destination env: the object home poses, the object dynamics and pair materials
 * (rr_set_object_dynamics), the actuators (rr_set_env_actuators), the cameras and the appearance -- settings of the env, not its
 * state --; the episode record (RR_EP_*: a setting of the handle, as for restores -- after a copy into running envs the caller
 * re-bases the previous score with rr_set_env_goals); the fields of rr_contact_observations (they hold what its last call computed);
 * a macro plan in flight and its cursor (rr_plan_macro: policy state); the images and the renderer's fragment lists.  A fork
 * between envs with different settings is therefore not a continuation of the source: the copy steps with its own mass, gains,
 * home poses and camera. */
#define RR_SLOT_LIVE (-1)    /* the running envs, as a slot number of rr_copy_envs */
#define RR_MAX_SLOTS 64
/* n_slots snapshot slots, numbered 0 .. n_slots - 1, each a record for every env (2 820 bytes per env at full list capacity, every
 * array rounded up to 256 bytes: 11.6 MB per slot at 4096 envs).  n_slots in [0, RR_MAX_SLOTS], RR_EINVAL otherwise.  Every new slot
 * is filled with the present records of the running envs (on the library's stream), so no slot ever holds an unwritten record.
 * A later call REPLACES all slots -- their contents are lost --; n_slots == 0 frees them.  Does not wait for the device unless it gives up old slots. */
int rr_snapshot_slots(rr_env *env, int32_t n_slots);
/* For every env i, the record of env i in dst_slot becomes the record of env src_index[i] in src_slot; RR_SLOT_LIVE names the
 * running envs.  An index of -1 keeps env i as it is; src_index == NULL is the identity over all envs.  One call, four operations:
 *   (RR_SLOT_LIVE, RR_SLOT_LIVE, idx)  fork between running envs         (s, RR_SLOT_LIVE, NULL)  restore (restoreState)
 *   (RR_SLOT_LIVE, s, NULL or idx)     save (saveState)                  (s, RR_SLOT_LIVE, idx)   one saved env into many running ones
 * and slot to slot.  A slot number outside [-1, n_slots) returns RR_EINVAL.
 * src_index is i32 [N].  A HOST pointer (index_on_device == 0) is checked before anything is launched: an entry outside
 * {-1} u [0, N) returns RR_EINVAL, the message names the env, and nothing changes; the array is copied into the pinned staging ring
 * before the call returns (the caller may reuse it at once).  A DEVICE pointer (index_on_device != 0) is read in place on the
 * library's stream under the STREAM CONTRACT of rr_step's cmd_on_device (produced on that stream or ordered before it; not
 * overwritten before later work on that stream, or rr_sync); an entry out of range keeps that env as it is, like -1 (the kernel
 * checks the range before it forms an address).
 * With src_slot == dst_slot and an index -- running envs onto running envs included -- the copy behaves as if every source were
 * read before any destination is written: swaps, cycles, chains and a broadcast from an env that is itself overwritten come out
 * right.  Such a call goes through a hidden staging slot (two launches), allocated by the first one.  Different slots, or a NULL index: one launch.  (NULL with equal slots
 * copies every record onto itself: nothing is done.)
 * When dst_slot is RR_SLOT_LIVE the call is a change of state from outside, like rr_reset: the next step prepares itself again;
 * a destination env takes the source's error bits 1, 2 and 4 -- a frozen env forks frozen -- while bit 8 is CLEARED: that bit
 * describes the destination's own last rendered frame (rr_set_state clears it too); the observation buffers and a mapped host
 * mirror are refreshed behind the copy.  The images are left alone: an env keeps its last frame until its own next render, which
 * shows the new state.  The step that follows continues the SOURCE's run bit for bit (tested), given equal settings.
 * On the library's stream, behind the steps enqueued before it; the call checks the launch and returns without waiting.
 * Out of scope: copying settings, the episode record, macro plans or images (above); forks between two handles or two devices. */
int rr_copy_envs(rr_env *env, int32_t src_slot, int32_t dst_slot, const int32_t *src_index, int32_t index_on_device);
/* Host mirror of the low-dimensional observations, for callers that read them on the host after every step (the gym facade:
 * Kuka.calc_state + get_touch_sensors, robot.py:152-163, 203-211): a pinned, device-mapped host block
 *   { f32 joints [N][9] | f32 touch [N][4] | f32 object poses [N][n_obj][7] | i32 timestep [N] | u32 errflags [N] }
 * which, once mapped, the last launch of every rr_step / rr_reset / rr_set_state / rr_set_object_pose(s) / rr_checkpoint_restore
 * on the library's stream refreshes.  Valid to read after rr_sync (one wait per step instead of one synchronising copy per
 * field); owned by the library until rr_destroy.  Repeated calls return the same block. */
int rr_map_observations(rr_env *env, void **host_ptr, size_t *bytes);
/* The same for the images of a handful of envs (EyeCamera.render returns host arrays, env.py:536-567): pinned host copies of
 * RR_F_RGB / RR_F_DEPTH / RR_F_MASK (pass NULL for what is not wanted), refreshed by asynchronous copies behind every rr_step that
 * renders and every rr_render; valid to read after rr_sync.  At most 256 MiB per step in total. */
int rr_map_images(rr_env *env, void **rgb_host, void **depth_host, void **mask_host);
/* Which of the mapped image blocks a rendered step refreshes: a mask of 1 (RGB), 2 (depth), 4 (mask); default 7.  A caller that
 * asked for the mask once (get_observation_extended, env.py:291-312) and then goes back to plain observations (env.py:266-289)
 * deselects it instead of paying its copy after every step; a field selected again is brought up to date at once (valid after
 * rr_sync_observations).  The blocks stay mapped either way. */
int rr_select_image_mirror(rr_env *env, int32_t fields);
/* Waits until the mapped blocks (rr_map_observations / rr_map_images) hold the observations of the last step -- not for the rest of
 * the stream: with a handful of envs the state part of the NEXT step is queued behind the mirror and runs while the
 * caller computes its next action.  Without a mapping it is rr_sync. */
int rr_sync_observations(rr_env *env);

/* Delta records for the observation gather of a sharded batch (the reference has one env per process and no gather):
 * the pixels in which the last rendered frame of every env may differ from the one before are the entries of the renderer's
 * fragment lists (RR_F_FRAG_COUNT of them per (env, tile) item).  rr_pack_image_delta writes one 12-byte record per entry --
 * { env * H * W + row * W + col, r | g << 8 | b << 16, depth bits }, the pixel's NEW value -- at offsets_dev[item] + i, where
 * offsets_dev (u32 [N * tiles], device) is the exclusive prefix sum of RR_F_FRAG_COUNT made by the caller; records beyond
 * `capacity` are dropped.  On the library's stream.  After a frame that rewrote whole images (the first render of a handle,
 * the first render of an env after rr_set_camera) the lists do not describe the change: ship the slabs then.
 * rr_apply_image_delta is the receiving side, with no env handle: `world` blocks of `capacity` records of which the first
 * totals_dev[r] are valid, applied to persistent images of world * pixels_per_rank pixels (rank r's records address its block);
 * enqueued on `stream` (a hipStream_t or NULL) of the current device. */
int rr_pack_image_delta(rr_env *env, const uint32_t *offsets_dev, uint32_t *records_dev, uint32_t capacity);
int rr_apply_image_delta(const uint32_t *records_dev, const uint32_t *totals_dev, int32_t world, uint32_t capacity, size_t pixels_per_rank,
                         uint8_t *rgb_dev, float *depth_dev, void *stream);

/* Replaces robot.parts[name].get_position()/get_pose() (env.py:230-232): world pose of the COM frame of
 * every robot link, f32 [N, 17, 7] (URDF depth-first link order, see data/realrobot_model_links.txt). */
int rr_link_poses(rr_env *env, float *out_host);
/* Replaces Kuka.get_contacts (robot.py:131-150) for one env: up to max_contacts rows of 12 floats
 * {bodyA, bodyB, linkA, x,y,z, nx,ny,nz, distance, normal_force, mu}; *count receives the number written.  This list --
 * the contacts of the last step with the normal forces the solver found -- is also the contact history the next step's
 * warm start matches its contacts against (Bullet: persistent manifolds, m_warmstartingFactor 0.85). */
int rr_get_contacts(rr_env *env, int32_t env_index, float *out_host, int32_t max_contacts, int32_t *count);
/* Replaces Kuka.get_contacts (robot.py:131-150), with and without forces=True, for ALL envs at once and on the device (additive in
 * ABI 7): one launch on the library's stream turns the contact list of the last solved step -- the one rr_get_contacts shows -- into
 * three device fields (rr_get_buffer / rr_copy_to_host / DLPack).  The call checks the launch and returns without waiting.
 *   RR_F_CONTACTS       f32 [N, 48, 12]: row c < RR_F_CONTACT_COUNT[env] is exactly the row rr_get_contacts gives for that env and
 *                       contact, {bodyA, bodyB, linkA, x, y, z, nx, ny, nz, distance, normal_force, mu}; the rows from the count on
 *                       are all zero.
 *   RR_F_BODY_FORCE     f32 [N, RR_CONTACT_ROWS, 2]: {max, sum} of the normal force over the contacts of the row's body.
 *   RR_F_BODY_PARTNERS  u32 [N, RR_CONTACT_ROWS]: what the row's body touches -- bit 0 a static body (table or shelf, body -1),
 *                       bit 1 + j object j, bit 4 the robot.
 * Rows 0..16 are the robot's URDF links in the order of rr_link_poses (data/realrobot_model_links.txt), rows 17..19 objects 0..2;
 * the rows of objects the handle does not have stay zero.  Only contacts with |distance| < 0.1 count (robot.py:136, the test behind
 * RR_F_TOUCH: the max column of the four skin links IS RR_F_TOUCH of an env that stepped).  A contact whose body A is a robot body
 * (0..15) counts for the row of its linkA, one whose body A is object i for row 17 + i; a body B that is object j counts for row
 * 17 + j as well, with partner bit 4 if A is a robot body and bit 1 + i if A is object i.  The model's collision pairs have a robot
 * body or an object as A and a static body or an object as B -- no robot body is ever B, so bit 4 appears on object rows only.
 * max and sum of a row are taken over its contacts in ascending contact index, in float32, one after the other from 0: a
 * sequential float32 loop over rr_get_contacts' rows reproduces them bit for bit.
 * The fields hold what the LAST CALL computed: steps do not refresh them (RR_F_CONTACT_COUNT, which they do refresh, is the count
 * of the rows at the moment of the call only until the next step).  After rr_reset / rr_set_state of an env, or a step that refused
 * its command (error flag 2), the env has no contacts and the next call gives it all-zero rows.
 * The three buffers are allocated on first use -- by this call, or by rr_get_buffer / rr_copy_to_host of one of the fields --,
 * zero-filled, and valid until rr_destroy.
 * STREAM CONTRACT as for the other zero-copy views (rr_step): the kernel runs on the library's stream behind the steps enqueued before
 * it; readers on another stream order themselves after the call (event / rr_sync), and a later call rewrites the buffers in place.
 * Out of scope: friction forces, contact positions in body frames, per-link rows for body B (body B is never a robot body). */
int rr_contact_observations(rr_env *env);

/* Replaces REALRobotEnv.evaluateGoal (env.py:181-200) for all envs at once: score[i] = sum over the objects o of env i whose
 * goal_mask byte is non-zero (NULL: every object) of exp(-(ln 4 / 0.10) * |goal_pos[i][o] - position[i][o]|), computed on the
 * device from the state.  goal_pos: f32 [N, n_obj, 3] (host), goal_mask: u8 [N, n_obj] (host), score_out: f32 [N] (host). */
int rr_evaluate_goals(rr_env *env, const float *goal_pos_host, const uint8_t *goal_mask_host, float *score_out_host);

/* ---- Goals and episodes on the device (additive in ABI 7) -------------------------------------------------------------------------
 * A goal table and a per-env episode record live on the device; one launch per step (rr_episode_update) gives every env's score,
 * reward and done bits and, on request, resets the finished envs into their next goal -- no host round trip.  The record's buffers
 * are NOT fields of rr_get_buffer (RR_F_COUNT stays 16): they have this enum and rr_episode_buffer. */
enum {
    RR_EP_SCORE = 0,      /* f32 [N]            evaluateGoal of the env's goal at the last update (env.py:181-200); 0 without a goal */
    RR_EP_REWARD = 1,     /* f32 [N]            score - previous score, one float32 subtraction */
    RR_EP_DONE = 2,       /* u32 [N]            bit 0 truncated (RR_F_TIMESTEP >= horizon, env.py:345-352), bit 1 frozen (RR_F_ERRFLAGS & 5) */
    RR_EP_GOAL_INDEX = 3, /* i32 [N]            the env's row of the goal table, -1: no goal */
    RR_EP_EPISODE = 4,    /* i32 [N]            auto-resets of the env so far */
    RR_EP_FINAL_OBS = 5,  /* f32 [N, 9 + 4 + 7 n_obj + 1]  joints, touch, object poses and score of the env's last finished episode; zero before */
    RR_EP_GOAL_POS = 6,   /* f32 [N, n_obj, 3]  the goal's positions; NaN where the goal does not name the object, all NaN without a goal */
    RR_EP_GOAL_RGB = 7,   /* u8  [N, H, W, 3]   the goal's image; all zero without a goal.  Exists only while the table has images */
    RR_EP_COUNT = 8
};
/* Replaces the goal list of REALRobotEnv (load_goals / set_goal, env.py:151-166) with a device table of n_goals goals.  All arrays are
 * host memory: start_poses f32 [G, n_obj, 7] (xyz + xyzw quaternion), final_pos f32 [G, n_obj, 3], flags u8 [G, n_obj], goal_rgb u8
 * [G, H, W, 3] or NULL.  Flag bit 0: the object counts in the score (it is named in the goal's final_state); bit 1: the object has
 * a start pose (it is named in initial_state), otherwise it starts from its home pose (rr_set_object_home).  Values of rows whose
 * bit is clear are not read; a value that is read and is not finite returns RR_EINVAL (the message names goal and object) and
 * nothing changes.  A new table leaves EVERY env without a goal (index -1) until rr_set_env_goals: indices into the old table mean
 * nothing in the new one; n_goals == 0 drops the table.  Synchronous.
 * RR_EP_GOAL_RGB (N H W 3 bytes: 201 MB at 4096 envs of 128 x 128) is allocated by the first table that carries images and freed by a
 * later table without: ITS POINTER MAY CHANGE whenever the image status of the table changes -- ask rr_episode_buffer again after
 * rr_set_goals.  The pointers of all other RR_EP_* buffers survive rr_set_goals. */
int rr_set_goals(rr_env *env, int32_t n_goals, const float *start_poses, const float *final_pos, const uint8_t *flags, const uint8_t *goal_rgb);
/* Replaces the goal choice of REALRobotEnv.set_goal (env.py:151-158) for the envs whose mask byte is non-zero (NULL: all): goal_index
 * i32 [N] host, -1: no goal, else a row in [0, G) (rows of unmasked envs are not read).  Stores the index, refreshes the env's
 * RR_EP_GOAL_POS / RR_EP_GOAL_RGB and RE-BASES the env's previous score to the score of its CURRENT state: the next reward is taken
 * against it.  Does not move objects and does not touch the state (the next step stays prepared).  An index out of range returns
 * RR_EINVAL, the message names the env, and no env changes.  Synchronous. */
int rr_set_env_goals(rr_env *env, const int32_t *goal_index, const uint8_t *env_mask_host);
/* Episode rules of rr_episode_update: horizon > 0: an env is truncated once RR_F_TIMESTEP >= horizon (env.py:345-352); <= 0: never.
 * goal_stride: an auto-reset takes the env from goal index i to (i + goal_stride) mod G; 0 keeps the goal; -1 (no goal) stays.
 * Defaults: horizon 0, stride 1. */
int rr_set_episode(rr_env *env, int32_t horizon, int32_t goal_stride);
/* Replaces evaluateGoal and the `done` of step_joints (env.py:181-200, 345-352) and, with reset_done != 0, reset() + set_goal
 * (env.py:151-166, 206-219) of the finished envs, for ALL envs in one launch on the library's stream; checks the launch and does not
 * wait.  Per env: RR_EP_SCORE -- rr_evaluate_goals' arithmetic (one device function serves both) against the env's goal;
 * RR_EP_REWARD = score - previous score, and the previous score becomes the score; RR_EP_DONE.  With reset_done != 0 every env with
 * done != 0 then (1) gets its row of RR_EP_FINAL_OBS from the observation buffers as the step left them, (2) is reset as by rr_reset,
 * (3) moves to its next goal, (4) has the objects with a start pose placed as by rr_set_object_poses -- the others keep their home
 * pose --, (5) gets its RR_EP_GOAL_POS / RR_EP_GOAL_RGB refreshed, (6) has its previous score set to the score of the new start state
 * and (7) its RR_EP_EPISODE incremented; score, reward and done of this call still describe the FINISHED episode.  The observation
 * buffers are refreshed behind it and the next step prepares itself again, as after rr_reset; images are not rendered (rr_render).
 * With reset_done == 0 the call changes no simulation state.
 * The episode record is a setting of the handle, like the cameras: rr_reset, rr_set_state, rr_set_object_pose(s) and
 * rr_checkpoint_restore leave it alone and checkpoints do not carry it -- after such an outside change the caller re-bases the
 * previous score with rr_set_env_goals.
 * Out of scope: orientation terms of the score, success thresholds, per-env horizons. */
int rr_episode_update(rr_env *env, int32_t reset_done);
/* Zero-copy device pointer + size of an RR_EP_* buffer, valid until rr_destroy (RR_EP_GOAL_RGB: until the table's image status
 * changes, see rr_set_goals; RR_EINVAL for it while the table has no images).  The buffers are allocated on first use and
 * zero-filled, except that every env starts without a goal: RR_EP_GOAL_INDEX -1, RR_EP_GOAL_POS NaN.  STREAM CONTRACT as for the other
 * zero-copy views (rr_step): written on the library's stream, read-only for the caller. */
int rr_episode_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_EP_* buffer to host memory (rr_copy_to_host for the episode record). */
int rr_episode_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Kinematic observations on the device (additive in ABI 7) ----------------------------------------------------------------------
 * Replaces pybullet's getJointState(s) velocity, getLinkState(computeLinkVelocity=1), getBaseVelocity and calculateJacobian(body,
 * link, localPosition, ...) for ALL envs at once and on the device: one launch on the library's stream (rr_kinematic_observations)
 * turns the present state into seven device buffers.  They are NOT fields of rr_get_buffer (RR_F_COUNT stays 16): they have this
 * enum and rr_kinematic_buffer, like the episode record. */
enum {
    RR_KIN_JOINT_VEL = 0,  /* f32 [N, 11]        qd, the order of q[11] in RR_F_STATE                          getJointState(s)[1] */
    RR_KIN_LINK_POSE = 1,  /* f32 [N, 17, 7]     the rows of rr_link_poses (COM frame, xyz + xyzw)             getLinkState[0:2]   */
    RR_KIN_LINK_VEL = 2,   /* f32 [N, 17, 6]     world linear velocity of that frame's origin, then angular    getLinkState[6:8]   */
    RR_KIN_OBJ_VEL = 3,    /* f32 [N, n_obj, 6]  linear, angular                                               getBaseVelocity     */
    RR_KIN_POINT_POS = 4,  /* f32 [N, P, 3]      world position of every point in force                                            */
    RR_KIN_POINT_VEL = 5,  /* f32 [N, P, 6]      its world linear velocity, its link's angular velocity                            */
    RR_KIN_JACOBIAN = 6,   /* f32 [N, P, 6, 11]  rows: linear xyz, angular xyz; columns: q[11]                 calculateJacobian   */
    RR_KIN_COUNT = 7
};
#define RR_KIN_MAX_POINTS 8
/* The points of RR_KIN_POINT_POS / RR_KIN_POINT_VEL / RR_KIN_JACOBIAN: point j is (link[j], local_pos[j]) -- a URDF link id in
 * [0, 17), the order of rr_link_poses and data/realrobot_model_links.txt, and a position in that link's COM frame (pybullet's
 * localPosition; local_pos f32 [P][3] host, NULL: zeros).  Its world position is x = p_link + R_link local_pos.  A fresh handle
 * has ONE point: link 8 (gripper `base`, the link rr_ik solves for) at (0, 0, 0).  n_points outside [1, RR_KIN_MAX_POINTS], a
 * link out of range or a local_pos that is not finite returns RR_EINVAL -- the message names the point -- and the points in force
 * stay as they are.  The points are a setting of the handle, like the cameras: rr_reset, rr_set_state, rr_copy_envs and
 * rr_checkpoint_restore keep them and checkpoints do not carry them.  Synchronous (it waits for the library's stream: an
 * observation call enqueued earlier still sees the earlier points) and launches nothing; after a change the three point buffers
 * hold unspecified data until the next rr_kinematic_observations. */
int rr_set_kinematic_points(rr_env *env, int32_t n_points, const int32_t *link, const float *local_pos);
/* The points in force: *n_points, link_out i32 [P], local_pos_out f32 [P][3] (room for RR_KIN_MAX_POINTS); each output may be NULL. */
int rr_get_kinematic_points(rr_env *env, int32_t *n_points, int32_t *link_out, float *local_pos_out);
/* One launch on the library's stream turns the PRESENT state -- whatever the last step, reset, rr_set_state, rr_set_object_pose(s),
 * rr_copy_envs or restore left -- into the seven buffers; the call checks the launch and returns without waiting.  It reads the
 * state (joint positions and velocities, object velocities), the model and the points, and writes the seven buffers only: not the
 * preparation record (RR_F_PREP: after an outside change of state that describes an older state), no error flag; the next step
 * stays prepared and no later step is affected.  The buffers hold what the LAST CALL computed: steps do not refresh them.
 * For link l on moving body b with COM-frame origin x, over the joints k that move b (b and its ancestors), with world joint axis
 * a_k and joint position p_k:   v = sum_k qd_k a_k x (x - p_k),   w = sum_k qd_k a_k;   a point takes its own x.  Column k of a
 * point's Jacobian is [a_k x (x - p_k); a_k] for such a k and +0.0 in all six rows otherwise.  Link 0 is rigid with the world: its
 * velocity row, and the velocity and every Jacobian column of a point on it, are +0.0.  Plain float32 arithmetic on the frames of
 * the step's own forward kinematics; RR_KIN_LINK_POSE is the expression of rr_link_poses.  RR_KIN_JOINT_VEL and RR_KIN_OBJ_VEL are
 * the floats of RR_F_STATE, bit for bit: its columns 11..21, and per object the six behind pos3 quat4.  An env whose state is not
 * finite (error flag 1) is computed like any other: its rows may be non-finite.
 * The Jacobian's columns are the eleven joints as INDEPENDENT coordinates.  The nine command entries drive them as Kuka.apply_action
 * does (robot.py:188-201): command c < 7 drives q[c]; command 7 drives q[7] and q[9]; command 8 drives -q[8] and -q[10].  With that
 * [11, 9] matrix Q, dq = Q dcmd and the Jacobian over the commands is J Q.
 * All seven buffers are allocated on first use -- by this call, or by rr_kinematic_buffer / rr_kinematic_copy_to_host --, all or
 * nothing, zero-filled, and valid until rr_destroy.  The three point buffers are allocated once for RR_KIN_MAX_POINTS points, so
 * no pointer ever changes; their layout is compact [N, P, ...] for the P in force, and `bytes` reports that size.
 * STREAM CONTRACT as for the other zero-copy views (rr_step, rr_contact_observations): the kernel runs on the library's stream behind
 * the work enqueued before it; readers on another stream order themselves after the call (event / rr_sync), and a later call
 * rewrites the buffers in place.
 * Out of scope: mass matrix, bias and gravity terms (the motors are position controlled: nothing here would consume them), Jacobian
 * time derivatives, URDF link frames (COM frames only, as rr_link_poses), points on objects, refreshing from inside a step. */
int rr_kinematic_observations(rr_env *env);
/* Zero-copy device pointer + size in bytes of an RR_KIN_* buffer (read-only for the caller); which outside [0, RR_KIN_COUNT): RR_EINVAL. */
int rr_kinematic_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_KIN_* buffer (its `bytes`) to host memory. */
int rr_kinematic_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Ray casts against the collision hulls on the device (additive in ABI 7) ---------------------------------------------------------
 * Replaces pybullet's rayTestBatch(rayFromPositions, rayToPositions, parentObjectUniqueId = robot, parentLinkIndex) for ALL envs at
 * once and on the device: "what does this segment hit first, where, and with which normal" -- proximity and height sensors on the
 * gripper, clearance checks along an approach, cheap range scans, line-of-sight tests.  One launch on the library's stream
 * (rr_ray_cast) casts R segments per env against the model's convex collision hulls -- the shapes the step's collision pass uses:
 * table, shelf, the robot's links, the handle's objects -- at the present state and writes two device buffers.  They are NOT fields
 * of rr_get_buffer (RR_F_COUNT stays 16): they have this enum and rr_ray_buffer, like the kinematic observations. */
enum {
    RR_RAY_HIT = 0,   /* f32 [N, R, 8]  {fraction, distance (m) = fraction * |to - from|, x, y, z (world), nx, ny, nz (world, outward)} */
    RR_RAY_ID = 1,    /* i32 [N, R, 4]  {uid as in RR_F_MASK, body as in the contact records (-1 static, 0..15 robot body, 16 + i object i),
                                         URDF link of the shape or -1, collision shape index}; all -1 on a miss */
    RR_RAY_COUNT = 2
};
#define RR_RAY_MAX 64
/* The ray table: R = n_rays rays in [0, RR_RAY_MAX].  Ray j has a frame -- link[j] = -1: the world; a URDF link id in [0, 17): that
 * link's COM frame, the frame of rr_link_poses and of the kinematic points, pybullet's parentLinkIndex -- and a default segment
 * from_to[j] = {from xyz, to xyz} in that frame (f32 [R][6] host; NULL: all zeros, legal only if every cast brings its own segments:
 * a zero-length segment is a miss).  A fresh handle has R = 0.  n_rays out of range, a link outside {-1} u [0, 17) or a coordinate
 * that is not finite returns RR_EINVAL -- the message names the ray -- and the table in force stays as it is.  The table is a setting
 * of the handle, like the kinematic points: rr_reset, rr_set_state, rr_write_state, rr_copy_envs and rr_checkpoint_restore keep it
 * and checkpoints do not carry it.  Synchronous (it waits for the library's stream: a cast enqueued earlier still sees the earlier
 * table) and launches nothing; after a change the two buffers hold unspecified data until the next rr_ray_cast. */
int rr_set_rays(rr_env *env, int32_t n_rays, const int32_t *link, const float *from_to);
/* The table in force: *n_rays, link_out i32 [R], from_to_out f32 [R][6] (room for RR_RAY_MAX); each output may be NULL. */
int rr_get_rays(rr_env *env, int32_t *n_rays, int32_t *link_out, float *from_to_out);
/* One launch on the library's stream casts the R segments of every env against the hulls at the PRESENT state -- whatever the last
 * step, reset, rr_set_state, rr_write_state, rr_set_object_pose(s), rr_copy_envs or restore left -- and writes the two buffers; the
 * call checks the launch and returns without waiting.  The kernel does its own forward kinematics from the state: it reads the state
 * and the model only, not the preparation record (RR_F_PREP), changes no error flag, the next step stays prepared and no later step
 * is affected.  The buffers hold what the LAST CALL computed: steps do not refresh them.
 * rays == NULL: every env casts the table's segments.  Otherwise rays is f32 [N, R, 6], per-env segments {from xyz, to xyz} in the
 * frames of the table's links.  on_device != 0: device memory, read IN PLACE on the library's stream under the STREAM CONTRACT of
 * rr_step's cmd_on_device (produced on that stream or ordered before it; not rewritten before later work on that stream), nothing
 * is allocated or staged and the values are not validated.  on_device == 0: host memory, checked finite (RR_EINVAL naming env and
 * ray, nothing cast), staged, and the call waits for the stream -- the split of rr_write_state.  R == 0: RR_EINVAL.
 * Semantics.  A shape's frame is the identity for the statics (table, shelf, the robot's fixed base), the body frame of the step's
 * forward kinematics for a robot shape, and the object's pose for an object, with the rotation the step forms from the quaternion.
 * The out-of-bounds re-pose of the step is not applied: the state is taken as it is.  Shapes of objects >= n_objects do not exist.
 * A hull is the set {x : n_k . x - d_k <= 0 for all k} of its up to 192 planes.  For one segment o + t (to - from), t in [0, 1],
 * expressed in a hull's frame: t_in is the largest entry parameter over the planes with n . dir < 0, t_out the smallest exit
 * parameter over those with n . dir > 0; a plane parallel to the segment with the origin outside it rules the hull out.  The hull is
 * hit iff the origin is outside it, t_in >= 0 and t_in <= min(t_out, 1).  The fraction is t_in and the normal that of the entering
 * plane, turned into the world; among equal entry parameters the lowest plane index wins.  An origin INSIDE a hull (or on its
 * surface) does not hit THAT hull -- Bullet's convex cast, and what lets a sensor sit inside its own link.  Over the hulls the
 * smallest float32 fraction wins; equal fractions go to the lowest shape index.  A miss gives fraction 1.0, distance |to - from|,
 * position the world end point, normal +0.0 and ids -1.  A zero-length segment is a miss.  A segment with a non-finite value (device
 * path only) is a miss whose float fields may be non-finite.  An env whose state is not finite is computed like any other: its rows
 * are unspecified.  No ray or state value ever forms an address.  Plain float32 arithmetic; the result is a function of the state
 * and the segments alone (no atomics: identical from call to call).
 * Both buffers are allocated on first use -- by this call, or by rr_ray_buffer / rr_ray_copy_to_host --, all or nothing, zero-filled,
 * once for RR_RAY_MAX rays, and valid until rr_destroy: no pointer ever changes.  Their layout is compact [N, R, ...] for the R in
 * force, and `bytes` reports that size.  STREAM CONTRACT as for the other zero-copy views (rr_step, rr_kinematic_observations): the
 * kernel runs on the library's stream behind the work enqueued before it; readers on another stream order themselves after the call
 * (event / rr_sync), and a later call rewrites the buffers in place.
 * Out of scope: the render meshes (the hulls are the collision shapes, coarser than what the camera sees), collision filter masks,
 * more than 64 rays per env, all hits along a ray (the first only), rays in object frames, refreshing from inside a step. */
int rr_ray_cast(rr_env *env, const float *rays, int32_t on_device);
/* Zero-copy device pointer + size in bytes of an RR_RAY_* buffer (read-only for the caller); which outside [0, RR_RAY_COUNT): RR_EINVAL. */
int rr_ray_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_RAY_* buffer (its `bytes`) to host memory. */
int rr_ray_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Closest points between collision hulls on the device (additive in ABI 7) --------------------------------------------------------
 * Replaces pybullet's getClosestPoints(bodyA, bodyB, distance, linkIndexA, linkIndexB) for ALL envs at once and on the device: "how
 * far apart are these two bodies, and where are the nearest points" -- clearance costs of rollouts on forked envs, reach and grasp
 * shaping by the surface distance of a pad and an object, early termination on a keep-out distance.  One launch on the library's
 * stream (rr_closest_points) computes Q pairs of collision shapes per env -- the convex shapes the step's collision pass uses: table,
 * shelf, the robot's links, the handle's objects -- at the present state and writes two device buffers.  They are NOT fields of
 * rr_get_buffer (RR_F_COUNT stays 16): they have this enum and rr_distance_buffer, like the ray casts. */
enum {
    RR_DIST_POINTS = 0,   /* f32 [N, Q, 12] {distance (m), lower bound (m), a xyz, b xyz (world), n xyz (world, from b towards a), +0.0} */
    RR_DIST_ID = 1,       /* i32 [N, Q, 4]  {status, iterations, body A, body B}: bodies as in the contact records (-1 static, 0..15 robot
                                             body, 16 + i object i) */
    RR_DIST_COUNT = 2
};
#define RR_DIST_MAX 96      /* = the model's pair capacity: the step's whole collision table fits */
/* The pair table: Q = n_pairs pairs in [0, RR_DIST_MAX].  Pair j is two collision-shape indices shape_a[j], shape_b[j] (i32 [Q],
 * host): the index is column 3 of RR_RAY_ID, the order of the model blob's shape_owner.  A fresh handle has Q = 0.  n_pairs == -1
 * (the arrays are ignored) installs the step's own collision pairs in list order -- every object x every static shape, object x
 * object, every moving robot shape x table and shelf, every moving robot shape x every object; pairs of objects the handle does not
 * have are left out (92 pairs at three objects).  max_distance (m) is the cull: a pair whose bounding spheres are further apart gets
 * status 2 instead of a search; max_distance <= 0 or +inf: no cull.  n_pairs out of range, an index outside the model's shapes,
 * a == b, a shape of an object >= n_objects, a NaN max_distance or a null array with n_pairs > 0 returns RR_EINVAL -- the message
 * names the pair -- and the table in force stays as it is.  The table is a setting of the handle, like the rays: rr_reset,
 * rr_set_state, rr_write_state, rr_copy_envs and rr_checkpoint_restore keep it and checkpoints do not carry it.  Synchronous (it waits
 * for the library's stream: a query enqueued earlier still sees the earlier table) and launches nothing; after a change the two
 * buffers hold unspecified data until the next rr_closest_points. */
int rr_set_distance_pairs(rr_env *env, int32_t n_pairs, const int32_t *shape_a, const int32_t *shape_b, float max_distance);
/* The table in force: *n_pairs, shape_a_out / shape_b_out i32 [Q] (room for RR_DIST_MAX), *max_distance_out; each output may be NULL. */
int rr_get_distance_pairs(rr_env *env, int32_t *n_pairs, int32_t *shape_a_out, int32_t *shape_b_out, float *max_distance_out);
/* One launch on the library's stream computes the Q pairs of every env at the PRESENT state -- whatever the last step, reset,
 * rr_set_state, rr_write_state, rr_set_object_pose(s), rr_copy_envs or restore left -- and writes the two buffers; the call checks the
 * launch and returns without waiting.  The kernel does its own forward kinematics from the state: it reads the state, the model and
 * the table only, not the preparation record (RR_F_PREP), changes no error flag, the next step stays prepared and no later step is
 * affected.  The buffers hold what the LAST CALL computed: steps do not refresh them.  Q == 0: RR_EINVAL.
 * Semantics.  A shape is the CONVEX HULL OF ITS VERTEX SET (up to 192 vertices, the blob's shape_verts) -- not the intersection of its
 * planes, which the model compiler fitted within 0.3 mm of the vertices and which the ray casts and the step's collision pass use.
 * A shape's frame is that of rr_ray_cast: the identity for the statics (table, shelf, the robot's fixed base), the body frame of the
 * step's forward kinematics for a robot shape, and the object's pose for an object, with the rotation the step forms from the
 * quaternion.  The out-of-bounds re-pose of the step is not applied: the state is taken as it is.
 * distance is the Euclidean distance of the two hulls; a and b are world points of A and B that realise it (|a - b| = distance; the
 * points need not be unique, the vector a - b is); n = (a - b) / distance is the unit vector from b towards a, pybullet's
 * contactNormalOnB; lower bound is a value the search has proved <= the distance, from the support plane of its last directions:
 * distance - lower bound bounds the error of distance from above.  status:
 *   0  separated and converged: the fields as above;
 *   1  overlapping or touching (a distance of at most 1e-6 m counts as touching): distance = lower bound = 0, n = +0.0, a = b = some
 *      finite point.  PENETRATION DEPTH IS OUT OF SCOPE: inside the 2 cm margin the contact records (rr_contact_observations) carry
 *      it; there is no negative distance;
 *   2  culled: the gap of the two bounding spheres (the blob's shape_sphere, which hold the vertices) exceeds max_distance; distance =
 *      lower bound = that gap (a true lower bound of the hull distance), a and b the points of the spheres on the line of their
 *      centres, n along the centres; iterations = 0;
 *   3  the iteration cap (32) was reached: distance is an upper bound (|a - b| of two points of the hulls), lower bound the best
 *      bound proved.
 * The search is GJK in float32 on the vertex sets.  It ends with status 0 when (distance - lower bound) <= 1e-12 distance (squared norms are summed in float64), when the
 * support vertex pair is already in the simplex, or when rounding allows no nearer point.  Support ties go to the lowest vertex
 * index, reductions run in a fixed order, there are no atomics: the result is a function of the state and the table alone,
 * identical from call to call, independent of N, of the env's position in the batch and of its neighbours; row (env, j) depends on
 * pair j alone, so a permuted table gives permuted rows.  Every loop bound is a constant or a model count, never data: an env
 * whose state is not finite is computed like any other and finishes like any other; its rows are unspecified.  No state value ever
 * forms an address.
 * Both buffers are allocated on first use -- by this call, or by rr_distance_buffer / rr_distance_copy_to_host --, all or nothing,
 * zero-filled, once for RR_DIST_MAX pairs, and valid until rr_destroy: no pointer ever changes.  Their layout is compact [N, Q, ...]
 * for the Q in force, and `bytes` reports that size.  STREAM CONTRACT as for the other zero-copy views (rr_step, rr_ray_cast): the
 * kernel runs on the library's stream behind the work enqueued before it; readers on another stream order themselves after the call
 * (event / rr_sync), and a later call rewrites the buffers in place.
 * Out of scope: penetration depth and negative distances, an all-pairs broad phase, groups of shapes reduced on the device (a min
 * over columns in the caller's tensor program does it), points in body frames, the render meshes, refreshing from inside a step. */
int rr_closest_points(rr_env *env);
/* Zero-copy device pointer + size in bytes of an RR_DIST_* buffer (read-only for the caller); which outside [0, RR_DIST_COUNT): RR_EINVAL. */
int rr_distance_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_DIST_* buffer (its `bytes`) to host memory. */
int rr_distance_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Clearance at candidate joint postures on the device (additive in ABI 7) ----------------------------------------------------------
 * The question of planners, MPPI / CEM samplers and trajectory optimisers: "how much clearance would the arm have at THESE K joint
 * postures, given where this env's objects are now?"  One launch on the library's stream (rr_posture_clearance) evaluates K candidate
 * postures per env of the whole batch against the pair table of rr_set_distance_pairs and writes four device buffers: per posture the
 * distance and status of every pair, and the full record of the NEAREST pair, reduced on the device.  Nothing of the simulation is
 * disturbed, and no handle of N * K envs is needed.  The buffers are NOT fields of rr_get_buffer and not RR_DIST_* buffers
 * (RR_F_COUNT stays 16, RR_DIST_COUNT stays 2): they have this enum and rr_posture_buffer. */
enum {
    RR_PC_NEAREST = 0,    /* f32 [N, K, 12] the RR_DIST_POINTS row {distance, lower bound, a xyz, b xyz, n xyz, +0.0} of the nearest pair of that posture */
    RR_PC_ID = 1,         /* i32 [N, K, 4]  {status of that row, pair index j in the table, body A, body B} */
    RR_PC_DISTANCE = 2,   /* f32 [N, K, Q]  the distance column of every pair, as rr_closest_points would report it */
    RR_PC_STATUS = 3,     /* i32 [N, K, Q]  byte 0: status 0..3, byte 1: iterations, bytes 2..3: zero */
    RR_PC_COUNT = 4
};
#define RR_PC_MAX_POSTURES 32
/* What is computed.  Posture (e, k), k in [0, K = n_postures), is evaluated as if columns 0..10 of env e's RR_F_STATE row were
 * postures[e][k][0..10]; the objects stay at env e's PRESENT pose -- whatever the last step, reset, rr_set_state, rr_write_state,
 * rr_set_object_pose(s), rr_copy_envs or restore left (an object attached to a link, rr_set_attachments, moves with that link instead).
 * The pair table and the cull are those of rr_set_distance_pairs, and a pair
 * means exactly what it means to rr_closest_points (the block above: the convex hulls of the vertex sets, the shapes' frames, the
 * statuses 0 to 3, the relative gap 1e-12 that ends the search, touching at 1e-6 m, the cap of 32 trips, support ties to the lowest
 * vertex index); the two kernels run the same device text for a pair.
 * Input.  postures is f32 [N][K][11], C order: the eleven INDEPENDENT joints in the order of the state's q[11].  The nine entries of a
 * joint command map into them through the binding's _native.Q_FROM_CMD (the coupled finger joints follow their drivers); this call
 * takes the 11 columns only.
 * The nearest row.  RR_PC_NEAREST / RR_PC_ID hold the pair at the FIRST MINIMUM of that posture's RR_PC_DISTANCE row: the lowest
 * pair index among equal values, so two overlapping pairs tie at 0 and the lower index wins.  A culled pair (status 2) takes part with
 * its sphere gap, a status-3 pair with its upper bound; the status in RR_PC_ID says which kind won.  The comparison is d < best over
 * ascending j, starting from pair 0 with best = +inf: a NaN never wins against a number, and the pair index is always in [0, Q) (pair 0
 * where no distance of the row is below +inf).
 * No effect on the simulation.  The call reads the state (the objects' columns), the model, the pair table and the tensor, and writes
 * the four buffers only: not the state, not the preparation record (RR_F_PREP), no error flag, no RR_DIST_* buffer.  The next step
 * stays prepared and no later step is affected.  The buffers hold what the LAST CALL computed.
 * on_device != 0: postures is device memory, read IN PLACE on the library's stream under the STREAM CONTRACT of rr_step's
 * cmd_on_device (produced on that stream or ordered before it; not rewritten before later work on that stream); the call allocates
 * nothing beyond the first-use buffers, checks the launch and returns without waiting.  on_device == 0: host memory, staged through a
 * buffer of the handle's own (N * 32 * 11 floats, allocated by the first such call), and the call waits for the stream.
 * Values are NOT validated on either path.  A non-finite posture, or an env whose object pose is not finite, is computed like any
 * other and finishes like any other -- every loop bound is a constant or a model count -- and its rows are unspecified (the pair
 * index stays in [0, Q), the status bytes in 0..3, the iterations <= 32).  No value of the tensor ever forms an address.
 * Errors: RR_EINVAL with nothing changed, the message naming the cause, for a null env, null postures, n_postures outside
 * [1, RR_PC_MAX_POSTURES], and Q == 0 (an empty pair table).
 * Buffers.  All four are allocated on first use -- by this call, or by rr_posture_buffer / rr_posture_copy_to_host --, all or nothing
 * through the handle's memory owner, zero-filled, sized once for RR_PC_MAX_POSTURES x RR_DIST_MAX, and valid until rr_destroy: no
 * pointer ever changes.  The layout is compact [N, K, ...] for the K of the last query and the Q in force, and `bytes` reports that;
 * before the first query K counts as 0.  After rr_set_distance_pairs the buffers hold unspecified data until the next query.  STREAM
 * CONTRACT for readers as for the other zero-copy views: the kernel runs on the library's stream behind the work enqueued before it;
 * readers on another stream order themselves after the call (event / rr_sync), and a later call rewrites the buffers in place.
 * Determinism.  No atomics and a fixed reduction order: row (e, k) is a function of (env e's objects, posture (e, k), the table)
 * alone -- identical from call to call, independent of N, of K, of the row's place and of its neighbours.
 * Out of scope: candidate object poses; per-posture pair tables; signed distances and penetration depth (rr_signed_distance);
 * gradients over the joints (rr_signed_gradient computes them at the candidate postures themselves; n . (J_a - J_b) with the
 * Jacobians of rr_kinematic_observations holds at the present state only); rays and kinematics at candidate postures; a switch of
 * the vector env (postures are an argument, not an observation). */
int rr_posture_clearance(rr_env *env, const float *postures /* f32 [N][K][11] */, int32_t n_postures, int32_t on_device);
/* Zero-copy device pointer + size in bytes of an RR_PC_* buffer (read-only for the caller); which outside [0, RR_PC_COUNT): RR_EINVAL. */
int rr_posture_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_PC_* buffer (its `bytes`) to host memory. */
int rr_posture_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Signed distance and penetration depth on the device (additive in ABI 7) -----------------------------------------------------------
 * rr_closest_points and rr_posture_clearance stop at the surface: every overlapping pair is "0".  This query goes on: over the pair
 * table of rr_set_distance_pairs, for every env at once, a pair whose hulls are apart gets what rr_closest_points reports, and a pair
 * whose hulls OVERLAP gets a NEGATIVE distance, minus the penetration depth -- the length of the shortest translation of shape a that
 * separates the two convex hulls --, the direction of that translation, two witness points and a proved bound: what pybullet's
 * getClosestPoints returns for penetrating bodies, and what a sampler needs to tell a finger 1 mm into the cube from a forearm 20 cm
 * through the table and to push the candidate out.  One launch on the library's stream, at the present state or at K candidate joint
 * postures per env.  The buffers are NOT fields of rr_get_buffer and not RR_DIST_* / RR_PC_* buffers (RR_F_COUNT stays 16,
 * RR_DIST_COUNT 2, RR_PC_COUNT 4): they have this enum and rr_signed_buffer.  K' below is 1 for a present-state query, else K. */
enum {
    RR_SD_DEEPEST = 0,    /* f32 [N, K', 12] {signed distance, bound, a xyz, b xyz, n xyz, +0.0} of the pair at the FIRST MINIMUM of that row's signed distances */
    RR_SD_ID = 1,         /* i32 [N, K', 4]  {status of that row, pair index j in the table, body A, body B} */
    RR_SD_SIGNED = 2,     /* f32 [N, K', Q]  the signed distance of every pair */
    RR_SD_STATUS = 3,     /* i32 [N, K', Q]  byte 0: status 0..5, byte 1: GJK iterations, byte 2: expansion trips, byte 3: zero */
    RR_SD_POINTS = 4,     /* f32 [N, Q, 12]  the full record of every pair; written by a PRESENT-STATE query only */
    RR_SD_COUNT = 5
};
/* Arguments.  postures == NULL with n_postures == 0: the present state -- one row per env, K' = 1, the joints from the state.
 * Otherwise the arguments are exactly those of rr_posture_clearance: postures f32 [N][K][11], K = n_postures in
 * [1, RR_PC_MAX_POSTURES], the objects at env e's present pose; on_device != 0: device memory read in place on the library's stream
 * under that call's STREAM CONTRACT, the call returns without waiting; on_device == 0: host memory, staged, and the call waits.
 * Shapes, frames, the pair table, the cull and the GJK (relative gap 1e-12, touching at 1e-6 m, 32 trips, ties to the lowest vertex
 * index) are those of rr_closest_points.
 * The record.  For both signs a is a point of hull A, b a point of hull B, n a unit vector from b towards a, and a - b = signed * n.
 * Separated (status 0, 2, 3): the RR_DIST_POINTS row of rr_closest_points.  Overlapping (status 1): signed = -depth, where depth is
 * the smallest separating translation the search found: moving shape a by depth * n separates the hulls (depth is the width of the
 * overlap along n: max over B of n . b minus min over A of n . a), so it is an upper bound of the true depth and one that is always
 * achievable; bound = -(the distance of the search polytope's nearest face from the origin of the Minkowski difference), a proved
 * lower bound of the depth: -bound <= true depth <= -signed.  a and b are the barycentric weights, on the two shapes' support
 * vertices, of the origin's projection on that nearest face (of coplanar faces the one that holds the projection); like the closest
 * points of parallel faces they need not be unique.  status:
 *   0  separated and converged;
 *   1  overlapping, the expansion converged: (-signed) - (-bound) <= 1e-6 m, or the support vertex pair was already a vertex of
 *      the polytope;
 *   2  culled by max_distance (the spheres' gap, as rr_closest_points);
 *   3  the GJK's iteration cap (32): signed is an upper bound of the distance;
 *   4  touching: the GJK ended with a distance of at most 1e-6 m, or its tetrahedron was too flat to expand; signed = bound = 0,
 *      n = +0.0, a = b = some finite point: the status-1 row of rr_closest_points;
 *   5  the expansion's cap (32 trips, or more than 64 faces): signed (the smallest width seen, with its n) and bound are still valid
 *      bounds of the depth; a and b are those of the nearest face, and a - b = signed * n holds only as far as the bounds agree.
 * The search for the depth is an expanding polytope from the GJK's final tetrahedron, one wave per pair, in float32 with float64
 * face normals and plane distances; ties (nearest face, support vertex) go to the lowest lane / vertex index, every reduction runs
 * in a fixed order, there are no atomics: a row is a function of (env e's objects, its joints, the table) alone -- identical from
 * call to call, independent of N, K, the row's place and its neighbours, and a permuted table gives permuted columns.  Every loop
 * bound is a constant, a model count or a count of at most 64 faces, never a coordinate: a non-finite posture or state is computed
 * like any other and finishes like any other; its rows are unspecified (the pair index stays in [0, Q), the status in 0..5, the
 * iterations and trips <= 32).  No value of the tensor or the state ever forms an address.
 * The deepest row.  RR_SD_DEEPEST / RR_SD_ID hold the pair at the first minimum of the row's RR_SD_SIGNED values, by
 * rr_posture_clearance's rule: d < best over ascending j from best = +inf -- the lowest pair index among equal values, pair 0 where
 * nothing is below +inf; a NaN never wins.  A culled pair takes part with its sphere gap.
 * RR_SD_POINTS is written by a present-state query only; a posture query leaves it untouched (at K = 32 it would be 600 MB for
 * 4096 envs, which is why the posture form keeps the layout of rr_posture_clearance).
 * No effect on the simulation.  The call reads the state, the model, the pair table and the tensor and writes these five buffers
 * only: not the state, not the preparation record, no error flag, no RR_DIST_* or RR_PC_* buffer.  The next step stays prepared.
 * Errors: RR_EINVAL with nothing allocated and no buffer pointer changed, the message naming the cause, for a null env, an empty
 * pair table, n_postures outside [1, RR_PC_MAX_POSTURES] with postures given, and postures == NULL with n_postures != 0.
 * Buffers.  All five are allocated on first use -- by this call, or by rr_signed_buffer / rr_signed_copy_to_host --, all or nothing
 * through the handle's memory owner, zero-filled, sized once for RR_PC_MAX_POSTURES x RR_DIST_MAX (RR_SD_POINTS for RR_DIST_MAX), and
 * valid until rr_destroy: no pointer ever changes.  The layout is compact for the K' of the last query (0 before the first) and the
 * Q in force, and `bytes` reports that; RR_SD_POINTS reports N * Q * 48.  After rr_set_distance_pairs the buffers hold unspecified
 * data until the next query.  STREAM CONTRACT for readers as for the other zero-copy views: the kernel runs on the library's stream
 * behind the work enqueued before it; readers on another stream order themselves after the call (event / rr_sync), and a later call
 * rewrites the buffers in place.
 * Out of scope: gradients with respect to the joints (rr_signed_gradient below: this query plus the gradients); a switch of the
 * vector env; penetration of non-convex shapes (a shape is the convex hull of its vertex set); any use by the step -- the step's
 * own narrow phase is untouched. */
int rr_signed_distance(rr_env *env, const float *postures /* f32 [N][K][11] or NULL */, int32_t n_postures, int32_t on_device);
/* Zero-copy device pointer + size in bytes of an RR_SD_* buffer (read-only for the caller); which outside [0, RR_SD_COUNT): RR_EINVAL. */
int rr_signed_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_SD_* buffer (its `bytes`) to host memory. */
int rr_signed_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Joint gradients of the signed distance on the device (additive in ABI 7) ----------------------------------------------------------
 * What a trajectory optimiser needs and a sampler does not: d(signed distance) / d(joint), at the present state or AT the K candidate
 * postures -- where rr_kinematic_observations has no Jacobian to offer.  One call is rr_signed_distance with the same arguments plus,
 * per row, the gradient of the deepest pair's signed distance over the eleven joints, a hinge collision cost over ALL pairs and that
 * cost's gradient, both reduced on the device; a present-state query also gets every pair's gradient.  The buffers are not fields of
 * rr_get_buffer and not buffers of the queries above (RR_F_COUNT stays 16, the count of the signed-distance enum 5): they have this
 * enum and rr_signed_gradient_buffer.  K' is 1 for a present-state query, else K. */
enum {
    RR_SG_GRADIENT = 0,       /* f32 [N, K', 12] {d s* / dq_0..10, +0.0}: s* the signed distance of the row's RR_SD_DEEPEST pair */
    RR_SG_COST = 1,           /* f32 [N, K', 12] {dC / dq_0..10, C} */
    RR_SG_PAIR_GRADIENT = 2,  /* f32 [N, Q, 12]  {d s_j / dq_0..10, +0.0} of every pair; written by a PRESENT-STATE query only */
    RR_SG_COUNT = 3
};
/* Arguments.  env, postures, n_postures and on_device mean what they mean to rr_signed_distance: the present state (NULL, 0) or
 * K <= RR_PC_MAX_POSTURES postures f32 [N][K][11], device memory read in place under that call's STREAM CONTRACT or host memory
 * staged (the call then waits); values are not validated.  margin (m, finite, >= 0) is the distance below which a pair costs.
 * What the call writes.  The five buffers of rr_signed_distance get what rr_signed_distance with the same arguments would write,
 * byte for byte (so the per-pair columns exist once, and rr_signed_buffer reads them); the three RR_SG_* buffers are written in addition.
 * The gradient.  With the record of pair j -- a on shape A, b on shape B, n the unit normal from b towards a, a - b = s n for both
 * signs of the signed distance s --,
 *     ds/dq_k = [joint k moves A's body] n . (a_k x (a - p_k)) - [joint k moves B's body] n . (a_k x (b - p_k)),
 * a_k the world axis of joint k at that row's posture and p_k its position; "moves": k is the body's own joint or an ancestor's.
 * Static shapes (table, shelf, robot_base) and the objects have no columns: the objects stay where they are, as for
 * rr_posture_clearance, and a joint that moves neither shape gets +0.0.  (An object attached to a link, rr_set_attachments, moves with that
 * link and takes the columns of the link's body.)  The columns are over the eleven independent joints of the
 * state's q[11]; over the nine command entries the gradient is gradient @ Q_FROM_CMD of the binding.  By status of the pair:
 * 0, 1: the gradient of the signed distance; 2 (culled): the same expression on the sphere points, exactly the gradient of the
 * reported sphere gap; 3, 5: the expression on the record as reported; 4 (touching, n = +0.0): +0.0 in every column.  Where the
 * witness features switch (face against face, parallel edges) s has a kink: the result is the gradient of the ACTIVE feature pair,
 * a generalised gradient, and like the witness points themselves it need not be unique there.  Plain float32.
 * The cost.  With c_j = margin - s_j where that is > 0 and 0 otherwise (a NaN therefore contributes nothing),
 *     C = 1/2 sum_j c_j^2,     dC/dq = - sum_j c_j ds_j/dq,
 * over every pair of the table with its RR_SD_SIGNED value; margin 0 counts penetrations only.
 * Summation order: each of the row's four waves sums its pairs j = w, w + 4, ... ascending, in float32, from +0.0; then the waves
 * are summed in the order 0, 1, 2, 3.  No atomics: a row is identical from call to call and independent of N, K, the row's place
 * and its neighbours.  RR_SG_PAIR_GRADIENT rows follow a permuted table; the cost sums do NOT stay bit-identical under a permuted
 * table (another order of the same terms).
 * No effect on the simulation: the call reads what rr_signed_distance reads and writes these eight buffers only; the next step stays
 * prepared.  Every loop bound is a constant or a count, no value of the tensor or the state forms an address; non-finite input
 * finishes like any other and its rows are unspecified.
 * Errors: RR_EINVAL with nothing allocated and nothing changed, the message naming the cause, for what rr_signed_distance refuses
 * (null env, an empty pair table, n_postures outside [1, RR_PC_MAX_POSTURES] with postures given, NULL postures with n_postures
 * != 0), for a margin that is NaN, infinite or negative, and for a cull in force (0 < max_distance < inf) with margin >
 * max_distance: a culled pair's sphere gap would then enter the hinge as if it were a distance.
 * Buffers.  All three are allocated on first use -- by this call, or by rr_signed_gradient_buffer /
 * rr_signed_gradient_copy_to_host --, all or nothing through the handle's memory owner, zero-filled, sized once for
 * RR_PC_MAX_POSTURES rows (RR_SG_PAIR_GRADIENT for RR_DIST_MAX pairs) and valid until rr_destroy: no pointer ever changes.  The
 * layout is compact for the K' of the last gradient query (0 before the first) and the Q in force, and `bytes` reports that.  After
 * rr_set_distance_pairs the buffers hold unspecified data until the next query.  STREAM CONTRACT for readers as for the sibling views.
 * Out of scope: gradients with respect to object poses; per-pair gradients at postures (600 MB at 4096 x 32 x 96: narrow the table
 * instead); second derivatives; a switch of the vector env; any use by the step. */
int rr_signed_gradient(rr_env *env, const float *postures /* f32 [N][K][11] or NULL */, int32_t n_postures, int32_t on_device, float margin);
/* Zero-copy device pointer + size in bytes of an RR_SG_* buffer (read-only for the caller); which outside [0, RR_SG_COUNT): RR_EINVAL. */
int rr_signed_gradient_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_SG_* buffer (its `bytes`) to host memory. */
int rr_signed_gradient_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Swept clearance along joint-space segments on the device (additive in ABI 7) ------------------------------------------------------
 * The queries above answer a question about a POSTURE; a planner's unit of work is an EDGE: "is the motion from q0 to q1 free, and
 * if not, where does it first touch and what?"  Sampling the edge proves nothing -- an arm passes through the shelf lip between two
 * free samples -- and costs 32 x Q pair searches whether the edge is near anything or not.  rr_swept_clearance decides K segments
 * per env of the whole batch by CONSERVATIVE ADVANCEMENT in one launch on the library's stream: it needs only the proved lower bound
 * of a pair's distance (the `lower` column of RR_DIST_POINTS) and a bound on how fast that distance can change, which for eleven
 * revolute joints is a constant table.  The buffers are NOT fields of rr_get_buffer and not buffers of the queries above: they have
 * this enum and rr_sweep_buffer. */
enum {
    RR_SW_STOP = 0,   /* f32 [N, K, 12] {fraction, q_stop[0..10]}: q_stop is the posture the kernel evaluated last */
    RR_SW_HIT = 1,    /* f32 [N, K, 12] the RR_DIST_POINTS row of the reported pair at q_stop; all +0.0 at status 0 */
    RR_SW_ID = 2,     /* i32 [N, K, 4]  {status, reported pair (-1 at status 0), steps, pair evaluations} */
    RR_SW_FREE = 3,   /* f32 [N, K, Q]  min(free_j, 1): every pair's proved free horizon at the end */
    RR_SW_COUNT = 4
};
#define RR_SW_MAX_STEPS 64
/* Input.  segments is f32 [N][K][2][11], C order, K = n_segments in [1, RR_PC_MAX_POSTURES]: the start posture q0 and the end
 * posture q1 of K independent segments per env, the eleven joints in the order of rr_posture_clearance.  The motion is
 * q(t) = q0 + t (q1 - q0), t in [0, 1]; the objects stay at env e's PRESENT pose; the pair table and the cull are those of
 * rr_set_distance_pairs.  on_device means what it means to rr_posture_clearance: device memory read in place on the library's stream
 * under that call's STREAM CONTRACT, without waiting, or host memory staged through a buffer of the handle's own (N * 32 * 22 floats,
 * allocated by the first such call), and the call waits.  Values are not validated.
 * The reach table.  R[k][s], built on the host in float64 when the handle is made and rounded UP to float32: for a robot shape s on
 * body b with joint k an ancestor-or-self of b, |sphere centre of s| + sphere radius of s + the sum of |body_jpos[m]| over the
 * bodies m on the chain from b up to, but not including, k; otherwise 0.  It bounds the distance of every point of s from joint k's
 * origin at any posture.  rr_sweep_reach returns it.
 * The pair bound.  B_j = sum of |q1_k - q0_k| (R[k][a] + R[k][b]) over the joints k that are an ancestor-or-self of the body of
 * exactly one of the two shapes (a joint above both moves them rigidly and changes no distance; statics and objects have no
 * joints): the distance of pair j is B_j-Lipschitz in t.  Summed in float32 over ascending k and scaled by 1 + 2^-20.
 * The advancement.  One common t per segment, from 0; every pair carries a horizon free_j, from 0.  A step evaluates the pairs with
 * free_j <= t at q(t) = fma(t, q1 - q0, q0) with the device text of rr_closest_points and rr_posture_clearance.  With
 * g = lower_j - safety: unless g > tolerance the pair HITS (so does a NaN); otherwise free_j = t + g / B_j, or +inf when B_j == 0.
 * If a pair hits, the row stops at this t and the lowest pair index among the hits is reported.  Otherwise t = min_j free_j (the
 * first minimum: the lowest index among equals); at or beyond 1 the row is free.  Every step advances t by more than
 * tolerance / max B.  At most RR_SW_MAX_STEPS postures are evaluated whatever the data, non-finite input included: a non-finite row
 * leaves the loop within the cap, its outputs unspecified, with status in {0, 1, 3}.
 * Status.  0: free, fraction = 1.0 exactly.  1: hit, fraction = the t of the stop; 0 for a segment that starts within
 * safety + tolerance.  3: step cap, fraction = the t reached: a proved free prefix, and the caller continues from q_stop; RR_SW_HIT
 * then holds the pair with the smallest horizon (the lowest index among equals), evaluated at q_stop.  `steps` counts the postures
 * evaluated, `pair evaluations` the pair searches of those steps (the one search that writes RR_SW_HIT of a stopped row is not
 * counted).
 * Guarantees.  For every pair j and every t < min(free_j, 1) the distance of pair j along the motion exceeds safety; for every
 * t < fraction every pair's distance exceeds safety.  A pair that is never evaluated again keeps the horizon of its last evaluation;
 * a pair that hits keeps the horizon it had.  (A culled pair's lower bound is its sphere gap, which is a lower bound too.)
 * No effect on the simulation: the call reads what rr_posture_clearance reads, and the reach table, and writes these four buffers
 * only; the next step stays prepared.  No atomics and a fixed reduction order: row (e, k) is a function of (env e's objects, segment
 * (e, k), the tables, safety, tolerance) alone.  No value of the tensor or the state forms an address.
 * Errors: RR_EINVAL with nothing allocated and nothing changed, the message naming the cause, for a null env, null segments,
 * n_segments outside [1, RR_PC_MAX_POSTURES], Q == 0, safety < 0 or NaN or infinite, tolerance < 1e-6 or NaN or infinite, and a cull
 * in force (0 < max_distance < inf) with max_distance < safety + tolerance: a culled pair's sphere gap could otherwise fake a hit.
 * Buffers.  All four are allocated on first use -- by this call, or by rr_sweep_buffer / rr_sweep_copy_to_host --, all or nothing
 * through the handle's memory owner, zero-filled, sized once for RR_PC_MAX_POSTURES x RR_DIST_MAX, and valid until rr_destroy: no
 * pointer ever changes.  The layout is compact for the K of the last query (0 before the first) and the Q in force, and `bytes`
 * reports that.  After rr_set_distance_pairs the buffers hold unspecified data until the next query.  STREAM CONTRACT for readers as
 * for the sibling views.
 * Out of scope: objects that move during the sweep; every pair's first hit (the earliest alone is reported); gradients of the hit
 * time; polylines as a type (stack the waypoints into segments); Cartesian segments; a switch of the vector env; any use by the step. */
int rr_swept_clearance(rr_env *env, const float *segments /* f32 [N][K][2][11] */, int32_t n_segments, int32_t on_device, float safety, float tolerance);
/* The reach table R[k][s] of the handle's model, f32 [11][n_shapes] (n_shapes: the model's collision shapes, the index space of
 * rr_set_distance_pairs), to host memory.  Null env or null out: RR_EINVAL. */
int rr_sweep_reach(rr_env *env, float *out /* f32 [11][n_shapes] */);
/* Zero-copy device pointer + size in bytes of an RR_SW_* buffer (read-only for the caller); which outside [0, RR_SW_COUNT): RR_EINVAL. */
int rr_sweep_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_SW_* buffer (its `bytes`) to host memory. */
int rr_sweep_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Kinematics at candidate joint postures on the device (additive in ABI 7) ----------------------------------------------------------
 * The queries above answer for the COLLISION side of K candidate postures per env; the other half of a sampler's or optimiser's
 * objective is "where would the tool be at these postures, and what is the Jacobian there?".  rr_kinematic_observations gives link
 * poses and Jacobians at the PRESENT state only.  One launch on the library's stream (rr_posture_kinematics) evaluates K candidate
 * postures per env of the whole batch and writes three device buffers.  The same [N, K, 11] tensor feeds rr_posture_kinematics (the
 * task cost and its Jacobian), rr_signed_gradient (the collision cost and its gradient) and rr_swept_clearance (the edge check).  The
 * buffers are NOT fields of rr_get_buffer and not RR_KIN_* or RR_PC_* buffers (RR_F_COUNT stays 16, RR_KIN_COUNT 7, RR_PC_COUNT 4):
 * they have this enum and rr_posture_kinematics_buffer. */
enum {
    RR_PK_LINK_POSE = 0,  /* f32 [N, K, 17, 7]     the RR_KIN_LINK_POSE row (COM frame, xyz + xyzw) of every URDF link at posture (e, k) */
    RR_PK_POINT_POS = 1,  /* f32 [N, K, P, 3]      world position of every kinematic point in force                                     */
    RR_PK_JACOBIAN = 2,   /* f32 [N, K, P, 6, 11]  the RR_KIN_JACOBIAN block of every point: rows linear xyz, angular xyz; columns q[11]  */
    RR_PK_COUNT = 3
};
/* Input.  postures, n_postures (K in [1, RR_PC_MAX_POSTURES]) and on_device mean exactly what they mean to rr_posture_clearance:
 * f32 [N][K][11], C order, the eleven INDEPENDENT joints in the order of the state's q[11].  on_device != 0: device memory, read IN
 * PLACE on the library's stream under that call's STREAM CONTRACT (produced on that stream or ordered before it; not rewritten before
 * later work on that stream); the call allocates nothing beyond the first-use buffers, checks the launch and returns without waiting.
 * on_device == 0: host memory, staged through the posture staging buffer of rr_posture_clearance (the handle's own, allocated by the
 * first host-path call of any posture query), and the call waits for the stream.  Values are NOT validated and NOT clamped to the
 * joint limits: the posture is evaluated as given.  The points are those of rr_set_kinematic_points: the P in force, on a fresh
 * handle the gripper base.
 * What is computed.  Row (e, k) is what rr_kinematic_observations would write into RR_KIN_LINK_POSE, RR_KIN_POINT_POS and
 * RR_KIN_JACOBIAN for env e if columns 0..10 of its RR_F_STATE row were postures[e][k][0..10]: the frames of the step's own forward
 * kinematics, in its operation order; the link expression of rr_link_poses; column k of a point's Jacobian is [a_k x (x - p_k); a_k]
 * if joint k moves the point's link and +0.0 in all six rows otherwise (the block above has the symbols and the map from the nine
 * command entries).  For a candidate equal to env e's present joints the three rows are those buffers BIT FOR BIT.  The velocity
 * fields of rr_kinematic_observations have no counterpart here: a candidate has no joint velocity.
 * A row is a function of (posture (e, k), the model, the points) ALONE.  It is independent of env e's state -- joints, objects, error
 * flags: N is the batch shape this query shares with its siblings, not an input.
 * No effect on the simulation.  The call reads the tensor, the model and the points, and writes these three buffers only: not the
 * state, not the preparation record (RR_F_PREP), no error flag, no RR_KIN_* buffer and no buffer of another query.  The next step
 * stays prepared and no later step is affected.  The buffers hold what the LAST CALL computed.
 * Every loop bound is a constant or a model count, and no value of the tensor ever forms an address: a non-finite posture finishes
 * like any other and its rows are unspecified.
 * Determinism.  No atomics: row (e, k) is identical from call to call, independent of N, of K, of the row's place and of its
 * neighbours.
 * Errors: RR_EINVAL with nothing allocated and nothing changed, the message naming the function and the cause, for a null env, null
 * postures, n_postures outside [1, RR_PC_MAX_POSTURES], and a model that rr_kinematic_observations refuses (not the 17 URDF links of
 * rr_link_poses, or a link on a body outside the kinematic tree).
 * Buffers.  All three are allocated on first use -- by this call, or by rr_posture_kinematics_buffer /
 * rr_posture_kinematics_copy_to_host --, all or nothing through the handle's memory owner, zero-filled, sized once for
 * RR_PC_MAX_POSTURES x RR_KIN_MAX_POINTS -- N x 85 888 bytes: 352 MB at 4096 envs --, and valid until rr_destroy:
 * no pointer ever changes.  The layout is compact for the K of the last query (0 before the first) and the P in force, and `bytes`
 * reports that.
 * After rr_set_kinematic_points the buffers hold unspecified data until the next query (a query enqueued before the change keeps the
 * points it was launched with).  STREAM CONTRACT for readers as for the other zero-copy views: the kernel runs on the library's stream
 * behind the work enqueued before it; readers on another stream order themselves after the call (event / rr_sync), and a later call
 * rewrites the buffers in place.
 * Out of scope: velocities (a candidate has none); candidate object poses; Jacobians of all 17 links (put points on the links that
 * matter); a switch of the vector env (postures are an argument, not an observation); ray casts at candidate postures; any use by
 * the step. */
int rr_posture_kinematics(rr_env *env, const float *postures /* f32 [N][K][11] */, int32_t n_postures, int32_t on_device);
/* Zero-copy device pointer + size in bytes of an RR_PK_* buffer (read-only for the caller); which outside [0, RR_PK_COUNT): RR_EINVAL. */
int rr_posture_kinematics_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_PK_* buffer (its `bytes`) to host memory. */
int rr_posture_kinematics_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Inverse kinematics at candidate targets on the device (additive in ABI 7) ---------------------------------------------------------
 * Every posture query above starts from joint postures [N, K, 11]; a user starts from tool poses: grasp candidates, pre-grasp poses,
 * via points, the cartesian samples of a CEM.  rr_ik below solves one target per env, for link 7 only, from the env's present joints,
 * through host arrays.  One launch on the library's stream (rr_posture_ik) solves K target poses per env of the whole batch, each from
 * a seed of its own, and writes three device buffers; RR_PIK_POSTURE is the [N, K, 11] tensor that rr_posture_clearance,
 * rr_signed_distance, rr_signed_gradient and rr_posture_kinematics read IN PLACE.  The buffers are NOT fields of rr_get_buffer and
 * not RR_PK_* or RR_PC_* buffers (RR_F_COUNT stays 16, RR_KIN_COUNT 7, RR_PC_COUNT 4, RR_PK_COUNT 3): they have this enum and
 * rr_posture_ik_buffer. */
#define RR_PIK_MAX_ITERATIONS 256
enum { RR_PIK_POSITION_ONLY = 1u, RR_PIK_CLAMP_LIMITS = 2u };   /* flags */
typedef struct rr_ik_options {
    int32_t point;           /* index into the points of rr_set_kinematic_points, [0, P)   default 0 */
    int32_t max_iterations;  /* [1, RR_PIK_MAX_ITERATIONS]                                  default 32 */
    float tolerance;         /* residual below which a row has converged, > 0, finite       default 1e-3 */
    float damping;           /* lambda of J^T (J J^T + lambda^2 I)^-1 e, > 0, finite        default 0.1 (rr_ik's) */
    float max_step;          /* cap on |dq|_inf per update, > 0, finite                     default 0.5 (rr_ik's) */
    uint32_t flags;          /* default RR_PIK_CLAMP_LIMITS */
} rr_ik_options;
enum { RR_PIK_POSTURE = 0,  /* f32 [N, K, 11]  the solution; feeds every posture query in place */
       RR_PIK_RESULT = 1,   /* f32 [N, K, 4]   {residual, position error (m), orientation error angle (rad), +0.0} */
       RR_PIK_INFO = 2,     /* i32 [N, K, 2]   {status, iterations} */
       RR_PIK_COUNT = 3 };
/* Target.  targets[e][k] is the world pose of the tool frame: xyz, then an xyzw quaternion, which the call normalises (as rr_ik does).
 * Tool frame.  Point opt->point of rr_set_kinematic_points: its position is the point's world position, its orientation the
 * orientation of the point's link COM frame -- exactly what rr_posture_kinematics reports as point_pos and as the quaternion of
 * link_pose[link].  Point 0 of a fresh handle is the gripper base: the frame rr_ik solves for.
 * Seed.  Row (e, k) starts from seeds[e][k] (f32 [N][K][11], the state's q[11]); with seeds == NULL from columns 0..10 of env e's
 * present state row, which the call READS and never writes.  on_device covers BOTH tensors and has the STREAM CONTRACT of
 * rr_posture_clearance: device memory read in place on the library's stream, no wait; on_device == 0: host memory -- the seeds are
 * staged through the posture staging buffer of rr_posture_clearance, the targets through a staging buffer [N, 32, 7] of their own
 * (allocated through the handle's memory owner with whatever else the call still needs, all or nothing) -- and the call waits.
 * Unknowns.  The seven arm joints.  Joints 7..10 (the fingers) are copied from the seed to the output unchanged; they may still
 * place the tool, a point on a finger link being legal.  An arm joint that does not move the point's link (a point on link_3 has
 * four) has a zero Jacobian column and keeps its seed value.
 * Residual (rr_ik's): e_p = target - x; w = half the antisymmetric part of Rt Re^T (sin(angle) x axis of the orientation error);
 * residual = |(e_p, w)|.  With RR_PIK_POSITION_ONLY residual = |e_p|, the system is 3 x 3 and the target quaternion is ignored by
 * the solve.  The RR_PIK_RESULT row always carries |e_p|, and the TRUE angle atan2(|w|, (trace(Rt Re^T) - 1) / 2) against the
 * given quaternion, so a caller can see an aliased orientation (in position-only mode it is informational, and NaN for a quaternion
 * that cannot be normalised).
 * Update (rr_ik's): dq = J^T (J J^T + lambda^2 I)^-1 e by Cholesky, scaled so that |dq|_inf <= max_step.  With RR_PIK_CLAMP_LIMITS
 * the seed's arm joints are first clamped into the model's body_limits and every iterate is clamped too: every returned arm joint
 * lies within its limits.  Without it every iterate is wrapped to (-pi, pi], as rr_ik does (a seed that needs no update is
 * returned as given).
 * Stop and status.  The residual is evaluated before each update and once more after the last; `iterations` is the number of
 * updates applied, 0 .. max_iterations.  status 0: converged -- residual < tolerance and, in full-pose mode,
 * (trace(Rt Re^T) - 1) / 2 > 0 (w vanishes at a half-turn too: stopping there would be a false success; such a row runs to the cap).
 * status 1: the iteration cap; the row holds the last iterate and its residual.  status 2: the residual is not finite (a non-finite
 * target or seed, a zero quaternion); the row's other values are unspecified.
 * Independence and determinism.  Row (e, k) is a function of (its target, its seed, the options, the model, the points) ALONE and
 * identical from call to call: independent of N, of K, of the row's place and of its neighbours; with seeds == NULL env e's joints
 * enter as the seed and in no other way.  No atomics.
 * Safety.  Every loop bound is a constant, a model count or max_iterations, and no value of a tensor ever forms an address.
 * No effect on the simulation.  The call writes these three buffers and nothing else: not the state, not the preparation record
 * (RR_F_PREP), no error flag, not the plan and IK buffers of rr_ik / rr_plan_macro, no buffer of another query.  The next step
 * stays prepared.  The buffers hold what the LAST CALL computed.
 * Cost.  One lane per row; a wave of 64 rows runs as long as its slowest row, so a few rows at the cap keep most waves for
 * max_iterations updates.
 * Errors: RR_EINVAL with nothing allocated and nothing changed, the message naming the function and the cause, for a null env, null
 * targets, n_targets outside [1, RR_PC_MAX_POSTURES], point outside [0, P), max_iterations outside [1, RR_PIK_MAX_ITERATIONS], a
 * tolerance, damping or max_step that is not finite or not > 0, an unknown flag bit, and a model that rr_kinematic_observations
 * refuses.  opt == NULL: the defaults.
 * Buffers.  All three are allocated on first use -- by this call, or by rr_posture_ik_buffer / rr_posture_ik_copy_to_host --, all
 * or nothing through the handle's memory owner, zero-filled, sized once for RR_PC_MAX_POSTURES -- N x 2 176 bytes --, and valid until
 * rr_destroy: no pointer ever changes.  The layout is compact for the K of the last call (0 before the first), and `bytes` reports
 * that.  STREAM CONTRACT for readers as for the other zero-copy views: a posture query enqueued behind this call on the library's
 * stream reads RR_PIK_POSTURE in order; readers on another stream order themselves after the call (event / rr_sync), and a later
 * call rewrites the buffers in place.
 * Out of scope: any use by the step (cartesian actions); null-space objectives; collision-aware IK (compose the posture with
 * rr_signed_gradient); random restarts inside the call (give several rows the same target with different seeds); a switch of the
 * vector env; any change to rr_ik, rr_plan_macro or the ik_single_seed option. */
int rr_posture_ik(rr_env *env, const float *targets /* f32 [N][K][7] */, const float *seeds /* f32 [N][K][11] or NULL */,
                  int32_t n_targets, int32_t on_device, const rr_ik_options *opt /* NULL: the defaults */);
/* Zero-copy device pointer + size in bytes of an RR_PIK_* buffer (read-only for the caller); which outside [0, RR_PIK_COUNT): RR_EINVAL. */
int rr_posture_ik_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_PIK_* buffer (its `bytes`) to host memory. */
int rr_posture_ik_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Joint-space dynamics at candidate joint postures on the device (additive in ABI 7) ------------------------------------------------
 * The posture queries above answer every kinematic and geometric question about K candidate postures per env; this one answers the
 * dynamic one: what does it cost to hold or move the arm there?  One launch on the library's stream (rr_posture_dynamics) evaluates
 * K rows per env of the whole batch -- a posture q, a joint velocity qd and a joint acceleration qdd each -- and writes the mass
 * matrix M(q), the gravity torques G(q), the bias G(q) + C(q, qd), the inverse dynamics M qdd + C + G and, on request, M^-1:
 * pybullet's calculateMassMatrix and calculateInverseDynamics for every row at once.  A trajectory optimiser's effort cost and
 * torque limits, a gravity-compensated or computed-torque controller and an operational-space controller (M^-1 beside the Jacobian
 * of rr_posture_kinematics) read them in place.  The buffers are NOT fields of rr_get_buffer and not buffers of another query: they
 * have this enum and rr_posture_dynamics_buffer. */
enum {
    RR_PD_MASS_MATRIX = 0,   /* f32 [N, K, 11, 11]  M(q) over the eleven independent joints, in the order of the state's q[11]       */
    RR_PD_GRAVITY = 1,       /* f32 [N, K, 11]      G(q): the joint torques that hold the posture still                            */
    RR_PD_BIAS = 2,          /* f32 [N, K, 11]      G(q) + C(q, qd): calculateInverseDynamics at zero acceleration                 */
    RR_PD_TORQUE = 3,        /* f32 [N, K, 11]      M qdd + bias: calculateInverseDynamics                                         */
    RR_PD_MASS_INVERSE = 4,  /* f32 [N, K, 11, 11]  M^-1; written only with RR_PD_INVERSE                                          */
    RR_PD_COUNT = 5
};
enum { RR_PD_INVERSE = 1u };   /* flags */
/* Input.  Three tensors f32 [N][K][11], C order, K = n_postures in [1, RR_PC_MAX_POSTURES], over the eleven INDEPENDENT joints in
 * the order of the state's q[11]: postures (rad), velocities (rad/s), accelerations (rad/s^2).
 *   velocities == NULL: qd = 0, and RR_PD_BIAS holds the same bytes as RR_PD_GRAVITY.
 *   accelerations == NULL: qdd = 0, and RR_PD_TORQUE holds the same bytes as RR_PD_BIAS.
 *   postures == NULL: the PRESENT-STATE form.  K = 1 (n_postures must be 1), q and qd are the joint columns of env e's RR_F_STATE
 *     row, read and never written; velocities must then be NULL too; accelerations may be given as [N][1][11].
 * on_device != 0: every tensor given is device memory, read IN PLACE on the library's stream under the STREAM CONTRACT of
 * rr_posture_clearance (produced on that stream or ordered before it; not rewritten before later work on that stream); the call
 * allocates nothing beyond the first-use buffers, checks the launch and returns without waiting.  on_device == 0: every tensor given
 * is host memory, staged through the posture staging blocks (the handle's own, allocated by the first host-path call that needs
 * them), and the call waits for the stream.  There is one flag for the whole set: a mixed set cannot be expressed, and the Python
 * layer refuses one.  Values are NOT validated and NOT clamped to the joint limits: a row is evaluated as given.
 * flags: RR_PD_INVERSE also writes RR_PD_MASS_INVERSE; without it that buffer is left as it was.  Other bits: RR_EINVAL.
 * What is computed.  The rigid-body dynamics of the eleven moving bodies of the arm and gripper, tau = M(q) qdd + C(q, qd) + G(q):
 * forward kinematics (the step's frames), the composite-body pass for M, one recursive Newton-Euler pass at qd = 0 for G and one at
 * qd for the bias, M qdd added to the bias, the Cholesky factor and its inverse for M^-1 -- the arithmetic of the step's
 * preparation, in float32 with contracted multiply-adds and 1-ulp reciprocal square roots on the Cholesky diagonal.
 *   The link masses and inertias are the HANDLE'S OWN: the body table the step's preparation reads, so a handle created with
 *     use_urdf_inertia answers with those inertias.
 *   Gravity is the step's (9.81 m/s^2 along -z).
 *   Joint damping and the motors are NOT part of any output -- as in pybullet, where joint damping (rr_set_env_actuators) is a force
 *     the step adds.
 *   M is computed for one triangle and mirrored: symmetric BIT FOR BIT.  An entry between joints of which neither moves the other's
 *     body (the two finger branches: joints {7, 8} against {9, 10}) is exactly +0.0.
 * A row is a function of its three input rows and the model ALONE.  It is independent of env e's state, of the object dynamics and
 * of the actuators: N is the batch shape this query shares with its siblings, not an input (the present-state form reads the joint
 * columns of the state as its input rows and nothing else of it).
 * No effect on the simulation.  The call writes these buffers only: not the state, not the preparation record (RR_F_PREP), no error
 * flag and no buffer of another query.  The look-ahead stays valid and the next step is bit for bit what it would have been.  The
 * buffers hold what the LAST CALL computed.
 * Every loop bound is a constant or the row count, and no value of the tensors ever forms an address: a non-finite row finishes like
 * any other, its outputs are non-finite, and no other row is affected.
 * Determinism.  No atomics: a row is identical from call to call, independent of N, of K, of the row's place and of its neighbours.
 * Errors: RR_EINVAL with nothing allocated and nothing changed, the message naming the function and the cause, for a null env,
 * n_postures outside [1, RR_PC_MAX_POSTURES], postures == NULL with velocities given or with n_postures != 1, and unknown flag bits.
 * Buffers.  All five are allocated on first use -- by this call, or by rr_posture_dynamics_buffer /
 * rr_posture_dynamics_copy_to_host --, all or nothing through the handle's memory owner, zero-filled, sized once for
 * RR_PC_MAX_POSTURES -- N x 35 200 bytes: 144 MB at 4096 envs --, and valid until rr_destroy: no pointer ever changes.  The layout is
 * compact for the K of the last call (0 before the first), and `bytes` reports that.  STREAM CONTRACT for readers as for the other
 * zero-copy views: the kernel runs on the library's stream behind the work enqueued before it; readers on another stream order
 * themselves after the call (event / rr_sync), and a later call rewrites the buffers in place.
 * Applying such torques is rr_set_joint_torques (below).  Out of scope: joint damping or motor terms; the operational-space inertia itself (form
 * (J M^-1 J^T)^-1 from this query and rr_posture_kinematics); derivatives of the dynamics. */
int rr_posture_dynamics(rr_env *env, const float *postures /* f32 [N][K][11] or NULL */, const float *velocities /* f32 [N][K][11] or NULL */,
                        const float *accelerations /* f32 [N][K][11] or NULL */, int32_t n_postures, int32_t on_device, uint32_t flags);
/* Zero-copy device pointer + size in bytes of an RR_PD_* buffer (read-only for the caller); which outside [0, RR_PD_COUNT): RR_EINVAL. */
int rr_posture_dynamics_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_PD_* buffer (its `bytes`) to host memory. */
int rr_posture_dynamics_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* ---- Joint torque inputs of the step: feed-forward and torque control (additive in ABI 7) ---------------------------------------------
 * rr_posture_dynamics computes joint torques; this applies them: pybullet's setJointMotorControl2(TORQUE_CONTROL, force=tau), the
 * actuation-force tensor of batched simulators.  The handle holds a table tau f32 [N][11] over the eleven INDEPENDENT joints in the
 * order of the state's q[11] (N m), all zero on a fresh handle.  EVERY rr_step uses the table in force -- each inner step of the
 * macro and episode entry points that call rr_step included -- and solves with
 *     qd*' = qd* + dt M^-1 tau
 * where qd* = qd + dt M^-1 (-bias - damping qd) and M^-1 are the values of the env's preparation record (RR_F_PREP) for this step.
 * Motor rows, limit rows and contacts act on top, exactly as without torques.  Three uses:
 *   max_force = 0 on a joint (rr_set_env_actuators) plus tau   torque control of that joint;
 *   default motors plus tau                                    feed-forward under the position motor;
 *   tau = RR_PD_BIAS of rr_posture_dynamics' present-state form  holds the arm against gravity (and the velocity terms).
 * Joint damping is NOT compensated: it remains in qd*.  Values are NOT clamped: no torque limit, no saturation model.
 * PERSISTENT, unlike pybullet: nothing clears the table after a step.  It holds until the next rr_set_joint_torques, like the motor
 * targets.  A command-side setting that stays with its env: rr_reset, an episode's auto-reset, rr_write_state, rr_set_state,
 * rr_copy_envs (forks, snapshot saves and loads) and rr_checkpoint_restore keep the table as it is, and neither a snapshot nor a
 * checkpoint carries it.
 * The zero-row rule.  An env whose row is all zero (either sign) is NOT TOUCHED by the step: its qd* keeps its bits, so a masked or
 * partly zero table leaves those envs bit for bit as without the feature.  A frozen env (error flag bit 0) is not touched either.
 * With no torque set at all -- a fresh handle, or after the clearing call below -- the step launches exactly the kernels it launched
 * before this entry point existed.
 * rr_set_joint_torques copies the rows of the masked envs (env_mask u8 [N], NULL: all envs) from `torques` f32 [N][11], C order, into
 * the table with one launch on the library's stream.
 *   torques_on_device != 0: device memory, read IN PLACE on the library's stream under the STREAM CONTRACT of rr_write_state (produced
 *     on that stream or ordered before it; not rewritten before later work on that stream); NOT validated; the call returns without
 *     waiting.  torques_on_device == 0: host memory; the masked rows are checked for finiteness -- a non-finite value is RR_EINVAL and
 *     the call changes NOTHING --, then staged, and the call waits for the stream.
 *   mask_on_device says the same of env_mask.  With both given they must live on the same side: a mixed pair is RR_EINVAL.
 *   torques == NULL zeroes the masked rows.  torques == NULL and env_mask == NULL zeroes the table and turns the feature OFF: the
 *     steps launch no torque kernel until the next call with a table.  (From the first successful call with a table until then every
 *     step launches it, whatever the values: rows that happen to be zero are found by the kernel's own test.)
 * The look-ahead stays valid: the call touches neither the state nor the preparation record, and the step applies the table BEHIND
 * the preparation, so a controller that sets new torques every step keeps the overlap of step t with the preparation of step t + 1.
 * For users who think in the NINE entries of a joint command (dq = Q dcmd with the [11][9] matrix of rr_kinematic_observations: entry
 * 7 drives q[7] and q[9], entry 8 drives -q[8] and -q[10]): tau11 = Q tau9 applies entry 7 to both of its joints and minus entry 8
 * to both of its; the generalised force on a command coordinate is Q^T tau11.
 * Errors: RR_EINVAL for a null env, a mixed pair, a non-finite host row; RR_EDEVICE for a failed allocation (all or nothing through
 * the handle's memory owner; the table, N x 44 bytes, zero-filled, on first use -- by this call with a table, rr_get_joint_torques or
 * rr_joint_torque_buffer) or a device error.
 * Wrenches on robot bodies and objects are rr_set_external_wrenches (below).  Out of scope: torque limits and saturation; compensation of joint damping; the table in forks, snapshots and
 * checkpoints; a controller library. */
int rr_set_joint_torques(rr_env *env, const float *torques /* f32 [N][11] or NULL */, int32_t torques_on_device, const uint8_t *env_mask /* u8 [N] or NULL */,
                         int32_t mask_on_device);
/* Synchronising copy of the table in force, f32 [N][11], to host memory. */
int rr_get_joint_torques(rr_env *env, float *out_host);
/* Zero-copy device pointer + size in bytes (N x 44) of the table: valid until rr_destroy, the pointer never changes.  A caller may
 * WRITE it in stream order (on the library's stream or ordered before later work on it): the next step uses what it finds --
 * provided the feature is on (a successful rr_set_joint_torques with a table since the last clearing call). */
int rr_joint_torque_buffer(rr_env *env, void **dev_ptr, size_t *bytes);

/* ---- External wrenches on robot bodies and objects in the step (additive in ABI 7) ---------------------------------------------------
 * pybullet's applyExternalForce / applyExternalTorque, the rigid-body force tensor of batched simulators: push an object, disturb the
 * arm, cancel a weight, model a payload on the gripper, feed a learned residual force.  The handle holds a table w f32
 * [N][RR_XW_BODIES][6], all zero on a fresh handle:
 *   rows 0..10   the eleven moving robot bodies; row j is the rigid body that joint j of the state's q[11] moves (the bodies of the
 *                preparation record, RR_F_PREP);
 *   rows 11..13  objects 0..2.  The step never reads the rows of objects the handle does not have; they are stored and read back as
 *                given.
 * A row is {Fx, Fy, Fz, Tx, Ty, Tz} in the WORLD frame (N, N m).  The force acts at the body's CENTRE OF MASS, the torque is about that
 * centre: for a robot body c_b = p_b + R_b com_b (the centre the mass matrix uses, body_com of the model), for an object the position
 * of its state.  EVERY rr_step uses the table in force -- each inner step of the macro and episode entry points that call rr_step
 * included -- and adds, behind the preparation and in front of the solve,
 *     object i:  v*' = v* + dt F / m_i      w*' = w* + dt Iinv_i T
 *     robot:     tau_k = sum over the bodies b that joint k moves of a_k . ((c_b - p_k) x F_b + T_b)      qd*' = qd* + dt M^-1 tau
 * with m_i the ENV's own mass (rr_set_object_dynamics), Iinv_i the world inverse inertia of the pose that counts -- for an object the
 * out-of-bounds rule sends home that is the HOME pose, and the wrench acts on it there --, a_k, p_k the world axis and origin of joint
 * k, and M^-1, qd*, v*, w* the values of the env's preparation record (RR_F_PREP) for this step.  Contacts, motor rows and limit rows
 * act on top, exactly as without wrenches.  Values are NOT clamped.  With joint torques (rr_set_joint_torques) also on, the torque
 * term is added first, then the wrench term.
 * A force at a point, or in a body frame: compose it in torch -- T += r x F for a force at c + r, F_world = R F_body with R from the
 * link poses of rr_kinematic_observations / the object poses -- and write the buffer; the kernel knows world-frame wrenches at the
 * centre of mass only.
 * PERSISTENT, unlike pybullet (whose external forces last one step): nothing clears the table after a step.  It holds until the next
 * rr_set_external_wrenches, like the joint torque table.  rr_reset, an episode's auto-reset, rr_write_state, rr_set_state, rr_copy_envs
 * (forks, snapshot saves and loads) and rr_checkpoint_restore keep the table as it is, and neither a snapshot nor a checkpoint
 * carries it.
 * The zero rule, PER TARGET.  With all eleven robot rows of an env zero (either sign) its qd* keeps its bits; an object whose row is
 * zero keeps the bits of its v* and w*: such targets are NOT TOUCHED, bit for bit as without the feature.  A frozen env (error flag
 * bit 0) is not touched.  A NaN counts as non-zero.  With no wrench set at all -- a fresh handle, or after the clearing call below --
 * the step launches exactly the kernels it launched before this entry point existed.
 * rr_set_external_wrenches copies the rows of the masked envs (env_mask u8 [N], NULL: all envs) from `wrenches` f32 [N][14][6], C
 * order, into the table with one launch on the library's stream.  The contract of rr_set_joint_torques, point for point:
 *   wrenches_on_device != 0: device memory, read IN PLACE on the library's stream under the STREAM CONTRACT of rr_write_state; NOT
 *     validated; the call returns without waiting.  wrenches_on_device == 0: host memory; the masked envs' rows are checked for
 *     finiteness -- a non-finite value is RR_EINVAL naming env, row and entry, and the call changes NOTHING --, then staged, and the
 *     call waits for the stream.
 *   mask_on_device says the same of env_mask.  With both given they must live on the same side: a mixed pair is RR_EINVAL.
 *   wrenches == NULL zeroes the masked rows.  wrenches == NULL and env_mask == NULL zeroes the table and turns the feature OFF.
 *     Zeroing a table that was never allocated is RR_OK with nothing allocated.
 * The look-ahead stays valid: the call touches neither the state nor the preparation record.
 * Errors: RR_EINVAL for a null env, a mixed pair, a non-finite host row; RR_EDEVICE for a failed allocation (all or nothing through
 * the handle's memory owner; the table, N x 336 bytes, zero-filled, on first use -- by this call with a table,
 * rr_get_external_wrenches or rr_external_wrench_buffer) or a device error.
 * Out of scope: body-frame wrenches and application points inside the kernel; timed or one-shot wrenches that clear themselves;
 * wrenches on the static scene; force limits; the table in forks, snapshots and checkpoints. */
#define RR_XW_BODIES 14
int rr_set_external_wrenches(rr_env *env, const float *wrenches /* f32 [N][14][6] or NULL */, int32_t wrenches_on_device,
                             const uint8_t *env_mask /* u8 [N] or NULL */, int32_t mask_on_device);
/* Synchronising copy of the table in force, f32 [N][14][6], to host memory. */
int rr_get_external_wrenches(rr_env *env, float *out_host);
/* Zero-copy device pointer + size in bytes (N x 336) of the table: valid until rr_destroy, the pointer never changes.  A caller may
 * WRITE it in stream order (on the library's stream or ordered before later work on it): the next step uses what it finds --
 * provided the feature is on (a successful rr_set_external_wrenches with a table since the last clearing call). */
int rr_external_wrench_buffer(rr_env *env, void **dev_ptr, size_t *bytes);

/* Carried objects in the posture queries: objects attached to robot links (additive in ABI 7; the <true> instantiations of
 * k_posture_clearance, k_signed_distance and k_signed_gradient; k_attach_capture: csrc/rr_carry.inc).  What planners call an ATTACHED body: once
 * the gripper holds the cube, a candidate posture must move the cube with the hand, or the (finger, cube) pairs report the arm's
 * motion against a stationary cube and the (cube, shelf) / (cube, table) pairs never change.  It replaces the write-and-query loop --
 * rr_write_state of the composed object pose per candidate, then a present-state query -- that rr_posture_clearance was added to
 * retire.
 * A QUERY-SIDE SETTING of the handle, like the pair table and the kinematic points: NOT a constraint of the simulation (pybullet's
 * createConstraint is out of scope), no step reads it, and the state, the preparation record and the look-ahead are never touched.
 * The table says, per (env, object), the URDF link the object is rigid with -- link[e][o] in [0, 17), the order of rr_link_poses and
 * rr_set_kinematic_points, or -1: FREE -- and rel_pose[e][o], xyz + xyzw: the object's state pose expressed in that link's COM frame
 * (the frame of RR_KIN_LINK_POSE), link_pose^-1 o object pose.  While the feature is on, rr_posture_clearance, rr_signed_distance and
 * rr_signed_gradient place an attached object at T_link(posture) o rel -- R_o = R_b R_rel, p_o = p_b + R_b t_rel from the row's forward
 * kinematics, not from the state -- and, in the gradient, give its shapes the joint columns of the link's body, at candidate postures
 * and at the present state (postures == NULL) alike: RR_SG_PAIR_GRADIENT then has columns for a carried object.  A free object, and
 * every object of an env with no attachment, is staged by the operations of the <false> instantiations: every number that no carried shape
 * enters has the bits it has with the feature off.  The same buffers with the same layouts are written; body_a / body_b keep reporting
 * 16 + o for an object, attached or not.  rr_closest_points is unaffected (at the present state an object is where the state says).
 * rr_swept_clearance REFUSES while the feature is on (RR_EINVAL, nothing written): its proof rests on a reach table that is a constant
 * of the model and it stages the objects once per row.  rr_carried_sweep, below, is the edge check that moves them.
 * rr_set_attachments replaces the rows of the masked envs (env_mask u8 [N] host, NULL: every env) WHOLE:
 *   link != NULL, rel_pose != NULL: the given poses; a quaternion is normalised on the host in float64.
 *   link != NULL, rel_pose == NULL: CAPTURE -- one small kernel on the library's stream, behind whatever was enqueued, writes
 *     rel = T_link(q_present)^-1 o T_object(present) for the attached objects of the masked envs with the step's forward kinematics:
 *     "attach what the gripper holds right now" without a host round trip for the poses.
 *   link == NULL: the masked envs' objects are detached.  link == NULL and env_mask == NULL turns the feature OFF: the three queries
 *     launch the <false> instantiations, the instructions they ran before this entry point existed, as on a handle that never attached.
 * The device table holds {moving body, rotation, translation in that body's frame}; the host converts from and to the link's COM
 * frame in float64 through the model's link table, so rr_get_attachments returns a pose that differs from the one given by float32
 * rounding (and possibly by the quaternion's sign).  The call waits for the stream: its arguments are host memory.
 * PERSISTENT: rr_reset, an episode's auto-reset, rr_write_state, rr_set_state, steps and rr_set_distance_pairs keep the table;
 * rr_copy_envs leaves it with the DESTINATION env, like every other setting; checkpoints and snapshots do not carry it.
 * Errors: RR_EINVAL with a message naming env and object, and NOTHING changed, for a link outside [0, 17) that is not -1, a link that
 * is rigid with the world, a non-finite rel pose or a quaternion of norm zero in a masked row; RR_EINVAL for a null env and for rel_pose
 * without link; RR_EDEVICE for a failed allocation (all or nothing through the handle's memory owner; the table, N x 192 bytes,
 * zero-filled, and its staging block on first use) or a device error.  Detaching on a handle that never attached is RR_OK with
 * nothing allocated.
 * Out of scope: a device-resident table or mask and a zero-copy view of the table; carried
 * poses as an output of rr_posture_kinematics (compose link_pose o rel in torch); gradients with respect to rel; any constraint in
 * the step. */
int rr_set_attachments(rr_env *env, const int32_t *link /* i32 [N][n_obj] host, or NULL: detach */,
                       const float *rel_pose /* f32 [N][n_obj][7] host, or NULL: capture from the present state */,
                       const uint8_t *env_mask /* u8 [N] host or NULL: every env */);
/* The table in force: link_out i32 [N][n_obj] (-1: free), rel_pose_out f32 [N][n_obj][7] (the identity for a free object); either
 * may be NULL.  Synchronising when rel_pose_out is given. */
int rr_get_attachments(rr_env *env, int32_t *link_out /* [N][n_obj] */, float *rel_pose_out /* [N][n_obj][7] */);

/* Swept clearance with carried objects: the attached-body edge check (additive in ABI 7; k_swept_clearance<true>: csrc/rr_sweep.inc).
 * rr_swept_clearance proves an edge free for the empty hand; the transport half of a pick-and-place plan moves an object through the
 * same shelf.  rr_carried_sweep is rr_swept_clearance -- its arguments, its validation and refusals (under this call's name), its host
 * staging and STREAM CONTRACT, its four RR_SW_* buffers in the same layouts, read through rr_sweep_buffer and rr_sweep_copy_to_host:
 * NO new buffer family -- with ONE difference: it does not refuse while attachments are on.
 * Attachments OFF (a handle that never attached, or after the unmasked detach): the call forwards to rr_swept_clearance -- the same
 * kernel, the same bytes.  A planner can always call this one function.
 * Attachments ON: one launch of k_swept_clearance<true> on the library's stream, one wave64 per (env, segment) like <false>.
 * The motion model.  q(t) = q0 + t (q1 - q0), t in [0, 1].  An ATTACHED object of env e moves with its link: at every posture the
 * advancement evaluates it is re-staged as R_o = R_b R_rel, p_o = p_b + R_b t_rel from that posture's forward kinematics and the
 * env's table row, by the device function rr_posture_clearance uses while attachments are on.  A FREE object stays at env e's present pose.
 * The carried reach.  A shape s of an object attached to moving body b takes the joint mask "ancestors-or-self of b".  For a joint k
 * of that mask its reach is chain[k][b] + rho: chain[k][b] is the sum of |body_jpos[m]| over the bodies m on the chain from b up
 * to, but not including, k -- the term of the reach table, built once on the host in float64 and rounded UP to float32, an 11 x 11
 * table allocated on first use through the handle's memory owner, all or nothing --, and rho = |t_rel + R_rel c_s| + ||R_rel|| r_s
 * with (c_s, r_s) the bounding sphere of s in the object's frame.  rho is computed per row on the device from the table row (a
 * captured row never visits the host), with ||R_rel|| MEASURED from the row (a captured rotation is orthonormal to float32 rounding
 * only), an absolute term for a cancelling t_rel + R_rel c_s, and the factor 1 + 2^-18: float32 rounding cannot lower it
 * (csrc/rr_sweep.inc derives the factor).  Robot shapes keep R[k][s] of rr_sweep_reach.
 * The pair bound.  B_j as rr_swept_clearance defines it, over the joints in exactly one of the two masks, ascending k in float32,
 * times 1 + 2^-20: the distance of pair j is B_j-Lipschitz in t with the carried objects moving.  A carried shape against a shape on
 * its own body, and two objects carried by one body, have B_j = 0: one look, horizon +inf.  Two objects on different bodies work
 * through the exclusive-or of their masks.  The advancement, the statuses, `steps` and `pair evaluations` are those of rr_swept_clearance.
 * Guarantees.  Those of rr_swept_clearance with "the distance of pair j along the motion" read with the carried objects moving: for
 * every pair j and every t < min(free_j, 1) it exceeds safety, for every t < fraction every pair's does.  The RR_SW_HIT record of a
 * stopped row is, bit for bit, what rr_posture_clearance returns for that pair at q_stop on the same attached handle.  An env with
 * no attachment on an attached handle gets, in every row, the bytes rr_swept_clearance writes on a handle that never attached.  No
 * atomics and a fixed order: row (e, k) is a function of (env e's objects, env e's table rows, segment (e, k), the tables, safety,
 * tolerance) alone.  The table's body index is clamped before it indexes anything; no other value of the table, the tensor or the
 * state forms an address.  At most RR_SW_MAX_STEPS postures are evaluated whatever the data, a non-finite segment or table row
 * included: such a row leaves the loop within the cap, its outputs unspecified, with status in {0, 1, 3}.
 * Reads what rr_swept_clearance reads, and the attachment table and the chain table; writes the four RR_SW_* buffers only: not the
 * state, the preparation record, la_valid, an error flag or a buffer of another query.  The next step stays prepared.
 * Errors: RR_EINVAL with nothing allocated, nothing written and nothing changed for every cause of rr_swept_clearance's list -- a null
 * env, null segments, n_segments outside [1, RR_PC_MAX_POSTURES], Q == 0, safety < 0 or NaN or infinite, tolerance < 1e-6 or NaN or
 * infinite, a cull's max_distance below safety + tolerance --, the message naming rr_carried_sweep; RR_EDEVICE for a failed allocation
 * or a device error.  The pair table's device copy, the four buffers with their staging block and the chain table are three groups,
 * each all or nothing on its own: a chain table that cannot be allocated leaves the buffers allocated, zero-filled and unwritten.
 * Out of scope: rr_swept_clearance with attachments on (it keeps refusing: its contract is "the objects stay at the present pose");
 * a switch of the vector env; carried poses as an output of rr_posture_kinematics; objects that move on their own during the sweep;
 * every pair's first hit; gradients of the hit time; any use by the step. */
int rr_carried_sweep(rr_env *env, const float *segments /* f32 [N][K][2][11] */, int32_t n_segments, int32_t on_device, float safety, float tolerance);

/* Batched damped-least-squares inverse kinematics for link 7 (gripper `base`), seeded with each env's current joints.
 * Replaces pybullet.calculateInverseKinematics(0, 7, pos, orn, maxNumIterations=1000, residualThreshold=0.001) in
 * step_cartesian (env.py:372-375).  targets: f32 [N, 7] (xyz + xyzw quaternion, host); q_out: f32 [N, 11] (all movable
 * dofs like pybullet; the fingers keep their current values); err_out (nullable): f32 [N] final pose residual. */
int rr_ik(rr_env *env, const float *targets_host, float *q_out_host, float *err_out_host);
/* Replaces REALRobotEnv.generate_plan (env.py:388-454) for the envs selected by the mask (NULL: all): builds the
 * 1000-step joint-space plan of a macro action [[x1, y1], [x2, y2]] on the device. macro: f32 [N, 4] host. */
int rr_plan_macro(rr_env *env, const float *macro_host, const uint8_t *env_mask_host);
/* Copies one env's plan to the host, f32 [1000, 9] (tests / debugging). */
int rr_get_plan(rr_env *env, int32_t env_index, float *plan_host);
/* Replaces step_macro's next_step() + step_joints (env.py:404-412, 463-467): every env consumes the next row of its
 * plan (the last row repeats once the plan is exhausted; the host decides when to re-plan) and steps. */
int rr_step_plan(rr_env *env, int32_t render_mode, const uint8_t *render_flags_host);
/* Same, but the envs whose idle byte is non-zero (u8 [N], host; NULL: none) take the command zeros(9) for this step and
 * keep their place in the plan: step_macro with macro_action None (env.py:391-393). */
int rr_step_plan_masked(rr_env *env, const uint8_t *idle_mask_host, int32_t render_mode, const uint8_t *render_flags_host);

/* Device-resident macro actions: REALRobotEnv.step_macro (env.py:388-467) for the whole batch in ONE call per step, the re-plan
 * decision of env.py:388-408 taken on the device.  The handle keeps, per env, a REQUEST RECORD f32 [4] {p1x, p1y, p2x, p2y} (all NaN on
 * creation), and shares the plan [1000][9] and the plan position with rr_plan_macro / rr_step_plan.  Buffers of rr_macro_buffer: */
enum {
    RR_MACRO_REQUEST = 0,   /* f32 [N, 4]        the request each env's plan was made for; NaN: none, or invalidated */
    RR_MACRO_POSITION = 1,  /* i32 [N]           the plan row the env's next step takes (rows beyond 999: the last row); rr_plan_macro's cursor */
    RR_MACRO_REPLANNED = 2, /* u8  [N]           1 where the last rr_step_macro planned, 0 elsewhere (idle envs included) */
    RR_MACRO_PLAN = 3,      /* f32 [N, 1000, 9]  the plans: what rr_get_plan reads, env by env */
    RR_MACRO_COUNT = 4
};
/* macro: f32 [N][4]; idle: u8 [N] or NULL (none).  With macro_on_device / idle_on_device != 0 they are device memory, read in place on
 * the library's stream WITHOUT a wait (produce them on that stream or synchronise first; keep them unchanged until later work on that
 * stream), as rr_set_joint_torques reads its table; otherwise host arrays, staged, and the call waits at its end.  Per env:
 *   idle[e] != 0 (the reference's `macro_action is None`, env.py:391-393): the command is zeros(9); record, plan and position untouched.
 *   otherwise: same = all four floats == the record (IEEE ==, as np.all(a == b): -0.0 equals 0.0, a NaN equals nothing -- a NaN request
 *   re-plans on every step); need = !same || position >= 1000 (env.py:395-403).  A needing env stores the request in its record, gets a
 *   new plan from its PRESENT joints (rr_plan_macro's rows bit for bit, RR_SOLVER_IK_SINGLE_SEED included) and position 0.  Every
 *   non-idle env then takes plan row min(position, 999) as its command and advances its position (env.py:404-412, 463-467).
 * The step itself is rr_step on that command, as in rr_step_plan_masked; render_mode / render_flags_host as there.  With device
 * arguments nothing waits and nothing is read back: the list of needing envs and its length stay on the device.
 * Values are not validated (as in rr_plan_macro).  The record, the list and the RR_MACRO_REPLANNED bytes are allocated by the first call
 * (with the plan buffers where the handle has none), all or nothing.
 * Errors: RR_EINVAL with every env and every record untouched for a null env, a null macro, a bad render_mode (rr_step_plan's rule), and
 * for an idle array on the other side than macro (a mixed pair); RR_EDEVICE for a failed allocation or a device error.
 * Resets (rr_reset, auto-resets), rr_write_state, rr_set_state, forks / rr_copy_envs, snapshot loads and checkpoint restores KEEP the
 * record, plan and position of the destination env: policy state, like a plan in flight.  The reference does not re-plan on reset
 * either; a caller who wants that calls rr_macro_invalidate.  rr_plan_macro and rr_step_plan* share the plan and the position but do not
 * know the record: mixing them with rr_step_macro on one handle is legal, and the result is defined by the three buffers alone -- after
 * rr_plan_macro an env whose record still equals the next request keeps the plan rr_plan_macro made and goes on from its position. */
int rr_step_macro(rr_env *env,
                  const float *macro /* f32 [N][4] {p1x, p1y, p2x, p2y} */, int32_t macro_on_device,
                  const uint8_t *idle /* u8 [N] or NULL */,                 int32_t idle_on_device,
                  int32_t render_mode, const uint8_t *render_flags_host);
/* NaN into the record rows of the envs whose mask byte is non-zero (u8 [N], host or device; NULL: all envs): the next non-idle
 * rr_step_macro re-plans them from their present joints -- "re-plan after a reset".  Plans and positions are not touched.  A device mask
 * is read in place without a wait; with a host mask the call waits.  A handle without a record has nothing to invalidate. */
int rr_macro_invalidate(rr_env *env, const uint8_t *env_mask, int32_t mask_on_device);
/* Zero-copy device pointer + size of an RR_MACRO_* buffer, valid until rr_destroy (allocates the group on first use: record NaN,
 * positions and plans zero).  STREAM CONTRACT as for the other device buffers.  Not a family of the query table: an accessor pair of
 * its own, like rr_episode_buffer / rr_episode_copy_to_host. */
int rr_macro_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_MACRO_* buffer to host memory. */
int rr_macro_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* Device-resident cartesian actions: REALRobotEnv.step_cartesian (env.py:358-386) for the whole batch in ONE call per step, the IK
 * decision of env.py:358-386 taken on the device.  The handle keeps, per env, a REQUEST RECORD f32 [7] {x, y, z, qx, qy, qz, qw} (all NaN
 * on creation), the SOLUTION f32 [7] of that request (the reference's last_ik) and its residual.  Buffers of rr_cartesian_buffer: */
enum {
    RR_CART_REQUEST = 0,    /* f32 [N, 7]        the request each env's solution was made for; NaN: none, or invalidated */
    RR_CART_SOLUTION = 1,   /* f32 [N, 7]        the stored solution: the arm joints a non-idle env is commanded to */
    RR_CART_RESIDUAL = 2,   /* f32 [N]           ik_solve's returned error of that solution (rr_ik's err_out) */
    RR_CART_SOLVED = 3,     /* u8  [N]           1 where the last rr_step_cartesian solved, 0 elsewhere (idle envs included) */
    RR_CART_COUNT = 4
};
/* cartesian: f32 [N][7]; gripper: f32 [N][2]; idle: u8 [N] or NULL (none).  ONE flag covers the three arrays: with on_device != 0 they
 * are device memory, read in place on the library's stream WITHOUT a wait (produce them on that stream or synchronise first; keep them
 * unchanged until later work on that stream), as rr_step_macro reads its request; otherwise host arrays, staged, and the call waits at
 * its end.  Per env (env.py:358-386):
 *   idle[e] != 0 (the reference's `cartesian_command is None`, env.py:359-361): the command is zeros(9); record and solution untouched.
 *   otherwise: same = all seven floats == the record (IEEE ==, as np.all(a == b): -0.0 equals 0.0, a NaN equals nothing -- a NaN request
 *   solves on every step; env.py:366-369).  When same, the arm command is the stored solution: it is NOT solved again from the new
 *   joints, exactly as the reference reuses last_ik (env.py:370).  When not same, the env is solved from its PRESENT joints by rr_ik's rule
 *   -- ik_solve with no predecessor, seeds {present joints, elbow-up} or one seed under RR_SOLVER_IK_SINGLE_SEED, maxNumIterations 1000
 *   (env.py:372-375); rr_ik's joints and residual bit for bit --, the request goes into the record, the result into the solution, the
 *   error into the residual (env.py:376-378).
 *   The command is [solution[0..6], gripper[0], gripper[1]] (env.py:380-381): the gripper is read every step and is no part of the record.
 * The step itself is rr_step on that command (env.py:386), as in rr_step_macro; render_mode / render_flags_host as there.  With device
 * arguments nothing waits and nothing is read back: the list of needing envs and its length stay on the device.
 * Values are not validated (as in rr_ik); a non-finite command is rr_step's business.  The four buffers, the list and the staging of host
 * arguments are allocated by the first call as one group, all or nothing.
 * Errors: RR_EINVAL with every env and every record untouched for a null env, a null cartesian or gripper, a bad render_mode
 * (rr_step_plan's rule), and for a mixed set: an array that the runtime knows to live on the other side than on_device says (pageable
 * host memory under on_device != 0, device memory under on_device == 0; pinned and managed memory serve either side); RR_EDEVICE for a
 * failed allocation or a device error.
 * Resets (rr_reset, auto-resets), rr_write_state, rr_set_state, forks / rr_copy_envs, snapshot loads and checkpoint restores KEEP the
 * record and solution of the destination env: policy state, like rr_step_macro's record.  The reference does not solve again on reset
 * either (env.py:358-386 know no reset); a caller who wants that calls rr_cartesian_invalidate.  rr_step, rr_step_macro and rr_ik do not
 * know these buffers and change none of them: mixing them with rr_step_cartesian on one handle is legal.
 * Out of scope: a cartesian action type of the vector env; targets for other links or points (rr_posture_ik has them); clamping to joint
 * limits (the reference wraps); any change of rr_ik or the ik defaults. */
int rr_step_cartesian(rr_env *env,
                      const float *cartesian /* f32 [N][7] {x, y, z, qx, qy, qz, qw} */,
                      const float *gripper /* f32 [N][2] */,
                      const uint8_t *idle /* u8 [N] or NULL */,
                      int32_t on_device, int32_t render_mode, const uint8_t *render_flags_host);
/* NaN into the record rows of the envs whose mask byte is non-zero (u8 [N], host or device; NULL: all envs): the next non-idle
 * rr_step_cartesian solves them from their present joints (env.py:358-386: "solve again after a reset").  Solutions and residuals are not
 * touched.  A device mask is read in place without a wait; with a host mask the call waits.  A handle without a record has nothing to
 * invalidate. */
int rr_cartesian_invalidate(rr_env *env, const uint8_t *env_mask, int32_t mask_on_device);
/* Zero-copy device pointer + size of an RR_CART_* buffer (the state of env.py:358-386 for the batch), valid until rr_destroy (allocates
 * the group on first use: record NaN, the others zero).  STREAM CONTRACT as for the other device buffers.  Not a family of the query
 * table: an accessor pair of its own, like rr_macro_buffer / rr_macro_copy_to_host. */
int rr_cartesian_buffer(rr_env *env, int32_t which, void **dev_ptr, size_t *bytes);
/* Synchronising copy of a whole RR_CART_* buffer (env.py:358-386's requested_coords / requested_orient / last_ik) to host memory. */
int rr_cartesian_copy_to_host(rr_env *env, int32_t which, void *dst, size_t bytes);

/* Per-kernel device timing with HIP events on the library's stream (bench.py roofline leg).
 * After rr_set_timing(env, 1), each rr_step/rr_render records events; rr_get_timing returns accumulated
 * milliseconds and launch counts per kernel since the last call and resets them.
 * kernel ids: 0 prep (state part: forward kinematics, object terms, joint-space dynamics), 1 collide, 2 solve (command part --
 * rate limit, clipping, motor targets -- then rows, Gauss-Seidel, integration), 3 render_setup, 4 raster, 5 image set-up outside
 * the two render kernels (the full static copy of the first frame, and of every frame with RR_FULL_COPY), 6 shade.
 * When the step would run its heavy envs on the side stream, the timed step runs the same launches one
 * after the other: 2 / 3 / 4 / 6 then hold what the main stream runs (the light envs), 7 the solve and 8 the render
 * (set-up + raster + shade) of the heavy envs, which run beside them in an untimed step.  0 and 1 are the LOOK-AHEAD of the
 * next step, which an untimed step runs under its render. */
#define RR_NUM_KERNELS 9
int rr_set_timing(rr_env *env, int32_t enable);
int rr_get_timing(rr_env *env, float *ms_out /*[RR_NUM_KERNELS]*/, int32_t *launches_out /*[RR_NUM_KERNELS]*/);

/* Device micro-benchmarks for the roofline of bench.py (the achievable figure is measured in the same run, not quoted):
 * kind 0: HBM copy bandwidth, 1: HBM triad bandwidth (GB/s; 256 MiB arrays); 2: VALU issue rate of a sample-test-like instruction
 * mix at eight waves per SIMD (G wave64-instructions/s).  No env handle needed; fails with RR_EDEVICE without a GPU. */
int rr_device_microbench(int32_t device, int32_t kind, double *result);

const char *rr_last_error(void);
int rr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
