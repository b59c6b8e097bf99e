"""ctypes binding of librealrobot_hip.so (C ABI in include/realrobot.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is present, creation fails
loudly (RuntimeError) -- nothing here imports the oracle.
"""
import ctypes as C
import gzip
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RR_LIB', os.path.join(_HERE, 'csrc', 'librealrobot_hip.so'))
BLOB_GZ = os.environ.get('RR_MODEL', os.path.join(_HERE, 'data', 'realrobot_model.bin.gz'))      # (RR_MODEL: another compiled model, A/B)
LINK_NAMES = open(os.path.join(_HERE, 'data', 'realrobot_model_links.txt')).read().split()

RR_ABI_VERSION = 7
(F_JOINTS, F_TOUCH, F_OBJ_POSE, F_RGB, F_DEPTH, F_MASK, F_TIMESTEP, F_ERRFLAGS, F_STATE, F_FRAG_COUNT, F_CONTACT_COUNT,
 F_ENV_CLASS, F_PREP, F_CONTACTS, F_BODY_FORCE, F_BODY_PARTNERS) = range(16)
PREP_FLOATS = 378          # RR_F_PREP: frames 165, M^-1 121, qd* 11, object terms 81 -- in this order (realrobot.hip S_*)
MAX_CONTACTS = 48          # rows of RR_F_CONTACTS per env
CONTACT_ROWS = 20          # RR_CONTACT_ROWS: body rows of RR_F_BODY_FORCE / RR_F_BODY_PARTNERS (17 URDF links, then objects 0..2)
NUM_KERNELS = 9
# id 5 = image set-up outside the two render kernels: the full static copy of the first frame (and of every frame with the
# earlier scheme RR_FULL_COPY); it does not run in steady state
KERNEL_NAMES = ('k_prep', 'k_collide', 'k_solve', 'k_render_setup', 'k_raster', 'k_image_setup', 'k_shade',
                'k_solve_heavy', 'render_heavy')      # 7, 8: the heavy envs' solve / render (side streams in an untimed step);
                                                      # k_prep / k_collide = the look-ahead of the next step

# every symbol include/realrobot.h declares (tests check the library exports all of them)
SYMBOLS = ('rr_create', 'rr_destroy', 'rr_set_stream', 'rr_reset', 'rr_set_object_pose', 'rr_set_object_home', 'rr_step', 'rr_render',
           'rr_get_buffer', 'rr_copy_to_host', 'rr_set_state', 'rr_sync', 'rr_link_poses', 'rr_get_contacts',
           'rr_set_timing', 'rr_get_timing', 'rr_last_error', 'rr_abi_version', 'rr_ik', 'rr_plan_macro', 'rr_get_plan',
           'rr_step_plan', 'rr_set_camera', 'rr_set_object_poses', 'rr_step_plan_masked', 'rr_checkpoint_bytes',
           'rr_checkpoint_save', 'rr_checkpoint_restore', 'rr_evaluate_goals', 'rr_device_microbench', 'rr_map_observations', 'rr_map_images', 'rr_sync_observations', 'rr_select_image_mirror',
           'rr_pack_image_delta', 'rr_apply_image_delta', 'rr_set_object_dynamics', 'rr_get_object_dynamics',
           'rr_set_env_cameras', 'rr_set_env_appearance', 'rr_get_env_appearance', 'rr_render_instances',
           'rr_set_env_actuators', 'rr_get_env_actuators', 'rr_contact_observations',
           'rr_set_goals', 'rr_set_env_goals', 'rr_set_episode', 'rr_episode_update', 'rr_episode_buffer', 'rr_episode_copy_to_host',
           'rr_snapshot_slots', 'rr_copy_envs',
           'rr_set_kinematic_points', 'rr_get_kinematic_points', 'rr_kinematic_observations', 'rr_kinematic_buffer', 'rr_kinematic_copy_to_host',
           'rr_write_state', 'rr_read_state',
           'rr_set_rays', 'rr_get_rays', 'rr_ray_cast', 'rr_ray_buffer', 'rr_ray_copy_to_host',
           'rr_set_distance_pairs', 'rr_get_distance_pairs', 'rr_closest_points', 'rr_distance_buffer', 'rr_distance_copy_to_host',
           'rr_posture_clearance', 'rr_posture_buffer', 'rr_posture_copy_to_host',
           'rr_signed_distance', 'rr_signed_buffer', 'rr_signed_copy_to_host',
           'rr_signed_gradient', 'rr_signed_gradient_buffer', 'rr_signed_gradient_copy_to_host',
           'rr_swept_clearance', 'rr_sweep_reach', 'rr_sweep_buffer', 'rr_sweep_copy_to_host',
           'rr_posture_kinematics', 'rr_posture_kinematics_buffer', 'rr_posture_kinematics_copy_to_host',
           'rr_posture_ik', 'rr_posture_ik_buffer', 'rr_posture_ik_copy_to_host',
           'rr_posture_dynamics', 'rr_posture_dynamics_buffer', 'rr_posture_dynamics_copy_to_host',
           'rr_set_joint_torques', 'rr_get_joint_torques', 'rr_joint_torque_buffer',
           'rr_set_external_wrenches', 'rr_get_external_wrenches', 'rr_external_wrench_buffer',
           'rr_set_attachments', 'rr_get_attachments', 'rr_carried_sweep',
           'rr_step_macro', 'rr_macro_invalidate', 'rr_macro_buffer', 'rr_macro_copy_to_host',
           'rr_step_cartesian', 'rr_cartesian_invalidate', 'rr_cartesian_buffer', 'rr_cartesian_copy_to_host')
# rr_set_object_dynamics / rr_get_object_dynamics: one row of f32 per (env, object)
DYN_ROW = ('mass', 'ixx', 'iyy', 'izz', 'friction', 'restitution', 'rolling', 'spinning')
# rr_set_env_actuators / rr_get_env_actuators: one row of f32 per (env, movable joint), the joints in the order of q[11] of RR_F_STATE
ACT_ROW = ('kp', 'kd', 'max_force', 'damping')
N_JOINTS = 11
# rr_set_external_wrenches: the rows of the wrench table [N, XW_BODIES, 6] -- the eleven moving robot bodies (row j: the body joint j moves), then objects 0..2
XW_BODIES = 14
# buffers of rr_episode_buffer (the RR_EP_* enum: goals and episodes on the device)
(EP_SCORE, EP_REWARD, EP_DONE, EP_GOAL_INDEX, EP_EPISODE, EP_FINAL_OBS, EP_GOAL_POS, EP_GOAL_RGB) = range(8)
EP_NAMES = ('score', 'reward', 'done', 'goal_index', 'episode', 'final_obs', 'goal_pos', 'goal_rgb')
# buffers of rr_macro_buffer (the RR_MACRO_* enum: macro actions decided on the device): request f32 [N, 4], position i32 [N], replanned u8 [N],
# plan f32 [N, 1000, 9]
(MACRO_REQUEST, MACRO_POSITION, MACRO_REPLANNED, MACRO_PLAN) = range(4)
MACRO_NAMES = ('request', 'position', 'replanned', 'plan')
PLAN_LEN = 1000
# buffers of rr_cartesian_buffer (the RR_CART_* enum: cartesian actions decided on the device): request f32 [N, 7], solution f32 [N, 7],
# residual f32 [N], solved u8 [N]
(CART_REQUEST, CART_SOLUTION, CART_RESIDUAL, CART_SOLVED) = range(4)
CARTESIAN_NAMES = ('request', 'solution', 'residual', 'solved')
GOAL_SCORED, GOAL_HAS_START = 1, 2      # rr_set_goals flag bits: the object counts in the score / has a start pose
# buffers of rr_kinematic_buffer (the RR_KIN_* enum), per env: joint_vel [11], link_pose [17, 7], link_vel [17, 6], obj_vel [n_obj, 6],
# point_pos [P, 3], point_vel [P, 6], jacobian [P, 6, 11] for the P points in force (rr_set_kinematic_points)
KIN_FIELDS = ('joint_vel', 'link_pose', 'link_vel', 'obj_vel', 'point_pos', 'point_vel', 'jacobian')
KIN_MAX_POINTS = 8
EE_LINK = 8                             # URDF link id of gripper `base`: the default point, the link rr_ik solves for
# dq = Q_FROM_CMD @ dcmd: how the nine command entries drive the eleven joints (Kuka.apply_action, robot.py:188-201: command 7
# drives q[7] and q[9], command 8 drives -q[8] and -q[10]); the Jacobian over the commands is J @ Q_FROM_CMD
Q_FROM_CMD = np.zeros((N_JOINTS, 9), np.float32)
Q_FROM_CMD[np.arange(7), np.arange(7)] = 1.0
Q_FROM_CMD[[7, 9], 7] = 1.0
Q_FROM_CMD[[8, 10], 8] = -1.0
# buffers of rr_ray_buffer (the RR_RAY_* enum), per env and ray: hit [8] f32 {fraction, distance, x, y, z, nx, ny, nz}, id [4] i32 {uid, body,
# link, shape} (all -1 on a miss), for the R rays in force (rr_set_rays)
RAY_FIELDS = ('hit', 'id')
RAY_MAX = 64
# buffers of rr_distance_buffer (the RR_DIST_* enum), per env and pair: points [12] f32 {distance, lower bound, a xyz, b xyz, n xyz, +0.0},
# id [4] i32 {status, iterations, body A, body B}, for the Q pairs in force (rr_set_distance_pairs)
DIST_FIELDS = ('points', 'id')
DIST_MAX = 96
# buffers of rr_posture_buffer (the RR_PC_* enum), per env and candidate posture: nearest [12] f32 (the `points` row of the nearest pair),
# id [4] i32 {status, pair index, body A, body B}, distance [Q] f32, status [Q] i32 {byte 0 status, byte 1 iterations}, for the K postures of
# the last rr_posture_clearance and the Q pairs in force
PC_FIELDS = ('nearest', 'id', 'distance', 'status')
PC_MAX_POSTURES = 32
# buffers of rr_signed_buffer (the RR_SD_* enum), per env and row (K' = 1 row at the present state, else the K candidate postures): deepest [12] f32
# {signed distance, bound, a xyz, b xyz, n xyz, +0.0} of the pair at the first minimum, id [4] i32 {status, pair index, body A, body B}, signed [Q] f32,
# status [Q] i32 {byte 0 status 0..5, byte 1 GJK iterations, byte 2 expansion trips}; points [N, Q, 12] f32: every pair's record, present-state queries only
SD_FIELDS = ('deepest', 'id', 'signed', 'status', 'points')
# buffers of rr_signed_gradient_buffer (the RR_SG_* enum), rows of 12 f32: gradient [N, K', 12] {d s*/dq_0..10, +0.0} of the row's deepest pair,
# cost [N, K', 12] {dC/dq_0..10, C} of the hinge cost over all pairs, pair_gradient [N, Q, 12] {d s_j/dq_0..10, +0.0}: present-state queries only
SG_FIELDS = ('gradient', 'cost', 'pair_gradient')
# buffers of rr_sweep_buffer (the RR_SW_* enum), per env and segment: stop [12] f32 {fraction, q_stop[11]}, hit [12] f32 (the `points` row of the
# reported pair at q_stop), id [4] i32 {status, pair, steps, pair evaluations}, free [Q] f32 (every pair's free horizon, at most 1), for the K
# segments of the last rr_swept_clearance and the Q pairs in force
SW_FIELDS = ('stop', 'hit', 'id', 'free')
SW_MAX_STEPS = 64
# buffers of rr_posture_kinematics_buffer (the RR_PK_* enum), per env and candidate posture: link_pose [17, 7], point_pos [P, 3], jacobian [P, 6, 11] --
# the rows of the kinematic observations of those names -- for the K postures of the last rr_posture_kinematics and the P points in force
PK_FIELDS = ('link_pose', 'point_pos', 'jacobian')
# buffers of rr_posture_ik_buffer (the RR_PIK_* enum), per env and target: posture f32 [11], result f32 [4] {residual, position error,
# orientation error angle, 0}, info i32 [2] {status, iterations}, for the K targets of the last rr_posture_ik
PIK_FIELDS = ('posture', 'result', 'info')
PIK_MAX_ITERATIONS = 256
PIK_POSITION_ONLY, PIK_CLAMP_LIMITS = 1, 2           # flags of rr_ik_options
PIK_CONVERGED, PIK_CAP, PIK_NOT_FINITE = 0, 1, 2     # status
# buffers of rr_posture_dynamics_buffer (the RR_PD_* enum), per env and row of the last rr_posture_dynamics: mass_matrix f32 [11, 11],
# gravity, bias, torque f32 [11], mass_inverse f32 [11, 11] (written only with PD_INVERSE, the flag RR_PD_INVERSE)
PD_FIELDS = ('mass_matrix', 'gravity', 'bias', 'torque', 'mass_inverse')
PD_INVERSE = 1
SLOT_LIVE, MAX_SLOTS = -1, 64           # RR_SLOT_LIVE: the running envs as a slot number of rr_copy_envs; RR_MAX_SLOTS
# `parts` of rr_write_state (the RR_W_* bits): the column groups of the 61-float state row that are written, a reset in front of them,
# the fresh-start clean-up of rr_set_state behind them
W_JOINT_POS, W_JOINT_VEL, W_OBJ_POSE, W_OBJ_VEL, W_RESET, W_FRESH = 1, 2, 4, 8, 16, 32
W_COLUMNS = W_JOINT_POS | W_JOINT_VEL | W_OBJ_POSE | W_OBJ_VEL
N_LINKS = 17                            # URDF links: the rows of rr_link_poses


class QueryFamily:
    """One whole-batch query family of include/realrobot.h: the fields tuple (the RR_*_ enum in order), the stem of its two symbols
    `<stem>_buffer` / `<stem>_copy_to_host`, the label of the ValueError for an unknown buffer, and per buffer (dtype, shape, free).
    A shape is made of numbers and the dims 'N' envs, 'K' rows of the last call, 'Q' pairs, 'P' points or rays, 'O' objects; `free` is
    the one dim that is solved from the library's byte count (None for the four kinematic buffers that have none)."""

    def __init__(self, stem, label, fields, buffers):
        self.stem, self.label, self.fields, self.buffers = stem, label, fields, buffers
        self.buffer, self.copy_to_host = stem + '_buffer', stem + '_copy_to_host'

    def shape(self, which, dims, nbytes=None):
        """Shape of buffer `which` for `dims`; with nbytes the free dim is solved from it (0 where another dim is 0)."""
        dt, shape, free = self.buffers[which]
        if nbytes is not None and free is not None:
            row = np.dtype(dt).itemsize * int(np.prod([x if isinstance(x, int) else dims[x] for x in shape if x != free]))
            dims = dict(dims, **{free: nbytes // row if row else 0})
        return tuple(x if isinstance(x, int) else int(dims[x]) for x in shape)

    def nbytes(self, which, dims):
        return np.dtype(self.buffers[which][0]).itemsize * int(np.prod(self.shape(which, dims)))


_f4, _i4 = np.float32, np.int32
_ROW12 = {'K': (_f4, ('N', 'K', 12), 'K'), 'Q': (_f4, ('N', 'Q', 12), 'Q')}      # a [12] f32 record per row / per pair
_PAIRS = lambda dt: (dt, ('N', 'K', 'Q'), 'K')
QUERY_FAMILIES = dict(
    kinematic=QueryFamily('rr_kinematic', 'kinematic', KIN_FIELDS, (
        (_f4, ('N', N_JOINTS), None), (_f4, ('N', N_LINKS, 7), None), (_f4, ('N', N_LINKS, 6), None), (_f4, ('N', 'O', 6), None),
        (_f4, ('N', 'P', 3), 'P'), (_f4, ('N', 'P', 6), 'P'), (_f4, ('N', 'P', 6, N_JOINTS), 'P'))),
    ray=QueryFamily('rr_ray', 'ray', RAY_FIELDS, ((_f4, ('N', 'P', 8), 'P'), (_i4, ('N', 'P', 4), 'P'))),
    distance=QueryFamily('rr_distance', 'distance', DIST_FIELDS, (_ROW12['Q'], (_i4, ('N', 'Q', 4), 'Q'))),
    posture=QueryFamily('rr_posture', 'posture', PC_FIELDS, (_ROW12['K'], (_i4, ('N', 'K', 4), 'K'), _PAIRS(_f4), _PAIRS(_i4))),
    signed=QueryFamily('rr_signed', 'signed-distance', SD_FIELDS, (_ROW12['K'], (_i4, ('N', 'K', 4), 'K'), _PAIRS(_f4), _PAIRS(_i4), _ROW12['Q'])),
    signed_gradient=QueryFamily('rr_signed_gradient', 'signed-gradient', SG_FIELDS, (_ROW12['K'], _ROW12['K'], _ROW12['Q'])),
    sweep=QueryFamily('rr_sweep', 'sweep', SW_FIELDS, (_ROW12['K'], _ROW12['K'], (_i4, ('N', 'K', 4), 'K'), _PAIRS(_f4))),
    posture_kinematics=QueryFamily('rr_posture_kinematics', 'posture kinematics', PK_FIELDS, (
        (_f4, ('N', 'K', N_LINKS, 7), 'K'), (_f4, ('N', 'K', 'P', 3), 'K'), (_f4, ('N', 'K', 'P', 6, N_JOINTS), 'K'))),
    posture_ik=QueryFamily('rr_posture_ik', 'posture IK', PIK_FIELDS, (
        (_f4, ('N', 'K', N_JOINTS), 'K'), (_f4, ('N', 'K', 4), 'K'), (_i4, ('N', 'K', 2), 'K'))),
    posture_dynamics=QueryFamily('rr_posture_dynamics', 'posture dynamics', PD_FIELDS, (
        (_f4, ('N', 'K', N_JOINTS, N_JOINTS), 'K'), (_f4, ('N', 'K', N_JOINTS), 'K'), (_f4, ('N', 'K', N_JOINTS), 'K'), (_f4, ('N', 'K', N_JOINTS), 'K'),
        (_f4, ('N', 'K', N_JOINTS, N_JOINTS), 'K'))),
)


class Config(C.Structure):
    _fields_ = [('abi_version', C.c_int32), ('num_envs', C.c_int32), ('n_objects', C.c_int32),
                ('width', C.c_int32), ('height', C.c_int32), ('device', C.c_int32), ('solver_iters', C.c_int32),
                ('envs_per_block', C.c_int32), ('dt', C.c_float), ('erp', C.c_float), ('margin', C.c_float),
                ('use_urdf_inertia', C.c_int32), ('flags', C.c_int32),
                # the constants the reference leaves to pybullet's defaults (include/realrobot.h: 0 -> default, < 0 -> literal zero)
                ('motor_kp', C.c_float), ('motor_kd', C.c_float), ('motor_max_force', C.c_float), ('warmstart', C.c_float),
                ('lin_damping', C.c_float), ('ang_damping', C.c_float), ('solver_flags', C.c_int32)]


FLAG_NO_MASK = 1
SOLVER_NO_RATE_LIMIT = 1
SOLVER_IK_SINGLE_SEED = 2
# `solver=` of BatchedREALRobotEnv / make(): name -> documented default (UPSTREAM, unverifiable here)
SOLVER_DEFAULTS = {'motor_kp': 0.1, 'motor_kd': 1.0, 'motor_max_force': 100000.0, 'warmstart': 0.85, 'lin_damping': 0.04,
                   'ang_damping': 0.04, 'erp': 0.2, 'rate_limit': True, 'ik_single_seed': False}


def apply_solver(cfg, solver):
    """Writes a `solver` dict (keys of SOLVER_DEFAULTS; None / missing: the default) into an rr_config.  A value of exactly 0 is
    passed as the header's "literal zero" (a negative number); unknown keys and non-finite values raise ValueError."""
    for k, v in (solver or {}).items():
        if k not in SOLVER_DEFAULTS:
            raise ValueError("unknown solver parameter %r (known: %s)" % (k, ', '.join(sorted(SOLVER_DEFAULTS))))
        if k == 'rate_limit':
            cfg.solver_flags = (cfg.solver_flags & ~SOLVER_NO_RATE_LIMIT) | (0 if v else SOLVER_NO_RATE_LIMIT)
            continue
        if k == 'ik_single_seed':
            cfg.solver_flags = (cfg.solver_flags & ~SOLVER_IK_SINGLE_SEED) | (SOLVER_IK_SINGLE_SEED if v else 0)
            continue
        v = float(v)
        if not np.isfinite(v) or v < 0:
            raise ValueError("solver parameter %s must be finite and >= 0" % k)
        if k == 'erp' and v == 0:
            raise ValueError("solver parameter erp must be > 0")
        setattr(cfg, k, v if v > 0 else -1.0)


_lib = None
_blob = None


def model_blob():
    global _blob
    if _blob is None:
        with gzip.open(BLOB_GZ, 'rb') as f:
            _blob = f.read()
    return _blob


def load_library():
    """Loads librealrobot_hip.so; raises RuntimeError with a build hint when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "real_robots_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C real_robots_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own HIP/HSA runtime. If torch is going to be used in this process (zero-copy
    # views of the observation buffers, torch.distributed), its runtime stack has to be loaded before this library's
    # (/opt/rocm) one, otherwise torch later reports "No HIP GPUs are available". Importing torch first is harmless
    # when it is not needed and is skipped when it is not installed.
    if os.environ.get('RR_NO_TORCH_PRELOAD') is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    L.rr_create.argtypes = [C.POINTER(Config), C.c_char_p, C.c_size_t, vp, C.POINTER(vp)]
    L.rr_destroy.argtypes = [vp]
    L.rr_set_stream.argtypes = [vp, vp]
    L.rr_reset.argtypes = [vp, vp]
    L.rr_set_object_pose.argtypes = [vp, i32, i32, vp]
    L.rr_set_object_home.argtypes = [vp, i32, i32, vp]
    L.rr_step.argtypes = [vp, vp, i32, i32, vp]
    L.rr_render.argtypes = [vp]
    L.rr_get_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rr_copy_to_host.argtypes = [vp, i32, vp, C.c_size_t]
    L.rr_set_state.argtypes = [vp, vp]
    L.rr_sync.argtypes = [vp]
    L.rr_link_poses.argtypes = [vp, vp]
    L.rr_get_contacts.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.rr_contact_observations.argtypes = [vp]
    L.rr_set_timing.argtypes = [vp, i32]
    L.rr_get_timing.argtypes = [vp, vp, vp]
    L.rr_ik.argtypes = [vp, vp, vp, vp]
    L.rr_plan_macro.argtypes = [vp, vp, vp]
    L.rr_get_plan.argtypes = [vp, i32, vp]
    L.rr_step_plan.argtypes = [vp, i32, vp]
    L.rr_set_camera.argtypes = [vp, vp, vp]
    L.rr_set_env_cameras.argtypes = [vp, vp, vp, vp]
    L.rr_set_env_appearance.argtypes = [vp, vp, vp, vp]
    L.rr_get_env_appearance.argtypes = [vp, vp, vp]
    L.rr_render_instances.argtypes = [vp, C.POINTER(i32), vp]
    L.rr_set_object_poses.argtypes = [vp, vp, vp]
    L.rr_step_plan_masked.argtypes = [vp, vp, i32, vp]
    L.rr_evaluate_goals.argtypes = [vp, vp, vp, vp]
    L.rr_device_microbench.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    L.rr_map_observations.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rr_sync_observations.argtypes = [vp]
    L.rr_map_images.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rr_select_image_mirror.argtypes = [vp, C.c_int32]
    L.rr_pack_image_delta.argtypes = [vp, vp, vp, C.c_uint32]
    L.rr_apply_image_delta.argtypes = [vp, vp, i32, C.c_uint32, C.c_size_t, vp, vp, vp]
    L.rr_set_object_dynamics.argtypes = [vp, vp, vp]
    L.rr_get_object_dynamics.argtypes = [vp, vp]
    L.rr_set_env_actuators.argtypes = [vp, vp, vp]
    L.rr_get_env_actuators.argtypes = [vp, vp]
    L.rr_set_goals.argtypes = [vp, i32, vp, vp, vp, vp]
    L.rr_set_env_goals.argtypes = [vp, vp, vp]
    L.rr_set_episode.argtypes = [vp, i32, i32]
    L.rr_episode_update.argtypes = [vp, i32]
    L.rr_episode_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rr_episode_copy_to_host.argtypes = [vp, i32, vp, C.c_size_t]
    L.rr_snapshot_slots.argtypes = [vp, i32]
    L.rr_copy_envs.argtypes = [vp, i32, i32, vp, i32]
    L.rr_set_kinematic_points.argtypes = [vp, i32, vp, vp]
    L.rr_get_kinematic_points.argtypes = [vp, C.POINTER(i32), vp, vp]
    L.rr_kinematic_observations.argtypes = [vp]
    L.rr_write_state.argtypes = [vp, vp, vp, C.c_uint32, i32]
    L.rr_read_state.argtypes = [vp]
    L.rr_set_rays.argtypes = [vp, i32, vp, vp]
    L.rr_get_rays.argtypes = [vp, C.POINTER(i32), vp, vp]
    L.rr_ray_cast.argtypes = [vp, vp, i32]
    L.rr_set_distance_pairs.argtypes = [vp, i32, vp, vp, C.c_float]
    L.rr_get_distance_pairs.argtypes = [vp, C.POINTER(i32), vp, vp, C.POINTER(C.c_float)]
    L.rr_closest_points.argtypes = [vp]
    L.rr_posture_clearance.argtypes = [vp, vp, i32, i32]
    L.rr_signed_distance.argtypes = [vp, vp, i32, i32]
    L.rr_signed_gradient.argtypes = [vp, vp, i32, i32, C.c_float]
    L.rr_swept_clearance.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float]
    L.rr_sweep_reach.argtypes = [vp, vp]
    L.rr_posture_kinematics.argtypes = [vp, vp, i32, i32]
    L.rr_posture_ik.argtypes = [vp, vp, vp, i32, i32, C.POINTER(IkOptions)]
    L.rr_posture_dynamics.argtypes = [vp, vp, vp, vp, i32, i32, C.c_uint32]
    L.rr_set_joint_torques.argtypes = [vp, vp, i32, vp, i32]
    L.rr_get_joint_torques.argtypes = [vp, vp]
    L.rr_joint_torque_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rr_set_external_wrenches.argtypes = [vp, vp, i32, vp, i32]
    L.rr_get_external_wrenches.argtypes = [vp, vp]
    L.rr_external_wrench_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rr_set_attachments.argtypes = [vp, vp, vp, vp]
    L.rr_get_attachments.argtypes = [vp, vp, vp]
    L.rr_carried_sweep.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float]
    L.rr_step_macro.argtypes = [vp, vp, i32, vp, i32, i32, vp]
    L.rr_macro_invalidate.argtypes = [vp, vp, i32]
    L.rr_macro_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rr_macro_copy_to_host.argtypes = [vp, i32, vp, C.c_size_t]
    L.rr_step_cartesian.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.rr_cartesian_invalidate.argtypes = [vp, vp, i32]
    L.rr_cartesian_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rr_cartesian_copy_to_host.argtypes = [vp, i32, vp, C.c_size_t]
    for fam in QUERY_FAMILIES.values():
        getattr(L, fam.buffer).argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
        getattr(L, fam.copy_to_host).argtypes = [vp, i32, vp, C.c_size_t]
    L.rr_checkpoint_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.rr_checkpoint_save.argtypes = [vp, vp, C.c_size_t]
    L.rr_checkpoint_restore.argtypes = [vp, vp, C.c_size_t]
    L.rr_last_error.restype = C.c_char_p
    L.rr_abi_version.restype = i32
    for name in SYMBOLS:
        if name not in ('rr_last_error', 'rr_abi_version'):
            getattr(L, name).restype = i32
    if L.rr_abi_version() != RR_ABI_VERSION:
        raise RuntimeError("real_robots_amd: ABI version mismatch, rebuild the HIP library")
    _lib = L
    return L


class IkOptions(C.Structure):
    """rr_ik_options (include/realrobot.h); the defaults are the header's."""
    _fields_ = [('point', C.c_int32), ('max_iterations', C.c_int32), ('tolerance', C.c_float), ('damping', C.c_float),
                ('max_step', C.c_float), ('flags', C.c_uint32)]

    def __init__(self, point=0, max_iterations=32, tolerance=1e-3, damping=0.1, max_step=0.5, flags=PIK_CLAMP_LIMITS):
        super().__init__(point, max_iterations, tolerance, damping, max_step, flags)


class NativeError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise NativeError("librealrobot_hip: error %d: %s" % (rc, load_library().rr_last_error().decode()))


class DeviceBuffer:
    """Device memory view exposing __cuda_array_interface__ (zero-copy into torch: torch.as_tensor(buf, device=...)).
    strides: bytes per axis for a view that is not compact row-major (a column of a wider buffer); None: compact."""

    def __init__(self, ptr, shape, typestr, owner, strides=None):
        self.ptr, self.shape, self.typestr, self._owner = ptr, tuple(shape), typestr, owner
        self.strides = None if strides is None else tuple(int(x) for x in strides)

    @property
    def __cuda_array_interface__(self):
        return {'shape': self.shape, 'typestr': self.typestr, 'data': (self.ptr, False), 'version': 2, 'strides': self.strides}


# ---------------------------------------------------------------------------------------------- DLPack export
class _DLDevice(C.Structure):
    _fields_ = [('device_type', C.c_int32), ('device_id', C.c_int32)]


class _DLDataType(C.Structure):
    _fields_ = [('code', C.c_uint8), ('bits', C.c_uint8), ('lanes', C.c_uint16)]


class _DLTensor(C.Structure):
    _fields_ = [('data', C.c_void_p), ('device', _DLDevice), ('ndim', C.c_int32), ('dtype', _DLDataType),
                ('shape', C.POINTER(C.c_int64)), ('strides', C.POINTER(C.c_int64)), ('byte_offset', C.c_uint64)]


class _DLManagedTensor(C.Structure):
    pass


_DLDeleter = C.CFUNCTYPE(None, C.POINTER(_DLManagedTensor))
_DLManagedTensor._fields_ = [('dl_tensor', _DLTensor), ('manager_ctx', C.c_void_p), ('deleter', _DLDeleter)]
KDL_ROCM = 10                       # DLDeviceType kDLROCM
_dl_alive = {}                      # address of a DLManagedTensor handed out -> (struct, shape array, strides array or None, owner)


@_DLDeleter
def _dl_deleter(ptr):
    _dl_alive.pop(C.addressof(ptr.contents), None)


_PyCapsuleDestructor = C.CFUNCTYPE(None, C.c_void_p)


@_PyCapsuleDestructor
def _dl_capsule_destructor(capsule):
    # a capsule nobody consumed is still called "dltensor": its tensor is ours to release
    api = C.pythonapi
    api.PyCapsule_IsValid.argtypes, api.PyCapsule_IsValid.restype = [C.c_void_p, C.c_char_p], C.c_int
    api.PyCapsule_GetPointer.argtypes, api.PyCapsule_GetPointer.restype = [C.c_void_p, C.c_char_p], C.c_void_p
    if api.PyCapsule_IsValid(capsule, b'dltensor'):
        _dl_alive.pop(api.PyCapsule_GetPointer(capsule, b'dltensor'), None)


def _dlpack_capsule(ptr, shape, np_dtype, device_id, owner, strides=None):
    """strides: bytes per axis (multiples of the item size) or None for compact row-major."""
    dt = np.dtype(np_dtype)
    code = {'f': 2, 'i': 0, 'u': 1}[dt.kind]
    m = _DLManagedTensor()
    shp = (C.c_int64 * len(shape))(*shape)
    m.dl_tensor.data = ptr
    m.dl_tensor.device = _DLDevice(KDL_ROCM, device_id)
    m.dl_tensor.ndim = len(shape)
    m.dl_tensor.dtype = _DLDataType(code, dt.itemsize * 8, 1)
    m.dl_tensor.shape = shp
    std = None if strides is None else (C.c_int64 * len(shape))(*[x // dt.itemsize for x in strides])
    m.dl_tensor.strides = std           # None: compact row-major; DLPack counts strides in elements
    m.dl_tensor.byte_offset = 0
    m.manager_ctx = None
    m.deleter = _dl_deleter
    _dl_alive[C.addressof(m)] = (m, shp, std, owner)
    api = C.pythonapi
    api.PyCapsule_New.argtypes, api.PyCapsule_New.restype = [C.c_void_p, C.c_char_p, _PyCapsuleDestructor], C.py_object
    return api.PyCapsule_New(C.addressof(m), b'dltensor', _dl_capsule_destructor)


def _dlpack(self, stream=None, **kwargs):
    """DLPack export of a device buffer (zero-copy into torch / cupy / jax on ROCm).  The buffer belongs to the env handle
    (kept alive by the capsule) and is rewritten by every step on the library's stream: `stream` is accepted for protocol
    compatibility, ordering follows the stream contract of include/realrobot.h."""
    return _dlpack_capsule(self.ptr, self.shape, self.typestr, getattr(self._owner, 'device', 0), self._owner, self.strides)


DeviceBuffer.__dlpack__ = _dlpack
DeviceBuffer.__dlpack_device__ = lambda self: (KDL_ROCM, getattr(self._owner, 'device', 0))


def device_microbench(device=0):
    """HBM copy / triad bandwidth (GB/s) and the VALU issue rate of a sample-test-like mix at eight waves per SIMD
    (G wave64-instructions/s), measured on `device` by the library (rr_device_microbench)."""
    L = load_library()
    out = {}
    for kind, name in ((0, 'hbm_copy_GBs'), (1, 'hbm_triad_GBs'), (2, 'valu_mix_G_wave_instr_s')):
        r = C.c_double()
        check(L.rr_device_microbench(int(device), kind, C.byref(r)))
        out[name] = round(r.value, 1)
    return out
