"""Vector-env adapter: N REALRobot envs behind the gymnasium `VectorEnv` calling convention (reset(seed, options) ->
(obs, info); step(actions) -> (obs, rewards, terminations, truncations, infos)), on top of BatchedREALRobotEnv.

The reference has no vectorised env (one env per process); this is the adoption surface SURVEY 8(f4) asks for.
When `gymnasium` is importable the class derives from `gymnasium.vector.VectorEnv`, otherwise it is a plain class with
the same methods and attributes (`num_envs`, `single_action_space`, `single_observation_space`, `action_space`,
`observation_space`).  Episodes end like the reference's (env.py:345-352): `truncated` once `timestep >=
max_episode_steps`.  Autoreset is gymnasium's SAME-STEP mode (`metadata["autoreset_mode"] = "same_step"`): a truncated env
is reset inside the step() that truncated it, the returned observation is the first one of its next episode and the last
observation of the finished episode is in `infos["final_obs"]` (an object array: a dict of the low-dim entries for every finished
env, None elsewhere; `infos["_final_obs"]` is the mask of the envs it applies to) -- every action acts on the episode its observation came from, no action is dropped.
Observations are batched numpy arrays; with `device_obs=True` the image / low-dim entries are the library's device
buffers instead (DLPack / __cuda_array_interface__, zero copy into torch on ROCm).
Domain randomisation of the object dynamics: `dynamics_randomization={'mass': (0.5, 2.0), 'friction': (0.5, 1.5)}` draws, for every
env and object, a multiplier of the model's value uniformly from (low, high) per field (fields: mass, inertia, friction,
restitution, rolling, spinning; inertia takes one multiplier for its three moments, and follows the mass multiplier when only the
mass is randomised -- uniform density).  reset(seed=...) draws every env's values from numpy.random.default_rng(seed); the
same-step autoreset draws again for the truncated envs only.  The values in force are returned under `infos["object_dynamics"]`
(a dict of arrays like BatchedREALRobotEnv.object_dynamics(): every env after reset(); after an autoreset
`infos["_object_dynamics"]` masks the envs that drew new ones).
Domain randomisation of the eye camera: `camera_randomization={'translation': 0.03, 'rotation': 3.0, 'fov': (75, 85)}` gives every env
its own camera (BatchedREALRobotEnv.set_env_cameras): the view is [R | t] V0, a perturbation in camera coordinates of the default
eye V0 (look-at from (0.01, 0, 1.2) to the table, up +z), with t uniform in +-translation metres per axis and R = Rz Ry Rx of
angles uniform in +-rotation degrees; the projection is perspective(fov, W / H, 0.1, 100) with fov uniform in (low, high) degrees
(missing keys: no translation, no rotation, fov 80).  Drawn like the dynamics -- every env on reset(seed=...), the truncated envs on
the same-step autoreset, before the re-render -- from a generator of its own (the dynamics draws of a seed do not depend on it).
The matrices in force are returned as `infos["camera"] = {"view": [N, 4, 4], "proj": [N, 4, 4]}` (float32, row-major); after an
autoreset `infos["_camera"]` masks the envs that drew.
Domain randomisation of the appearance: `appearance_randomization={'colour': (0.7, 1.0), 'brightness': (0.8, 1.2), 'light': 30.0}` gives
every env its own instance colours and light direction (BatchedREALRobotEnv.set_env_appearance): the colour of every render instance
is the model's times a multiplier uniform in `colour` per channel, times one factor per env uniform in `brightness`; the light is the
default direction turned by an angle uniform in [0, `light`] degrees about an axis drawn uniformly among those perpendicular to it
(missing keys: multipliers 1, angle 0).  Drawn like the cameras -- every env on reset(seed=...), the truncated envs on the same-step
autoreset, before the re-render -- from a third generator (the dynamics and camera draws of a seed do not depend on it).  The values
in force are returned as `infos["appearance"] = {"colours": [N, n_inst, 3], "light_dirs": [N, 3]}` (float32; unit light vectors as
drawn, in float32); after an autoreset `infos["_appearance"]` masks the envs that drew.
Domain randomisation of the actuators: `actuator_randomization={'kp': (0.8, 1.2), 'kd': (1.0, 1.2), 'max_force': (0.5, 1.0), 'damping':
(0.5, 2.0)}` gives every env AND joint its own motor gains, motor force and joint damping (BatchedREALRobotEnv.set_env_actuators): a
multiplier of the handle's value (`solver=`, the model's joint damping), uniform in (low, high) per field, missing fields 1.  Drawn
like the other three -- every env on reset(seed=...), the truncated envs on the same-step autoreset -- from a fourth generator (the
dynamics, camera and appearance draws of a seed do not depend on it).  The values in force are returned as `infos["actuators"]` (a
dict of float32 arrays kp, kd, max_force, damping [N, 11], joints in the order of the state's q[11]); after an autoreset
`infos["_actuators"]` masks the envs that drew.  WARNING: the ranges are the user's responsibility.  A velocity gain below 1, or large
position gains without the rate limit (`solver={'rate_limit': False}`), can diverge under full-range commands -- in the float64
oracle as on the device; the error flags (RR_F_ERRFLAGS) tell.
Contact observations: `contact_obs=True` adds `body_force` [N, 20, 2] (float32: {max, sum} of the normal force on each of the 17
robot links and the three objects) and `body_partners` [N, 20] (uint32 bit mask: bit 0 a static body, bit 1 + j object j, bit 4 the
robot) to the observation dict and to the spaces (BatchedREALRobotEnv.contact_observations), computed where the other entries are
gathered: after a same-step autoreset they describe the reset state.  The default leaves dict and spaces as they are.
Kinematic observations: `kinematic_obs=True` adds `joint_velocities` [N, 11], `link_poses` [N, 17, 7], `link_velocities` [N, 17, 6],
`object_velocities` [N, n_objects, 6], `point_positions` [N, P, 3], `point_velocities` [N, P, 6] and `jacobian` [N, P, 6, 11] (float32,
unbounded; BatchedREALRobotEnv.kinematic_observations) to the observation dict and to the spaces, computed where the other entries are
gathered, device views or host copies by `device_obs`.  `kinematic_points=` is a sequence of links (names or indices), or a pair
(links, local_pos [P, 3]); the default is the one point of a fresh handle, the gripper base.  `jacobian @ _native.Q_FROM_CMD` is the
Jacobian over the nine entries of `joint_command`.  The default leaves dict and spaces as they are.  These two arguments and the ones
behind them (`ray_sensors`, `distance_pairs`, `distance_max`, `contact_obs`, `goals`, `goal_stride`) are keyword-only.
Dynamics observations: `dynamics_obs=True` adds the present-state joint-space dynamics `mass_matrix` [N, 11, 11] (M(q) over the eleven
independent joints) and `bias` [N, 11] (G(q) + C(q, qd): the joint torques that keep the present velocities, without joint damping
and motors) to the observation dict and to the spaces (float32, unbounded; BatchedREALRobotEnv.posture_dynamics in its present-state
form), computed where the other entries are gathered, device views or host copies by `device_obs`.  Keyword-only; the default leaves
dict and spaces as they are.
Joint torque actions: `joint_torque_actions=True` adds `"joint_torques"` [N, 11] (float32, unbounded; N m over the eleven independent
joints in the order of the state's q[11]) to the action dict and its spaces: step() forwards it to
BatchedREALRobotEnv.set_joint_torques in front of the step (a numpy array or a CUDA tensor).  The table is PERSISTENT: when the key is
absent the torques in force are kept; nothing clears them after a step, and resets keep them.  Keyword-only; the default leaves dict
and spaces as they are.
External wrench actions: `external_wrench_actions=True` adds `"external_wrenches"` [N, 14, 6] (float32, unbounded; world-frame {force,
torque} rows on the eleven moving robot bodies and objects 0..2, BatchedREALRobotEnv.wrench_row_names) to the action dict and its
spaces: step() forwards it to BatchedREALRobotEnv.set_external_wrenches in front of the step (a numpy array or a CUDA tensor).  The
table is PERSISTENT: when the key is absent the wrenches in force are kept; nothing clears them after a step, and resets keep them.
Keyword-only; the default leaves dict and spaces as they are.
Ray sensors: `ray_sensors=(links, segments)` -- the arguments of BatchedREALRobotEnv.set_rays: R links (names, indices, 'world' / -1)
and segments [R, 6] {from xyz, to xyz} in those links' COM frames -- casts the table against the collision hulls where the other
entries are gathered (BatchedREALRobotEnv.ray_cast: pybullet's rayTestBatch) and adds `ray_distance` [N, R] (float32, metres along the
ray to the first hit; the segment's length on a miss) and `ray_uid` [N, R] (int32, the uid of the mask image; -1 on a miss) to the
observation dict and to the spaces.  With `device_obs` they are strided device views (DLPack / `__cuda_array_interface__`) of the
cast's two buffers.  The default leaves dict and spaces as they are.
Pair distances: `distance_pairs=` -- the `pairs` of BatchedREALRobotEnv.set_distance_pairs: (a, b) collision shapes by name or index,
or 'collision' -- with `distance_max=` (metres; None: no cull) computes the closest points of the pairs where the other entries are
gathered (BatchedREALRobotEnv.closest_points: pybullet's getClosestPoints) and adds `pair_distance` [N, Q] (float32, metres between
the two convex hulls; 0 when they overlap) and `pair_status` [N, Q] (int32: 0 separated, 1 overlapping, 2 culled, 3 iteration cap)
to the observation dict and to the spaces.  With `device_obs` they are strided device views of the query's two buffers.  The
default leaves dict and spaces as they are.
Goals: `goals=` (the path of a goals dataset, or a list of `Goal` objects) with `goal_stride=` puts the goal table and the episode
record on the device (BatchedREALRobotEnv.set_goals_from / episode_update; evaluateGoal, env.py:181-200).  reset() gives env i the
goal i mod G and starts it from that goal's start poses; every step() returns as rewards the change of the env's goal score over
the step (`score - previous score`; the first one of an episode is taken against the score of its start state) -- a device view
with `device_obs=True`, a host copy otherwise --, `infos["goal_score"]` (the score behind the reward: on a truncation step that of
the FINISHED episode) and `infos["goal_index"]` (the goal the returned observation belongs to).  The observations gain `"goal"`
[N, H, W, 3] when the goals carry images (all zero for an env without a goal) and, with `additional_obs`, `"goal_positions"`
[N, n_objects, 3] (NaN where the goal does not name the object).  A truncated env moves on to goal (index + goal_stride) mod G
inside the step that truncated it, on the device: reset, start poses, goal observations; `infos["final_obs"]` comes from the
device's record of the finished episode, in the layout above.  Terminations stay all False.  An env the step froze (a non-finite
state, RR_F_ERRFLAGS & 5) is NOT reset at once: it is reset with the next truncation sweep -- the next step in which any env
reaches `max_episode_steps` --, and is reported as truncated in that step.  Without `goals` nothing changes: zero rewards, the
observation dict and infos as they were.
Macro actions: `action_type='macro_action'` makes the action dict `{"macro_action": [N, 2, 2], "render": ...}` -- the reference's
`macro_space` bounds ([[-0.25, -0.5], [-0.25, -0.5]] .. [[0.05, 0.5], [0.05, 0.5]], env.py:49-52) with a leading env axis -- and step()
calls BatchedREALRobotEnv.step_macro_device: the re-plan decision of REALRobotEnv.step_macro is taken on the device, a numpy array or a
float32 CUDA tensor alike (a bare array [N, 2, 2] is taken as the requests).  The optional key `"macro_idle"` (bool / uint8 [N], on the
same side as the requests; not part of the spaces) flags envs that step with zeros(9) and keep their plan (`macro_action is None`).  As
in the reference a reset keeps an env's plan and its place in it; with `macro_replan_on_reset=True` reset() and the same-step
autoresets -- the device-side reset of a goal step included -- call `macro_invalidate` for the envs they reset, which then re-plan from
their reset posture at their next step.  Both keyword-only; the default `action_type='joints'` leaves spaces, dicts and launches as they
are.
"""
import numpy as np

from . import _native as nat
from . import mathutil, spaces
from .batched import OBJECT_NAMES, BatchedREALRobotEnv
from .envs.robot import Kuka
from .model import load_model

try:                                    # optional dependency
    from gymnasium.vector import VectorEnv as _Base
except Exception:                       # pragma: no cover - gymnasium is not installed in the build container
    _Base = object


def _batch_dict_space(space, n):
    """Dict of Boxes -> the same Dict with a leading axis of n (other entry types are kept as they are)."""
    out = {}
    for k, sp in space.spaces.items():
        if hasattr(sp, 'low') and hasattr(sp, 'high'):
            out[k] = spaces.Box(low=np.broadcast_to(sp.low, (n,) + tuple(sp.shape)).copy(),
                                high=np.broadcast_to(sp.high, (n,) + tuple(sp.shape)).copy(), dtype=sp.dtype)
        else:
            out[k] = sp
    return spaces.Dict(out)


class REALRobotVectorEnv(_Base):
    # observation key -> field of BatchedREALRobotEnv.kinematic_observations
    KINEMATIC_KEYS = (("joint_velocities", "joint_vel"), ("link_poses", "link_pose"), ("link_velocities", "link_vel"),
                      ("object_velocities", "obj_vel"), ("point_positions", "point_pos"), ("point_velocities", "point_vel"),
                      ("jacobian", "jacobian"))

    def __init__(self, num_envs, objects=3, additional_obs=False, eye_width=320, eye_height=240, device=0,
                 max_episode_steps=int(15e6), render_every_step=True, device_obs=False, solver=None, dynamics_randomization=None,
                 camera_randomization=None, appearance_randomization=None, actuator_randomization=None, *, kinematic_obs=False,
                 kinematic_points=None, dynamics_obs=False, joint_torque_actions=False, external_wrench_actions=False, action_type='joints', macro_replan_on_reset=False, ray_sensors=None, distance_pairs=None, distance_max=None, contact_obs=False, goals=None,
                 goal_stride=1):
        self.num_envs = int(num_envs)
        if action_type not in ('joints', 'macro_action'):
            raise ValueError("action_type must be 'joints' or 'macro_action', not %r" % (action_type,))
        self.action_type, self.macro_replan_on_reset = action_type, bool(macro_replan_on_reset)
        if self.macro_replan_on_reset and action_type != 'macro_action':
            raise ValueError("macro_replan_on_reset needs action_type='macro_action'")
        self._goals = None if goals is None else self._check_goals(goals, OBJECT_NAMES[:int(objects)], int(eye_height), int(eye_width))
        self.goal_stride = int(goal_stride)
        self._robot = Kuka(additional_obs, objects, eye_width, eye_height, env=None)
        self.joint_torque_actions = bool(joint_torque_actions)
        self.external_wrench_actions = bool(external_wrench_actions)
        self.single_action_space, self.action_space = self._action_spaces(self._robot, self.num_envs, self.joint_torque_actions, self.external_wrench_actions,
                                                                             self.action_type)
        self.single_observation_space = self._robot.observation_space
        self.contact_obs = bool(contact_obs)
        if self.contact_obs:
            self.single_observation_space = spaces.Dict(dict(
                self._robot.observation_space.spaces,
                body_force=spaces.Box(low=0.0, high=np.inf, shape=(nat.CONTACT_ROWS, 2), dtype=np.float32),
                body_partners=spaces.Box(low=0, high=31, shape=(nat.CONTACT_ROWS,), dtype=np.uint32)))
        self.kinematic_obs = bool(kinematic_obs)
        kin_points = None
        if kinematic_points is not None:
            if not self.kinematic_obs:
                raise ValueError("kinematic_points needs kinematic_obs=True")
            kp = kinematic_points
            pair = isinstance(kp, tuple) and len(kp) == 2 and not isinstance(kp[1], (str, int, np.integer))
            kin_points = BatchedREALRobotEnv._kinematic_points_arg(*(kp if pair else (kp,)))
        if self.kinematic_obs:
            n_pts, n_links = 1 if kin_points is None else len(kin_points[0]), len(nat.LINK_NAMES)
            box = lambda *shape: spaces.Box(low=-np.inf, high=np.inf, shape=shape, dtype=np.float32)
            self.single_observation_space = spaces.Dict(dict(
                self.single_observation_space.spaces,
                joint_velocities=box(nat.N_JOINTS), link_poses=box(n_links, 7), link_velocities=box(n_links, 6),
                object_velocities=box(int(objects), 6), point_positions=box(n_pts, 3), point_velocities=box(n_pts, 6),
                jacobian=box(n_pts, 6, nat.N_JOINTS)))
        self.dynamics_obs = bool(dynamics_obs)
        if self.dynamics_obs:
            self.single_observation_space = spaces.Dict(dict(
                self.single_observation_space.spaces,
                mass_matrix=spaces.Box(low=-np.inf, high=np.inf, shape=(nat.N_JOINTS, nat.N_JOINTS), dtype=np.float32),
                bias=spaces.Box(low=-np.inf, high=np.inf, shape=(nat.N_JOINTS,), dtype=np.float32)))
        ray_table = None
        if ray_sensors is not None:
            if not (isinstance(ray_sensors, (tuple, list)) and len(ray_sensors) == 2):
                raise ValueError("ray_sensors is a pair (links, segments [R, 6])")
            ray_table = BatchedREALRobotEnv._rays_arg(*ray_sensors)
            n_rays = len(ray_table[0])
            if n_rays == 0:
                raise ValueError("ray_sensors: at least one ray")
            self.single_observation_space = spaces.Dict(dict(
                self.single_observation_space.spaces,
                ray_distance=spaces.Box(low=0.0, high=np.inf, shape=(n_rays,), dtype=np.float32),
                ray_uid=spaces.Box(low=-1, high=np.iinfo(np.int32).max, shape=(n_rays,), dtype=np.int32)))
        self.ray_sensors = ray_table is not None
        dist_table = None
        if distance_pairs is not None:
            dist_table = BatchedREALRobotEnv._distance_arg(distance_pairs, distance_max, int(objects))
            n_pairs = len(dist_table[1])
            if dist_table[0] == -1:
                own = np.array(load_model()['shape_owner'])
                n_obj, n_rob, n_sta = int(objects), int((own[:, 0] == 1).sum()), int((own[:, 0] == 0).sum())
                n_pairs = n_obj * n_sta + n_obj * (n_obj - 1) // 2 + 2 * n_rob + n_rob * n_obj
            if n_pairs == 0:
                raise ValueError("distance_pairs: at least one pair")
            self.single_observation_space = spaces.Dict(dict(
                self.single_observation_space.spaces,
                pair_distance=spaces.Box(low=0.0, high=np.inf, shape=(n_pairs,), dtype=np.float32),
                pair_status=spaces.Box(low=0, high=3, shape=(n_pairs,), dtype=np.int32)))
        self.pair_distances = dist_table is not None
        # batched spaces = the single spaces with a leading env axis (gymnasium.vector.utils.batch_space)
        self.observation_space = _batch_dict_space(self.single_observation_space, self.num_envs)
        self.metadata = {"autoreset_mode": "same_step"}
        self.max_episode_steps = int(max_episode_steps)
        self.render_every_step, self.device_obs, self.additional_obs = bool(render_every_step), bool(device_obs), bool(additional_obs)
        self._be = BatchedREALRobotEnv(self.num_envs, objects=objects, width=eye_width, height=eye_height, device=device,
                                       want_mask=additional_obs, solver=solver)
        if kin_points is not None:
            self._be.set_kinematic_points(*kin_points)
        if ray_table is not None:
            self._be.set_rays(*ray_table)
        if dist_table is not None:
            self._be.set_distance_pairs(distance_pairs, distance_max)
        # host-side episode clocks (no device read-back per step): the batched env behind this adapter is private to it, every
        # path that resets an env goes through reset() / step() below and resets its clock with it
        self._steps = np.zeros(self.num_envs, np.int64)
        if self._goals is not None:
            self._g_init, self._g_final, self._g_flags, rgb = self._be.set_goals_from(self._goals)
            self._goal_images = rgb is not None
            self._be.set_episode(self.max_episode_steps, self.goal_stride)
        self._dyn_rand = None
        if dynamics_randomization:
            self._dyn_rand = {}
            for k, r in dynamics_randomization.items():
                if k not in self.DYNAMICS_FIELDS:
                    raise ValueError("dynamics_randomization: unknown field %r (known: %s)" % (k, ', '.join(self.DYNAMICS_FIELDS)))
                lo, hi = (float(x) for x in r)
                if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo <= hi) or (k in ('mass', 'inertia') and lo <= 0):
                    raise ValueError("dynamics_randomization[%r]: need finite 0 <= low <= high (low > 0 for mass / inertia)" % k)
                self._dyn_rand[k] = (lo, hi)
            self._dyn_default = self._be.default_object_dynamics()
        self._dyn_rng = np.random.default_rng()
        self._cam_rand = None
        if camera_randomization:
            cr = dict(translation=0.0, rotation=0.0, fov=(80.0, 80.0))
            for k, r in camera_randomization.items():
                if k not in cr:
                    raise ValueError("camera_randomization: unknown field %r (known: %s)" % (k, ', '.join(cr)))
                if k == 'fov':
                    lo, hi = (float(x) for x in r)
                    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi < 180):
                        raise ValueError("camera_randomization['fov']: need finite 0 < low <= high < 180 (degrees)")
                    cr[k] = (lo, hi)
                else:
                    v = float(r)
                    if not (np.isfinite(v) and v >= 0):
                        raise ValueError("camera_randomization[%r]: need a finite value >= 0" % k)
                    cr[k] = v
            self._cam_rand = cr
            self._cam_aspect = float(eye_width) / float(eye_height)
            self._cam_view0 = mathutil.look_at((0.01, 0.0, 1.2), np.asarray(load_model()['table_pos'], np.float64), (0.0, 0.0, 1.0))
            self._cam_view = np.broadcast_to(self._cam_view0.astype(np.float32), (self.num_envs, 4, 4)).copy()
            self._cam_proj = np.broadcast_to(mathutil.perspective(80.0, self._cam_aspect, 0.1, 100.0).astype(np.float32),
                                             (self.num_envs, 4, 4)).copy()
        self._cam_rng = np.random.default_rng()
        self._app_rand = None
        if appearance_randomization:
            ar = dict(colour=(1.0, 1.0), brightness=(1.0, 1.0), light=0.0)
            for k, r in appearance_randomization.items():
                if k not in ar:
                    raise ValueError("appearance_randomization: unknown field %r (known: %s)" % (k, ', '.join(ar)))
                if k == 'light':
                    v = float(r)
                    if not (np.isfinite(v) and 0 <= v <= 180):
                        raise ValueError("appearance_randomization['light']: need a finite angle in [0, 180] (degrees)")
                    ar[k] = v
                else:
                    try:
                        lo, hi = (float(x) for x in r)
                    except (TypeError, ValueError):
                        raise ValueError("appearance_randomization[%r]: need a (low, high) pair" % k)
                    if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo <= hi):
                        raise ValueError("appearance_randomization[%r]: need finite 0 <= low <= high" % k)
                    ar[k] = (lo, hi)
            self._app_rand = ar
            d = self._be.default_env_appearance()
            self._app_colour0 = d['colours'][0].astype(np.float64)            # the model's colours [n_inst, 3]
            self._app_light0 = d['light_dirs'][0].astype(np.float64)
            self._app_light0 /= np.linalg.norm(self._app_light0)
            self._app_colours, self._app_lights = d['colours'].copy(), d['light_dirs'].copy()
        self._app_rng = np.random.default_rng()
        self._act_rand = None
        if actuator_randomization:
            self._act_rand = {}
            for k, r in actuator_randomization.items():
                if k not in nat.ACT_ROW:
                    raise ValueError("actuator_randomization: unknown field %r (known: %s)" % (k, ', '.join(nat.ACT_ROW)))
                try:
                    lo, hi = (float(x) for x in r)
                except (TypeError, ValueError):
                    raise ValueError("actuator_randomization[%r]: need a (low, high) pair" % k)
                if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo <= hi):
                    raise ValueError("actuator_randomization[%r]: need finite 0 <= low <= high" % k)
                self._act_rand[k] = (lo, hi)
            self._act_default = self._be.default_env_actuators()
        self._act_rng = np.random.default_rng()

    @staticmethod
    def _check_goals(goals, names, H, W):
        """`goals=` -> a non-empty list of Goal-like objects, checked on the host (before any device is touched): a path is loaded
        like REALRobotEnv.load_goals; every goal needs `final_state` / `initial_state` dicts that name at least one of this env's
        objects in final_state, and a retina -- if it has one -- of this env's camera size.  ValueError otherwise."""
        import os
        if isinstance(goals, (str, bytes, os.PathLike)):
            if not os.path.exists(goals):
                raise ValueError("goals: no goals dataset at %r" % (goals,))
            goals = list(np.load(goals, allow_pickle=True).items())[0][1]
        try:
            goals = list(goals)
        except TypeError:
            raise ValueError("goals must be a path or a list of Goal objects, not %r" % type(goals).__name__)
        if not goals:
            raise ValueError("goals: the goal list is empty")
        for k, g in enumerate(goals):
            fs, ins = getattr(g, 'final_state', None), getattr(g, 'initial_state', None)
            if not isinstance(fs, dict) or not isinstance(ins, dict):
                raise ValueError("goals[%d] is not a Goal (final_state / initial_state dicts expected)" % k)
            if not any(n in names for n in fs):
                raise ValueError("goals[%d] names none of this env's objects (%s) in its final_state" % (k, ', '.join(names)))
            r = getattr(g, 'retina', None)
            if r is not None and np.shape(r) != (H, W, 3):
                raise ValueError("goals[%d].retina has shape %s, this env's camera gives (%d, %d, 3)" % (k, np.shape(r), H, W))
        return goals

    DYNAMICS_FIELDS = ('mass', 'inertia', 'friction', 'restitution', 'rolling', 'spinning')

    def _draw_dynamics(self, mask):
        """Draws new multipliers for the envs in `mask` (bool [N]) and applies them; returns the values in force."""
        n, k = int(mask.sum()), self._be.n_objects
        mult = {f: self._dyn_rng.uniform(*self._dyn_rand[f], size=(n, k)) for f in self.DYNAMICS_FIELDS if f in self._dyn_rand}
        if 'inertia' not in mult and 'mass' in mult:
            mult['inertia'] = mult['mass']
        args = {}
        cur = self._be.object_dynamics()
        for f, m in mult.items():
            v = cur[f].astype(np.float64)
            d = self._dyn_default[f][mask].astype(np.float64)
            v[mask] = d * (m[..., None] if f == 'inertia' else m)
            args[f] = v
        self._be.set_object_dynamics(env_mask=mask.astype(np.uint8), **args)
        return self._be.object_dynamics()

    @staticmethod
    def _rot_zyx(a):
        """R = Rz(a[2]) Ry(a[1]) Rx(a[0]) for rows of angles a [n, 3] (radians) -> [n, 3, 3]."""
        cx, sx, cy, sy, cz, sz = np.cos(a[:, 0]), np.sin(a[:, 0]), np.cos(a[:, 1]), np.sin(a[:, 1]), np.cos(a[:, 2]), np.sin(a[:, 2])
        o, z = np.ones_like(cx), np.zeros_like(cx)
        Rx = np.stack([o, z, z, z, cx, -sx, z, sx, cx], -1).reshape(-1, 3, 3)
        Ry = np.stack([cy, z, sy, z, o, z, -sy, z, cy], -1).reshape(-1, 3, 3)
        Rz = np.stack([cz, -sz, z, sz, cz, z, z, z, o], -1).reshape(-1, 3, 3)
        return Rz @ Ry @ Rx

    def _draw_cameras(self, mask):
        """Draws new cameras for the envs in `mask` (bool [N]) and applies them; returns the matrices in force."""
        cr, n = self._cam_rand, int(mask.sum())
        t = self._cam_rng.uniform(-cr['translation'], cr['translation'], size=(n, 3))
        ang = np.radians(self._cam_rng.uniform(-cr['rotation'], cr['rotation'], size=(n, 3)))
        fov = self._cam_rng.uniform(*cr['fov'], size=n)
        T = np.tile(np.eye(4), (n, 1, 1))
        T[:, :3, :3], T[:, :3, 3] = self._rot_zyx(ang), t
        self._cam_view[mask] = (T @ self._cam_view0).astype(np.float32)
        self._cam_proj[mask] = np.stack([mathutil.perspective(f, self._cam_aspect, 0.1, 100.0) for f in fov]).astype(np.float32) \
            if n else np.zeros((0, 4, 4), np.float32)
        self._be.set_env_cameras(self._cam_view, self._cam_proj, env_mask=mask.astype(np.uint8))
        return {"view": self._cam_view.copy(), "proj": self._cam_proj.copy()}

    def _draw_appearance(self, mask):
        """Draws new colours and lights for the envs in `mask` (bool [N]) and applies them; returns the values in force."""
        ar, n = self._app_rand, int(mask.sum())
        mult = self._app_rng.uniform(*ar['colour'], size=(n,) + self._app_colour0.shape)
        bright = self._app_rng.uniform(*ar['brightness'], size=n)
        ang = np.radians(self._app_rng.uniform(0.0, ar['light'], size=n))
        phi = self._app_rng.uniform(0.0, 2 * np.pi, size=n)
        d = self._app_light0
        u = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        axis = np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * np.cross(d, u)      # unit vectors perpendicular to d
        # Rodrigues' rotation of d about an axis perpendicular to it: d cos a + (axis x d) sin a
        self._app_lights[mask] = (np.cos(ang)[:, None] * d + np.sin(ang)[:, None] * np.cross(axis, d)).astype(np.float32)
        self._app_colours[mask] = (self._app_colour0 * mult * bright[:, None, None]).astype(np.float32)
        self._be.set_env_appearance(colours=self._app_colours, light_dirs=self._app_lights, env_mask=mask.astype(np.uint8))
        return {"colours": self._app_colours.copy(), "light_dirs": self._app_lights.copy()}

    def _draw_actuators(self, mask):
        """Draws new multipliers for the envs in `mask` (bool [N]) and applies them; returns the values in force.  One draw of
        [n, 11] per field, in the order kp, kd, max_force, damping, for the fields that are randomised."""
        n = int(mask.sum())
        args = {}
        cur = self._be.env_actuators()
        for f in nat.ACT_ROW:
            if f in self._act_rand:
                m = self._act_rng.uniform(*self._act_rand[f], size=(n, nat.N_JOINTS))
                v = cur[f].astype(np.float64)
                v[mask] = self._act_default[f][mask].astype(np.float64) * m
                args[f] = v
        self._be.set_env_actuators(env_mask=mask.astype(np.uint8), **args)
        return self._be.env_actuators()

    def _redraw(self, truncated, infos):
        """The domain-randomisation draws of a same-step autoreset: new values for the envs in `truncated`, reported in infos."""
        if self._dyn_rand:
            infos["object_dynamics"] = self._draw_dynamics(truncated)
            infos["_object_dynamics"] = truncated.copy()
        if self._cam_rand:
            infos["camera"] = self._draw_cameras(truncated)
            infos["_camera"] = truncated.copy()
        if self._app_rand:
            infos["appearance"] = self._draw_appearance(truncated)
            infos["_appearance"] = truncated.copy()
        if self._act_rand:
            infos["actuators"] = self._draw_actuators(truncated)
            infos["_actuators"] = truncated.copy()

    # ------------------------------------------------------------------ observations
    def _obs(self, rendered):
        be = self._be
        get = be.device_buffer if self.device_obs else be.host
        obs = {"joint_positions": get(nat.F_JOINTS), "touch_sensors": get(nat.F_TOUCH)}
        if rendered:
            obs["retina"], obs["depth"] = get(nat.F_RGB), get(nat.F_DEPTH)
            if self.additional_obs:
                obs["mask"] = get(nat.F_MASK)
        if self.additional_obs:
            obs["object_positions"] = get(nat.F_OBJ_POSE)
        if self.contact_obs:
            co = be.contact_observations(host=not self.device_obs)
            obs["body_force"], obs["body_partners"] = co["body_force"], co["body_partners"]
        if self.kinematic_obs:
            ko = be.kinematic_observations(host=not self.device_obs)
            for key, name in self.KINEMATIC_KEYS:
                obs[key] = ko[name]
        if self.dynamics_obs:
            pd = be.posture_dynamics(host=not self.device_obs)
            for key in ("mass_matrix", "bias"):       # the present-state form has K = 1: [N, 1, ...] -> [N, ...]
                v = pd[key]
                obs[key] = nat.DeviceBuffer(v.ptr, v.shape[:1] + v.shape[2:], v.typestr, be) if self.device_obs else v[:, 0]
        if self.ray_sensors:
            rc = be.ray_cast(host=not self.device_obs)
            obs["ray_distance"], obs["ray_uid"] = be.ray_column(rc['hit'], 1), be.ray_column(rc['id'], 0)
        if self.pair_distances:
            cp = be.closest_points(host=not self.device_obs)
            obs["pair_distance"], obs["pair_status"] = cp['distance'], cp['status']
        if self._goals is not None:
            if self._goal_images:
                obs["goal"] = be.episode_buffer('goal_rgb', host=not self.device_obs)
            if self.additional_obs:
                obs["goal_positions"] = be.episode_buffer('goal_pos', host=not self.device_obs)
        return obs

    def reset(self, *, seed=None, options=None):
        infos = {}
        if seed is not None:
            self._dyn_rng = np.random.default_rng(seed)
            self._cam_rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(1,)))
            self._app_rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(2,)))
            self._act_rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(3,)))
        if self._dyn_rand:
            infos["object_dynamics"] = self._draw_dynamics(np.ones(self.num_envs, bool))
        if self._cam_rand:
            infos["camera"] = self._draw_cameras(np.ones(self.num_envs, bool))
        if self._app_rand:
            infos["appearance"] = self._draw_appearance(np.ones(self.num_envs, bool))
        if self._act_rand:
            infos["actuators"] = self._draw_actuators(np.ones(self.num_envs, bool))
        self._be.reset()
        if self.macro_replan_on_reset:
            self._be.macro_invalidate()
        self._steps[:] = 0
        if self._goals is not None:
            # env i starts goal i mod G from its start poses (set_goal, env.py:151-166); the first reward is taken against that state
            gi = (np.arange(self.num_envs) % len(self._goals)).astype(np.int32)
            start = self._be.host(nat.F_OBJ_POSE)
            named = (self._g_flags[gi] & nat.GOAL_HAS_START) != 0
            start[named] = self._g_init[gi][named]
            self._be.set_object_poses(start)
            self._be.set_env_goals(gi)
            infos["goal_index"] = gi
        if self.render_every_step:
            self._be.render()
        return self._obs(self.render_every_step), infos

    @staticmethod
    def _action_spaces(robot, num_envs, joint_torque_actions=False, external_wrench_actions=False, action_type='joints'):
        """(single_action_space, action_space) of a vector env over `robot`'s joint command: the batched space is the single one with
        a leading env axis (gymnasium.vector.utils.batch_space); `joint_torque_actions` adds the unbounded "joint_torques" entry,
        `external_wrench_actions` the unbounded "external_wrenches" entry."""
        single = {"joint_command": robot.action_space, "render": spaces.MultiBinary(1)}
        batched = {"joint_command": spaces.Box(low=np.tile(robot.min_joints, (num_envs, 1)), high=np.tile(robot.max_joints, (num_envs, 1)), dtype=float),
                   "render": spaces.MultiBinary(num_envs)}
        if action_type == 'macro_action':      # the reference's macro_space (env.py:49-52) in place of the joint command
            lo, hi = np.array([[-0.25, -0.5], [-0.25, -0.5]]), np.array([[0.05, 0.5], [0.05, 0.5]])
            single = {"macro_action": spaces.Box(low=lo, high=hi, dtype=float), "render": spaces.MultiBinary(1)}
            batched = {"macro_action": spaces.Box(low=np.tile(lo, (num_envs, 1, 1)), high=np.tile(hi, (num_envs, 1, 1)), dtype=float),
                       "render": spaces.MultiBinary(num_envs)}
        if joint_torque_actions:
            single["joint_torques"] = spaces.Box(low=-np.inf, high=np.inf, shape=(nat.N_JOINTS,), dtype=np.float32)
            batched["joint_torques"] = spaces.Box(low=-np.inf, high=np.inf, shape=(num_envs, nat.N_JOINTS), dtype=np.float32)
        if external_wrench_actions:
            single["external_wrenches"] = spaces.Box(low=-np.inf, high=np.inf, shape=(nat.XW_BODIES, 6), dtype=np.float32)
            batched["external_wrenches"] = spaces.Box(low=-np.inf, high=np.inf, shape=(num_envs, nat.XW_BODIES, 6), dtype=np.float32)
        return spaces.Dict(single), spaces.Dict(batched)

    def step(self, actions):
        """actions: float array [N, 9] of joint commands (or a dict with "joint_command" [N, 9], optional "render" and, with
        joint_torque_actions, optional "joint_torques" [N, 11]: absent, the torques in force are kept; with external_wrench_actions,
        optional "external_wrenches" [N, 14, 6], likewise).  With action_type='macro_action': an array [N, 2, 2] of requests, host or
        device (or a dict with "macro_action", optional "macro_idle" [N] and "render")."""
        render = self.render_every_step
        if isinstance(actions, dict):
            render = bool(np.any(actions.get("render", render)))
            if self.joint_torque_actions and actions.get("joint_torques") is not None:
                self._be.set_joint_torques(actions["joint_torques"])
            if self.external_wrench_actions and actions.get("external_wrenches") is not None:
                self._be.set_external_wrenches(actions["external_wrenches"])
            idle = actions.get("macro_idle") if self.action_type == 'macro_action' else None
            actions = actions["macro_action" if self.action_type == 'macro_action' else "joint_command"]
        else:
            idle = None
        if self.action_type == 'macro_action':
            self._be.step_macro_device(actions, idle=idle, render=render)
        else:
            self._be.step(np.asarray(actions, dtype=np.float32), render=render)
        self._steps += 1
        truncated = self._steps >= self.max_episode_steps
        n = self.num_envs
        infos = {}
        if self._goals is not None:
            return self._finish_goal_step(render, truncated, infos)
        if truncated.any():
            # same-step autoreset: keep the finished episodes' last low-dim observation, reset those envs, re-render them
            # (gymnasium's layout: an object array with one dict per finished env and None elsewhere, plus the boolean mask)
            j, tc = self._be.host(nat.F_JOINTS), self._be.host(nat.F_TOUCH)
            op = self._be.host(nat.F_OBJ_POSE) if self.additional_obs else None
            fin = np.full(n, None, dtype=object)
            for i in np.flatnonzero(truncated):
                fin[i] = {"joint_positions": j[i], "touch_sensors": tc[i]}
                if op is not None:
                    fin[i]["object_positions"] = op[i]
            infos["final_obs"] = fin
            infos["_final_obs"] = truncated.copy()
            self._redraw(truncated, infos)
            self._be.reset(truncated.astype(np.uint8))
            if self.macro_replan_on_reset:
                self._be.macro_invalidate(truncated.astype(np.uint8))
            self._steps[truncated] = 0
            if render:
                self._be.render()
        return self._obs(render), np.zeros(n), np.zeros(n, bool), truncated, infos

    def _finish_goal_step(self, render, truncated, infos):
        """The rest of a step() with goals: score, reward and done bits on the device and, on a truncation step, the reset of the
        finished envs into their next goal there (one launch); the host reads back only what it returns as host data."""
        be, n = self._be, self.num_envs
        sweep = bool(truncated.any())
        be.episode_update(reset_done=sweep)
        get = (lambda name: be.episode_buffer(name)) if self.device_obs else (lambda name: be.episode_buffer(name, host=True))
        rewards = get('reward')
        infos["goal_score"] = get('score')
        if sweep:
            # the device reset every env with a done bit: the truncated ones and any the step froze earlier
            truncated = truncated | (be.episode_buffer('done', host=True) != 0)
            fo = be.episode_buffer('final_obs', host=True)
            k = be.n_objects
            fin = np.full(n, None, dtype=object)
            for i in np.flatnonzero(truncated):
                fin[i] = {"joint_positions": fo[i, :9].copy(), "touch_sensors": fo[i, 9:13].copy()}
                if self.additional_obs:
                    fin[i]["object_positions"] = fo[i, 13:13 + 7 * k].reshape(k, 7).copy()
            infos["final_obs"] = fin
            infos["_final_obs"] = truncated.copy()
            self._redraw(truncated, infos)
            if self.macro_replan_on_reset:
                be.macro_invalidate(truncated.astype(np.uint8))
            self._steps[truncated] = 0
            if render:
                be.render()
        infos["goal_index"] = get('goal_index')
        return self._obs(render), rewards, np.zeros(n, bool), truncated, infos

    def close(self, **kwargs):
        self._be.close()
