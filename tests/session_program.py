"""Seeded programmes of API calls for the twin-handle session test (tests/test_gpu_session.py; not collected).

`program(seed, N, nobj, length)` draws a list of op records -- plain data: a kind, masks, indices, values -- as a pure function of its
arguments; nothing here imports torch or the library at module level.  `Session(env, road)` executes records on a handle, `run` a
whole programme.  A record says WHAT changes; the road says HOW the call is made:

    'device'   the device road wherever one exists: device masks, indices, command buffers, state tensors (the default handle A)
    'host'     the host road wherever one exists, and for write_state the matching reset / set_object_poses / state = calls where
               the header (include/realrobot.h, "Equivalences, each bit for bit") names one (the plain-road twin B)
    'written'  as the record says (`device` of the record): the mix a caller would write

Every programme is a chain of units that begin with a mutator:

    pair     mutator, step                 -- the mutator is DIRECTLY followed by a step of a given render form
    pair+    mutator, step, observer       -- ... and the observer stands directly between a step and the next unit's mutator
    triple   mutator, observer, step       -- the observer stands directly between a mutator and a step
    filler   appended to a pair without observer: step_plan, render, a refused step, a further step

`check_conditions` asserts what every programme holds (tests/test_session_program.py).  Masks are never all-clear, and
every written value is a fresh draw, so it differs from what is there.

Values that depend on the handle are kept as recipes and resolved by the Session in float32 on the host, the same for every handle:
object positions are offsets from BASE (where the reference puts cube, tomato, mustard on the table), cameras are eye / target /
field of view, colours a tint per env.

`program(..., queries=True)` draws a QUERY programme instead (sessions q70 and q5; the other programmes are drawn exactly as before,
tests/test_session_program.py pins their digests): the same units, with three more mutators -- set_distance_pairs,
set_kinematic_points, set_rays: the tables of the read-only batch queries are handle state -- and the nine query calls as observers
(Q_OBSERVERS), each record with its own arguments: K in {1, 3, 32} postures (`_Draw.rows()['q']`), segments between two postures, IK
goals (postures whose float64 tool pose at the point in force is the target: a recipe, resolved by `Session.ik_targets`) and seeds.
A query record carries `compared`: True -- the plain-road twin makes the call too, with host arrays, and the result buffers of the
two calls are compared; False -- the call is A's alone.  `check_query_conditions` asserts what a query programme holds.  The Session
keeps the tables it has set (`points`, `max_distance`, `n_rays`) so that the arguments of later calls fit them, and `last`: which
record wrote which result buffers last.  `probe_arguments` are the fixed query arguments of every comparison, `anchor_references`
the float64 restatements on a state that a record itself defines (`is_anchor`).

`program(..., commands=True)` draws a COMMAND programme (sessions c70 and c5; its own generator and rng stream again): the calls that
put per-env command-side state into the handle or launch inside the step.  Ten more mutators (C_MUTATORS) -- the joint torque and
external wrench tables (set, masked and unmasked clearing, `torques_from_dynamics`: the bias of posture_dynamics() fed straight back),
the attachments (given poses, capture, masked detach, the unmasked detach) and macro_invalidate --, one more step kind, `step_macro`
(rr_step_macro: requests held per env, an idle mask, a render form, now and then a NaN or a -0.0), and ten observers (C_OBSERVERS):
posture_dynamics, carried_sweep, the four posture queries that run their `_carry` kernels while attachments are on,
`swept_clearance_refused` and the three table read-backs, each `compared` or silent like a query record.  The Session keeps what the
roads need -- `attached`: the feature is on -- and a pure-numpy MODEL of the macro decision rule of the header (`macro`: record,
position, replanned), which plan_macro, step_plan, step_macro and macro_invalidate move and no state mutator does: A and B both run
k_macro_decide, so the model is the independent reference of that rule.  `check_command_conditions` asserts what a command programme
holds; `command_anchor_references` are the float64 restatements (tests/numpy_dynamics.py, tests/numpy_carry.py) behind the two
anchors, a set_state and a full write_state that each stand directly behind an attach of known poses (`anchor_attach`).
"""
import numpy as np

STEP_KINDS = ('step', 'step_plan', 'render', 'step_refused')
MUTATORS = ('reset_host', 'reset_dev', 'set_state', 'write_state', 'set_object_pose', 'set_object_poses', 'set_object_home',
            'set_object_dynamics', 'set_env_actuators', 'fork_host', 'fork_dev', 'save_snapshot', 'load_snapshot', 'checkpoint',
            'restore', 'plan_macro', 'set_env_goals', 'episode_reset', 'set_camera', 'set_camera_default', 'set_env_cameras',
            'set_env_appearance', 'select_image_mirror')
IMAGE_ONLY = ('set_camera', 'set_camera_default', 'set_env_cameras', 'set_env_appearance', 'select_image_mirror')
OBSERVERS = ('ray_table', 'ray_dev', 'kinematic_observations', 'contact_observations', 'read_state', 'link_poses', 'evaluate_goals',
             'episode_peek', 'contacts', 'sync', 'sync_observations')
RENDER_FORMS = (0, 1, 2)                    # no camera, all envs, per-env flags
# the query programmes (sessions q70, q5): three more mutators -- the tables of the read-only batch queries are handle state -- and
# the nine query calls as observers; `compared` of a query record: B makes the call too (host arrays against A's device tensors)
Q_MUTATORS = ('set_distance_pairs', 'set_kinematic_points', 'set_rays')
Q_OBSERVERS = ('closest_points', 'posture_clearance', 'signed_distance', 'signed_distance_at', 'signed_distance_gradient',
               'swept_clearance', 'posture_kinematics', 'posture_ik', 'posture_ik_present')
STATE_READERS = tuple(k for k in Q_OBSERVERS if k not in ('posture_kinematics', 'posture_ik'))     # (those two read tensors, model, points)
PAIR_READERS = STATE_READERS[:6]            # ... and the pair table
# which result buffers a query call writes: a compared record is judged on these, as its own call left them
FAMILY = {'closest_points': ('dist',), 'posture_clearance': ('pc',), 'signed_distance': ('sd',), 'signed_distance_at': ('sd',),
          'signed_distance_gradient': ('sd', 'sg'), 'swept_clearance': ('sw',), 'posture_kinematics': ('pk',), 'posture_ik': ('pik',),
          'posture_ik_present': ('pik',)}
# a query observer must stand directly behind each of these, with no step between (write_state: a pose part and a joint part)
READ_BEHIND = ('write_state', 'fork_dev', 'load_snapshot', 'reset_dev', 'restore', 'set_object_poses', 'episode_reset',
               'set_distance_pairs', 'set_kinematic_points')
Q_KS, Q_PAIR_CLASSES, Q_RAY_COUNTS = (1, 3, 32), ('one', 'default', 'collision', 'full'), (1, 4, 64)
# the command programmes (sessions c70, c5): ten more mutators, the step kind step_macro, ten observers
C_MUTATORS = ('set_joint_torques', 'set_external_wrenches', 'clear_joint_torques', 'clear_external_wrenches', 'torques_from_dynamics',
              'attach', 'attach_capture', 'detach', 'detach_all', 'macro_invalidate')
C_STEP_KINDS = STEP_KINDS + ('step_macro',)
CARRY_QUERIES = ('posture_clearance', 'signed_distance', 'signed_distance_at', 'signed_distance_gradient')     # (_carry kernels while attached)
C_OBSERVERS = ('posture_dynamics', 'carried_sweep') + CARRY_QUERIES + ('swept_clearance_refused', 'joint_torques', 'external_wrenches',
                                                                       'attachments')
FAMILY.update({'posture_dynamics': ('pd',), 'torques_from_dynamics': ('pd',), 'carried_sweep': ('sw',), 'swept_clearance_refused': (),
               'joint_torques': (), 'external_wrenches': (), 'attachments': ()})
# the state mutators whose interplay with the tables, the attachments and the macro record the header fixes (state_kind(op))
STATE_MUTATORS = ('reset_dev', 'fork_dev', 'load_snapshot', 'restore', 'episode_reset', 'set_state', 'write_joints', 'write_poses')
CAPTURE_BEHIND = ('fork_dev', 'load_snapshot', 'reset_dev', 'restore', 'write_joints')     # ... and a step
N_WRENCH_ROWS = 14                          # (RR_XW_BODIES: eleven robot bodies, three objects)
MACRO_LO, MACRO_HI = np.array([-0.25, -0.5, -0.25, -0.5], np.float32), np.array([0.05, 0.5, 0.05, 0.5], np.float32)      # (plan_macro's draws)
PLAN_LEN = 1000

# the sessions of tests/test_gpu_session.py: name -> (seed, N, objects, width, height, ops); the seed was fixed once, for the
# coverage the device reports (NOTEBOOK.md), and is never changed to make a comparison pass
Q_LENGTH = 74                               # what the conditions of a query programme cost (below)
C_LENGTH = 212                           # what the conditions of a command programme cost (the comment at C_MIN_LENGTH)
SESSIONS = {'n70': (20261, 70, 3, 64, 64, 200), 'n5': (20262, 5, 1, 96, 64, 200), 'n1100': (20263, 1100, 3, 32, 32, 200),
            'q70': (20264, 70, 3, 64, 64, Q_LENGTH), 'q5': (20265, 5, 1, 96, 64, Q_LENGTH),
            'c70': (20266, 70, 3, 64, 64, C_LENGTH), 'c5': (20267, 5, 1, 96, 64, C_LENGTH)}
QUERY_SESSIONS = ('q70', 'q5')              # drawn with program(..., queries=True)
COMMAND_SESSIONS = ('c70', 'c5')            # drawn with program(..., commands=True)

# What a programme holds, whatever its size (check_conditions): M = 23 mutator kinds, O = 11 observer kinds; a pair costs 2 ops, a
# triple 3, an observer behind a pair 1.  Every mutator 3 times in pairs, once with each render form (138); every observer behind a
# pair (11) and in a triple (33) whose mutator is a write_state; five more write_state pairs (10), so that write_state occurs 19
# times: once with each of the 16 subsets of the column groups (the empty one with reset or fresh alone) and the three forms the
# header names bitwise equal to host calls; one launch (2): a write that throws an object out of bounds within one step, in front of
# a set_object_home.  194 ops; the rest are fillers.
MIN_LENGTH = 200
# A query programme holds other conditions (check_query_conditions).  Pairs (2 ops): each of the three table mutators with each render
# form (18) -- two of the set_distance_pairs put the default table of `Session.setup` back in force and are glued in front of the two
# anchors, a set_state and a full write_state, whose state is known on the CPU (4) --, a checkpoint and a save_snapshot (4).  Triples
# (3 ops), a query observer directly between a mutator and a step: one behind each of write_state (object poses), fork_dev,
# load_snapshot, reset_dev, restore, set_object_poses, episode_reset -- the seven state readers, rotated by the seed --, two behind a
# set_distance_pairs, three behind a set_kinematic_points (posture_ik without seeds, posture_kinematics, posture_ik), and the last
# unit: write_state (joint positions) -- posture_ik without seeds (39).  Every query observer once more behind a pair, directly in
# front of the next unit's mutator (9).  74 ops; a longer programme gets further steps.
Q_MIN_LENGTH = Q_LENGTH
# A command programme holds the conditions of check_command_conditions, and they cost more than a query programme's: a mutator needs
# a step of its own directly behind it, so every condition of the form "X directly followed by a step" is a pair of two ops that
# nothing else can share.  In the order of _command_program: plan_macro and four step_macro with the same requests (5); both tables,
# the attachments, a snapshot and two checkpoints, each with its step (12); the eight state mutators with everything on, each
# directly behind the step_macro of a new mutator and in front of a step (8 x 4, and the carry query of the attach_capture: 33), once
# more with a step_macro behind them (16); attach_capture with its carry query behind five of them (20) and a carry query alone behind
# the same five (15); the other render forms of the ten new mutators with torques_from_dynamics behind a fork (7 + 8 + 8), of
# macro_invalidate with the second plan_macro, a step_plan and a step_macro (10), of detach and detach_all with the attach calls that
# turn the feature on again and the two anchors with their attach (24); the three unmasked clearing calls and the eight state mutators
# with everything off (22): 180 ops.  32 observers behind steps, so that each of the ten kinds is made both compared and silent, the
# sweeps with attachments on and off: 212 ops, about three query programmes; a longer programme gets further steps.
C_MIN_LENGTH = C_LENGTH
# collision shapes of the model by name (BatchedREALRobotEnv.collision_shapes; tests/test_session_program.py asserts the list)
ROBOT_SHAPES = ('lbr_iiwa_link_1', 'lbr_iiwa_link_2', 'lbr_iiwa_link_3', 'lbr_iiwa_link_4', 'lbr_iiwa_link_5', 'lbr_iiwa_link_6',
                'lbr_iiwa_link_7', 'base', 'finger_00', 'finger_01', 'skin_01', 'skin_00', 'finger_10', 'finger_11', 'skin_11', 'skin_10')
STATIC_SHAPES = ('table', 'shelf', 'robot_base')
OBJECT_SHAPES = ('cube', 'tomato', 'mustard')
N_LINKS, FINGER_LINKS, ARM_LINKS = 17, tuple(range(9, 17)), tuple(range(1, 7))      # (LINK_NAMES: 9.. the gripper's; 1..6 below joint 7)
PROBE_K, PROBE_ITERATIONS, PROBE_MARGIN = 2, 8, 0.25


def default_pairs(nobj):
    """the pair table of `Session.setup`, by name: robot-object, robot-static, robot-robot, object-object, object-static; the
    objects are those the handle has (with fewer than three, a missing one is replaced by one it has; doubles are dropped)"""
    o = [OBJECT_SHAPES[i % nobj] for i in range(3)]
    pairs = [('skin_00', o[0]), ('finger_01', o[2]), ('lbr_iiwa_link_6', o[1]), ('skin_10', o[0]), ('finger_00', 'shelf'),
             ('lbr_iiwa_link_7', 'table'), ('lbr_iiwa_link_5', 'table'), ('lbr_iiwa_link_7', 'robot_base'),
             ('lbr_iiwa_link_3', 'lbr_iiwa_link_6'), (o[0], o[1]), (o[1], o[2]), (o[0], 'table'), (o[1], 'table'), (o[2], 'shelf')]
    out = []
    for p in pairs:
        if p[0] != p[1] and p not in out:
            out.append(p)
    return out

BASE = np.array([[-0.1, 0.0, 0.45], [-0.1, -0.3, 0.45], [-0.1, 0.3, 0.45]], np.float32)      # cube, tomato, mustard (robot.py:19-24)
CMD_LO = np.array([-2.09, -2.09, -2.96, -2.09, -2.96, -2.09, -3.05, 0.0, 0.0], np.float32)
CMD_HI = np.array([2.09, 2.09, 2.96, 2.09, 2.96, 2.09, 3.05, 1.5708, 1.5708], np.float32)
N_WORLD_RAYS, N_LINK_RAYS = 3, 1            # the ray table of `setup`: three world rays down onto the table, one along the gripper
N_GOALS, HORIZON, GOAL_STRIDE, N_SLOTS = 5, 12, 2, 2      # the warm-up leaves every clock at 60: an auto-reset takes every env that the
                                                         # programme has not reset in its last 12 steps
W_JOINT_POS, W_JOINT_VEL, W_OBJ_POSE, W_OBJ_VEL = 1, 2, 4, 8


class _Draw:
    """the value draws of one programme"""

    def __init__(self, rng, N, nobj, salt=0):
        self.rng, self.N, self.nobj, self.salt = rng, N, nobj, salt
        self.cmd = rng.uniform(CMD_LO, CMD_HI, (N, 9)).astype(np.float32)
        self.sel = 7
        self.n_write = 0
        self.n_points = self.n_rays = self.n_query = 0
        self.n_kind = {}

    def mask(self):
        """uint8 [N], never all-clear, not all-set when N > 1; set bytes are any non-zero value"""
        N, rng = self.N, self.rng
        m = rng.random(N) < rng.uniform(0.25, 0.6)
        m[rng.integers(N)] = True
        if N > 1 and m.all():
            m[rng.integers(N)] = False
        return (m * rng.integers(1, 256, N)).astype(np.uint8)

    def command(self):
        """resample-and-hold: a tenth of the envs take a new command"""
        N, rng = self.N, self.rng
        new = rng.random(N) < 0.1
        self.cmd = np.where(new[:, None], rng.uniform(CMD_LO, CMD_HI, (N, 9)).astype(np.float32), self.cmd)
        return self.cmd.copy()

    def render(self, form):
        return dict(render=form, flags=np.minimum(self.mask(), 1) if form == 2 else None)

    def rows(self):
        """recipe of a state [N, 61]: joints, joint velocities, per object an offset from BASE, a unit quaternion and a twist"""
        N, rng = self.N, self.rng
        q = np.empty((N, 11), np.float32)
        q[:, :7] = rng.uniform(-0.8, 0.8, (N, 7))
        q[:, [7, 9]] = rng.uniform(0.0, 1.0, (N, 2))
        q[:, [8, 10]] = rng.uniform(-1.0, 0.0, (N, 2))
        quat = rng.normal(size=(N, 3, 4))
        quat = (quat / np.linalg.norm(quat, axis=-1, keepdims=True)).astype(np.float32)
        off = rng.uniform([-0.08, -0.08, 0.03], [0.08, 0.08, 0.15], (N, 3, 3)).astype(np.float32)
        return dict(q=q, qd=rng.uniform(-0.3, 0.3, (N, 11)).astype(np.float32), off=off, quat=quat,
                    twist=rng.uniform(-0.2, 0.2, (N, 3, 6)).astype(np.float32))

    def index(self, keep=True):
        """source index [N] of a fork: a swap, a cycle, a self copy, kept envs, a broadcast, a seeded draw for the rest"""
        N, rng = self.N, self.rng
        idx = rng.integers(-1 if keep else 0, N, N).astype(np.int32)
        if N >= 2:
            idx[0], idx[1] = 1, 0
        if N >= 5:
            idx[2], idx[3], idx[4] = 3, 4, 2
        if N >= 16:
            idx[8] = 8
            if keep:
                idx[9:12] = -1
            idx[12:16] = rng.integers(N)
        return idx

    def mutator(self, kind):
        N, nobj, rng = self.N, self.nobj, self.rng
        op = dict(kind=kind)
        if kind in ('reset_host', 'reset_dev'):
            op.update(mask=self.mask(), device=kind == 'reset_dev')
        elif kind == 'set_state':
            op.update(rows=self.rows())
        elif kind == 'write_state':
            k = self.n_write
            self.n_write += 1
            k %= 19
            if k < 16:                      # every subset of the column groups; reset / fresh rotate with the programme's salt
                c = (k + self.salt) % 4
                parts, reset, fresh = k, bool(c & 1), bool(c & 2)
                reset = reset or (parts == 0 and not fresh)
            else:                           # the forms the header names bitwise equal to rr_set_object_poses, the auto-reset's pair, rr_set_state
                parts, reset, fresh = ((W_OBJ_POSE, False, False), (W_OBJ_POSE, True, False), (15, False, True))[k - 16]
            op.update(parts=parts, reset=reset, fresh=fresh, rows=self.rows(), mask=None if k == 18 or k % 5 == 4 else self.mask())
        elif kind == 'set_object_pose':
            r = self.rows()
            e, o = int(rng.integers(N)), int(rng.integers(nobj))
            op.update(env=e, obj=o, off=r['off'][e, o], quat=r['quat'][e, o])
        elif kind == 'set_object_poses':
            op.update(mask=self.mask(), rows=self.rows())
        elif kind == 'set_object_home':
            r = self.rows()
            e, o = int(rng.integers(N)), int(rng.integers(nobj))
            op.update(env=None if rng.random() < 0.3 else e, obj=o, off=r['off'][e, o] * np.float32(0.5), quat=r['quat'][e, o])
        elif kind == 'set_object_dynamics':
            op.update(mask=self.mask(), mass=rng.uniform(0.3, 1.5, (N, nobj)).astype(np.float32),
                      friction=rng.uniform(0.3, 1.0, (N, nobj)).astype(np.float32))
        elif kind == 'set_env_actuators':
            op.update(mask=self.mask(), kp=rng.uniform(0.05, 0.2, (N, 1)).astype(np.float32),
                      max_force=rng.uniform(200.0, 1000.0, (N, 1)).astype(np.float32),
                      damping=rng.uniform(0.0, 0.5, (N, 11)).astype(np.float32))      # (the damping is what the look-ahead has used)
        elif kind in ('fork_host', 'fork_dev'):
            op.update(index=self.index(), device=kind == 'fork_dev')
        elif kind == 'save_snapshot':
            op.update(slot=int(rng.integers(N_SLOTS)), index=None if rng.random() < 0.5 else self.index(), device=bool(rng.integers(2)))
        elif kind == 'load_snapshot':
            op.update(slot=int(rng.integers(N_SLOTS)), index=None if rng.random() < 0.3 else self.index(), device=bool(rng.integers(2)))
        elif kind == 'plan_macro':
            macro = np.empty((N, 2, 2), np.float32)
            macro[..., 0] = rng.uniform(-0.25, 0.05, (N, 2))
            macro[..., 1] = rng.uniform(-0.5, 0.5, (N, 2))
            op.update(mask=self.mask(), macro=macro)
        elif kind == 'set_env_goals':
            op.update(mask=self.mask(), index=rng.integers(-1, N_GOALS, N).astype(np.int32))
        elif kind == 'set_camera':
            op.update(eye=rng.uniform([0.2, -0.4, 0.7], [0.5, 0.4, 1.2]), target=rng.uniform([-0.15, -0.1, 0.3], [0.05, 0.1, 0.5]),
                      fov=float(rng.uniform(60.0, 90.0)))
        elif kind == 'set_env_cameras':
            op.update(mask=self.mask(), eye=rng.uniform([0.2, -0.4, 0.7], [0.5, 0.4, 1.2], (N, 3)),
                      target=rng.uniform([-0.15, -0.1, 0.3], [0.05, 0.1, 0.5], (N, 3)), fov=rng.uniform(60.0, 90.0, N))
        elif kind == 'set_env_appearance':
            light = rng.normal(size=(N, 3))
            light[:, 2] = np.abs(light[:, 2]) + 0.5
            op.update(mask=self.mask(), tint=rng.uniform(0.1, 1.0, (N, 3)).astype(np.float32), light=light.astype(np.float32))
        elif kind == 'select_image_mirror':
            sel = int(rng.integers(0, 8))
            if sel == self.sel:
                sel ^= int(rng.choice([1, 2, 4]))
            self.sel = sel
            op.update(sel=sel)
        elif kind == 'set_distance_pairs':          # (a query programme passes `pairs=` itself: the class of the table)
            raise AssertionError("set_distance_pairs is drawn by table()")
        elif kind == 'set_kinematic_points':
            P = int(rng.integers(1, 9))
            links = rng.integers(1, N_LINKS, P)
            n = self.n_points
            self.n_points += 1
            finger, arm = FINGER_LINKS[int(rng.integers(len(FINGER_LINKS)))], ARM_LINKS[int(rng.integers(len(ARM_LINKS)))]
            if P == 1:                              # the last point is the IK's: a finger link and a link below joint 7 take turns
                links[0] = arm if n % 2 else finger
            else:
                links[P - 1], links[P - 2] = (arm, finger) if n % 2 else (finger, arm)
            local = rng.uniform(0.01, 0.1, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))
            op.update(links=links.astype(np.int32), local=local.astype(np.float32))
        elif kind == 'set_rays':
            R = int(Q_RAY_COUNTS[(self.n_rays + self.salt) % 3])
            self.n_rays += 1
            links = np.where(rng.random(R) < 0.5, -1, rng.integers(0, N_LINKS, R)).astype(np.int32)
            if R > 1:
                links[0], links[1] = -1, 8          # a world ray and a ray of the gripper base, whatever the draw
            seg = np.zeros((R, 6), np.float32)
            xy = rng.uniform([-0.3, -0.45], [0.2, 0.45], (R, 2))
            seg[:, 0:2], seg[:, 3:5], seg[:, 2], seg[:, 5] = xy, xy + rng.uniform(-0.1, 0.1, xy.shape), 1.0, 0.2
            local = links >= 0
            seg[local, :3] = 0.0
            seg[local, 3:] = rng.uniform([-0.1, -0.1, 0.2], [0.1, 0.1, 0.5], (int(local.sum()), 3))
            op.update(links=links, segments=seg)
        # checkpoint, restore, episode_reset, set_camera_default: the kind says it all
        return op

    def table(self, cls):
        """a set_distance_pairs record of class `cls`: 'default' (the table of Session.setup, no cull), 'one' pair, the step's own
        'collision' table, or 'full': 96 pairs; pairs by name, only of objects the handle has; the others with or without a cull"""
        rng, nobj = self.rng, self.nobj
        md = None if cls == 'default' or rng.random() < 0.4 else float(np.float32(rng.uniform(0.05, 0.25)))
        if cls == 'default':
            pairs = default_pairs(nobj)
        elif cls == 'collision':
            pairs = 'collision'
        else:
            names = ROBOT_SHAPES + STATIC_SHAPES + OBJECT_SHAPES[:nobj]
            pairs = []
            while len(pairs) < (1 if cls == 'one' else 96):
                a, b = (int(i) for i in rng.integers(len(names), size=2))
                if a != b and not (a >= len(ROBOT_SHAPES) and b >= len(ROBOT_SHAPES) and max(a, b) < len(ROBOT_SHAPES) + 3):      # (not two statics)
                    pairs.append((names[a], names[b]))
        return dict(kind='set_distance_pairs', cls=cls, pairs=pairs, max_distance=md)

    def postures(self, K):
        """float32 [N, K, 11], every [:, k] a draw of rows()['q']"""
        return np.ascontiguousarray(np.stack([self.rows()['q'] for _ in range(K)], axis=1))

    def query(self, kind, compared):
        """a query observer's record: K cycles through {1, 3, 32}; postures as rows()['q'], segments between two of them, IK goals
        such postures (the Session turns them into tool poses at the point in force) and seeds the goals plus U(-0.3, 0.3)"""
        rng = self.rng
        op = dict(kind=kind, compared=bool(compared))
        if kind in ('closest_points', 'signed_distance'):
            return op
        K = int(Q_KS[(self.n_query + self.salt) % 3])
        self.n_query += 1
        family = 'ik' if kind.startswith('posture_ik') else kind
        n = self.n_kind[family] = self.n_kind.get(family, -1) + 1      # safety, margin, position_only and clamp take turns
        if kind in ('posture_clearance', 'signed_distance_at', 'posture_kinematics'):
            op.update(postures=self.postures(K))
        elif kind == 'signed_distance_gradient':
            op.update(postures=self.postures(K), margin=float(np.float32((0.03, 0.3, 0.0)[n % 3])))
        elif kind == 'swept_clearance':
            op.update(segments=np.ascontiguousarray(np.stack([self.postures(K), self.postures(K)], axis=2)),
                      safety=float(np.float32((0.0, 0.01, 0.04)[n % 3])))
        else:
            goals = self.postures(K)
            op.update(goals=goals, position_only=bool(n & 1), clamp=not n & 2,
                      max_iterations=int(rng.choice([4, 16, 32])))
            if kind == 'posture_ik':
                seeds = goals.copy()
                seeds[..., :7] += rng.uniform(-0.3, 0.3, seeds[..., :7].shape).astype(np.float32)
                op.update(seeds=seeds)
        return op

    def launch(self, env, obj):
        """a write_state of one env that puts object `obj` 1.5 m in front of the table, 5 mm above the height below which the
        out-of-bounds rule fires there (x > 0.11 and z < 0.29, env.py:257-264), falling at 5 m/s: out of bounds behind one step"""
        rows = self.rows()
        rows['off'][env, obj] = np.array([1.5, 0.0, 0.295], np.float32) - BASE[obj]
        rows['twist'][env, obj] = np.array([0, 0, -5.0, 0, 0, 0], np.float32)
        mask = np.zeros(self.N, np.uint8)
        mask[env] = 1
        return dict(kind='write_state', parts=W_OBJ_POSE | W_OBJ_VEL, reset=False, fresh=False, rows=rows, mask=mask)

    def observer(self, kind):
        N, nobj, rng = self.N, self.nobj, self.rng
        op = dict(kind=kind)
        if kind == 'ray_dev':
            seg = np.empty((N, N_WORLD_RAYS + N_LINK_RAYS, 6), np.float32)
            xy = rng.uniform([-0.3, -0.45], [0.2, 0.45], (N, N_WORLD_RAYS, 2))
            seg[:, :N_WORLD_RAYS, 0:2] = xy
            seg[:, :N_WORLD_RAYS, 3:5] = xy + rng.uniform(-0.1, 0.1, xy.shape)
            seg[:, :N_WORLD_RAYS, 2], seg[:, :N_WORLD_RAYS, 5] = 1.0, 0.2
            seg[:, N_WORLD_RAYS:, :3] = 0.0
            seg[:, N_WORLD_RAYS:, 3:] = rng.uniform([-0.1, -0.1, 0.2], [0.1, 0.1, 0.5], (N, N_LINK_RAYS, 3))
            op.update(segments=seg)
        elif kind == 'evaluate_goals':
            pos = (BASE[:nobj] + rng.uniform(-0.1, 0.1, (N, nobj, 3))).astype(np.float32)
            gm = (rng.random((N, nobj)) < 0.7).astype(np.uint8)
            op.update(goal_pos=pos, goal_mask=None if rng.random() < 0.3 else gm)
        elif kind == 'contacts':
            op.update(env=int(rng.integers(N)))
        return op

    def step(self, form, device=None):
        op = dict(kind='step', cmd=self.command(), device=bool(self.rng.integers(2)) if device is None else device)
        op.update(self.render(form))
        return op

    def filler(self, what, form):
        if what == 'step_plan':
            op = dict(kind='step_plan', idle=np.minimum(self.mask(), 1))
        elif what == 'render':
            return dict(kind='render')
        elif what == 'step_refused':
            cmd = self.command()
            bad = self.mask() != 0
            cmd[bad, self.rng.integers(9)] = np.nan if self.rng.random() < 0.5 else np.inf
            op = dict(kind='step_refused', cmd=cmd, refused=bad, device=bool(self.rng.integers(2)))
        else:
            return self.step(form)
        op.update(self.render(form))
        return op


def _units(rng):
    """the units of a programme as (mutator, observer before the step or None, render form, observer behind the step or None, launch)"""
    obs = list(OBSERVERS)
    units = []
    for f in RENDER_FORMS:
        units += [[m, None, f, None, m == 'set_object_home' and f == 0] for m in MUTATORS]
    units += [['write_state', None, int(rng.integers(3)), None, False] for _ in range(5)]       # 3 + 11 + 5 = 19 write_states
    units += [['write_state', o, int(rng.integers(3)), None, False] for o in obs]
    pairs = [u for u in units if u[1] is None]                                                  # every observer once behind a pair
    for o, k in zip(obs, rng.permutation(len(pairs))):
        pairs[k][3] = o
    return [tuple(u) for u in units]


def _ordered(units, rng):
    """a seeded order in which every unit finds what it needs: a restore a checkpoint of the programme behind the one of the set-up
    (it takes the checkpoint before last), an auto-reset a device reset (so that it finds young clocks), and the last restore and the
    last load_snapshot a fork and a device reset before them"""
    units = [units[i] for i in rng.permutation(len(units))]
    last = {k: max((i for i, u in enumerate(units) if u[0] == k), default=None) for k in ('restore', 'load_snapshot')}
    guarded = {id(units[i]) for i in last.values() if i is not None}
    out, seen = [], set()
    while units:
        for j, u in enumerate(units):
            need = set()
            if u[0] == 'restore':
                need.add('checkpoint')
            if u[0] == 'episode_reset':
                need.add('reset_dev')       # envs with a young clock: the auto-reset takes a part of the batch
            if id(u) in guarded:
                need |= {'fork', 'reset_dev'}
            if need <= seen:
                break
        else:
            raise AssertionError("no unit can go next")
        u = units.pop(j)
        out.append(u)
        seen.add('fork' if u[0].startswith('fork') else u[0])
    if out[-1][3] is not None:              # an observer behind the last step would stand in front of no mutator: an earlier pair takes it
        k = next(i for i in range(len(out) - 2, -1, -1) if out[i][3] is None and out[i][1] is None)
        out[k], out[-1] = out[k][:3] + (out[-1][3], out[k][4]), out[-1][:3] + (None, out[-1][4])
    return out


def _query_program(seed, N, nobj, length):
    """a query programme (the comment at Q_MIN_LENGTH): its own generator, so that the draws of the other programmes stay as they are"""
    if length < Q_MIN_LENGTH:
        raise ValueError("a query programme needs at least %d ops" % Q_MIN_LENGTH)
    rng = np.random.default_rng([int(seed), int(N), int(nobj), int(length), 1])
    salt = int(seed) % 7

    def unit(mut, form=None, before=None, **kw):
        return dict(mut=mut, form=int(rng.integers(3)) if form is None else int(form), before=before, behind=None, glue=None, fill=0, **kw)
    forms = [int(f) for f in rng.permutation(3)]
    classes = [str(c) for c in rng.permutation(['one', 'collision', 'full'])]
    anchors = [unit('set_state'), unit('write_state', parts=15)]
    glued = [dict(unit('set_distance_pairs', forms[k], cls='default'), glue=anchors[k]) for k in range(2)]
    pairs = [unit('set_distance_pairs', forms[2], cls=classes[0])]
    pairs += [unit(m, f) for m in ('set_kinematic_points', 'set_rays') for f in RENDER_FORMS]
    pairs += [unit('checkpoint'), unit('save_snapshot')]
    behind_state = ('write_state', 'fork_dev', 'load_snapshot', 'reset_dev', 'restore', 'set_object_poses', 'episode_reset')
    triples = [unit(m, before=STATE_READERS[(i + salt) % 7], **({'parts': W_OBJ_POSE} if m == 'write_state' else {})) for i, m in enumerate(behind_state)]
    triples += [unit('set_distance_pairs', before=PAIR_READERS[(salt + 3 * k) % 6], cls=classes[1 + k]) for k in range(2)]
    triples += [unit('set_kinematic_points', before=o) for o in ('posture_ik_present', 'posture_kinematics', 'posture_ik')]
    last = unit('write_state', before='posture_ik_present', parts=W_JOINT_POS)
    hosts = pairs + anchors                   # every query observer once behind a pair, in front of the next unit's mutator
    for o, k in zip(Q_OBSERVERS, rng.permutation(len(hosts))):
        hosts[k]['behind'] = o
    for _ in range(length - Q_MIN_LENGTH):
        pairs[int(rng.integers(len(pairs)))]['fill'] += 1
    todo = glued + pairs + triples
    todo = [todo[i] for i in rng.permutation(len(todo))]
    need = {'restore': 'checkpoint', 'load_snapshot': 'save_snapshot', 'episode_reset': 'reset_dev'}
    order, seen = [], set()
    while todo:
        j = next(j for j, u in enumerate(todo) if need.get(u['mut']) is None or need[u['mut']] in seen)
        u = todo.pop(j)
        order += [u] + ([u['glue']] if u['glue'] else [])
        seen.add(u['mut'])
    order.append(last)
    draw = _Draw(rng, N, nobj, salt=int(seed) % 4)
    ops, n_seen, slot = [], {}, 0

    def query(kind):
        n = n_seen[kind] = n_seen.get(kind, 0) + 1
        return draw.query(kind, (n + Q_OBSERVERS.index(kind) + salt) % 2 == 0)
    for u in order:
        mut = u['mut']
        if mut == 'set_distance_pairs':
            op = draw.table(u['cls'])
        elif mut == 'write_state':
            full = u['parts'] == 15
            op = dict(kind=mut, parts=u['parts'], reset=False, fresh=full, rows=draw.rows(), mask=None if full else draw.mask())
        else:
            op = draw.mutator(mut)
        if mut == 'save_snapshot':
            slot = op['slot']
        elif mut == 'load_snapshot':
            op['slot'] = slot               # (a slot that has been saved)
        ops.append(op)
        if u['before'] is not None:
            ops.append(query(u['before']))
        ops.append(draw.step(u['form']))
        ops += [draw.step(int(rng.integers(3))) for _ in range(u['fill'])]
        if u['behind'] is not None:
            ops.append(query(u['behind']))
    assert len(ops) == length, (len(ops), length)
    return ops


# ------------------------------------------------------------------------------------------------------- the command programmes
class MacroModel:
    """The decision rule of rr_step_macro as the header states it (include/realrobot.h, "Device-resident macro actions"), in numpy:
    the request record f32 [N, 4] (NaN on creation), the plan position i32 [N], shared with rr_plan_macro (position 0 for a planned
    env) and rr_step_plan* (a non-idle env advances), and `replanned` u8 [N] of the last step_macro.  No state mutator moves any of
    them.  float32 ==: -0.0 equals 0.0, a NaN equals nothing."""

    def __init__(self, N):
        self.record = np.full((N, 4), np.nan, np.float32)
        self.position = np.zeros(N, np.int32)
        self.replanned = np.zeros(N, np.uint8)

    @staticmethod
    def _on(mask, N):
        return np.ones(N, bool) if mask is None else np.asarray(mask) != 0

    def plan(self, mask):
        self.position[self._on(mask, len(self.position))] = 0

    def step_plan(self, idle):
        self.position[np.ones(len(self.position), bool) if idle is None else np.asarray(idle) == 0] += 1

    def invalidate(self, mask):
        self.record[self._on(mask, len(self.position))] = np.nan

    def step_macro(self, macro, idle):
        macro = np.asarray(macro, np.float32).reshape(-1, 4)
        act = np.ones(len(macro), bool) if idle is None else np.asarray(idle) == 0
        same = (macro == self.record).all(axis=1)
        need = act & (~same | (self.position >= PLAN_LEN))
        self.record[need] = macro[need]
        self.position[need] = 0
        self.replanned = need.astype(np.uint8)
        self.position[act] += 1
        return need

    def apply(self, op):
        """the four kinds of record that move the model; every other record leaves it alone"""
        k = op['kind']
        if k == 'plan_macro':
            self.plan(op['mask'])
        elif k == 'step_plan':
            self.step_plan(op.get('idle'))
        elif k == 'step_macro':
            self.step_macro(op['macro'], op['idle'])
        elif k == 'macro_invalidate':
            self.invalidate(op['mask'])


def state_kind(op):
    """the kind of a state mutator of STATE_MUTATORS ('write_joints' / 'write_poses': a masked write_state of that column group
    alone), else None"""
    k = op['kind']
    if k == 'write_state':
        return {W_JOINT_POS: 'write_joints', W_OBJ_POSE: 'write_poses'}.get(op['parts']) if op['mask'] is not None and not op['fresh'] and not op['reset'] else None
    return k if k in STATE_MUTATORS else None


class Situation:
    """What a command programme has set so far, from its records alone: which envs have a non-zero row in either table, whether the
    features are on, which envs carry something, and the macro model.  Forks, resets, writes, snapshot loads and restores leave all
    of it with the env, as the header says, so no state mutator appears here."""

    def __init__(self, N):
        self.N = N
        self.t_nz, self.w_nz, self.att = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
        self.t_on = self.w_on = self.attached = False
        self.macro = MacroModel(N)

    def apply(self, op):
        k = op['kind']
        m = MacroModel._on(op.get('mask'), self.N)
        if k == 'set_joint_torques':
            self.t_nz[m], self.t_on = (op['torques'][m] != 0).any(axis=1), True
        elif k == 'torques_from_dynamics':
            self.t_nz[m], self.t_on = True, True          # (the gravity torques of an arm that is not folded onto its axis)
        elif k == 'set_external_wrenches':
            self.w_nz[m], self.w_on = (op['wrenches'][m] != 0).reshape(int(m.sum()), -1).any(axis=1), True
        elif k == 'clear_joint_torques':
            self.t_nz[m], self.t_on = False, self.t_on and op['mask'] is not None
        elif k == 'clear_external_wrenches':
            self.w_nz[m], self.w_on = False, self.w_on and op['mask'] is not None
        elif k in ('attach', 'attach_capture'):
            self.att[m], self.attached = (op['links'][m] >= 0).any(axis=1), True
        elif k == 'detach':
            self.att[m] = False
        elif k == 'detach_all':
            self.att[:], self.attached = False, False
        self.macro.apply(op)

    def tables(self):
        return bool(self.t_nz.any() and self.w_nz.any())

    def carrying(self):
        return bool(self.attached and self.att.any())

    def in_flight(self):
        return bool(((self.macro.position > 0) & ~np.isnan(self.macro.record).any(axis=1)).any())

    def all_off(self):
        return not (self.t_on or self.w_on or self.attached)


ANCHOR_SALT = 0                             # moved on the CPU until the float64 reference decides every anchor item (test_the_command_anchors_are_decided)


def anchor_attach(N, nobj, which):
    """the attach record in force at anchor `which` (0: the set_state, 1: the full write_state): every env, poses given.  Object o of
    env e hangs on a finger link or on a link below joint 7, 20 to 30 cm from that link's frame; every third (env, object) is free."""
    rng = np.random.default_rng([96, int(N), int(nobj), int(which), ANCHOR_SALT])
    pool = np.array(FINGER_LINKS + ARM_LINKS, np.int32)
    links = pool[rng.integers(len(pool), size=(N, nobj))].astype(np.int32)
    links[(np.arange(N)[:, None] + np.arange(nobj)[None, :] + which) % 3 == 2] = -1
    v = rng.normal(size=(N, nobj, 3))
    rel = np.zeros((N, nobj, 7), np.float32)
    rel[..., :3] = v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.2, 0.3, (N, nobj, 1))
    quat = rng.normal(size=(N, nobj, 4))
    rel[..., 3:] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    return dict(kind='attach', links=links, rel=rel, mask=None, anchor=True)


def is_command_anchor(op):
    """a set_state or full write_state of a command programme that stands directly behind its `anchor_attach`"""
    return bool(op.get('anchor')) and is_anchor(op)


class _CDraw(_Draw):
    """the value draws of a command programme"""

    def __init__(self, rng, N, nobj, salt=0):
        super().__init__(rng, N, nobj, salt)
        self.req = self.requests(N)
        self.req[0, 1] = 0.0                # (a component that is exactly 0.0, whatever the draw)
        self.n_macro = self.n_pd = self.n_sweep = 0
        self.n_seen = {}

    def requests(self, n):
        """n requests in the range of plan_macro's draws; about one in six has a component that is exactly 0.0"""
        rng = self.rng
        r = rng.uniform(MACRO_LO, MACRO_HI, (n, 4)).astype(np.float32)
        zero = np.flatnonzero(rng.random(n) < 1 / 6)
        r[zero, rng.integers(4, size=len(zero))] = 0.0
        return r

    def compared(self, kind):
        n = self.n_seen[kind] = self.n_seen.get(kind, 0) + 1
        return (n + C_OBSERVERS.index(kind) + self.salt) % 2 == 0

    def step_macro(self, form, hold=False):
        """the requests are held per env and redrawn for about a tenth of the envs per op (`hold`: for none); every fourth op gives a
        NaN to one env, every fifth -0.0 wherever a request is 0.0 -- in the record of the call, not in the held requests"""
        N, rng = self.N, self.rng
        n = self.n_macro
        self.n_macro += 1
        if not hold:
            new = rng.random(N) < 0.1
            new[rng.integers(N)] = True
            new[0] = False                  # (env 0 keeps its request, with the 0.0 in it, for the whole programme)
            self.req[new] = self.requests(int(new.sum()))
        m = self.req.copy()
        if not hold and n % 4 == 3:
            m[rng.integers(1, N), rng.integers(4)] = np.nan
        idle = rng.random(N) < 0.15
        idle[rng.integers(N)] = True
        if not hold and n % 5 == 2:
            m[m == 0.0] = np.float32(-0.0)
            idle[0] = False                 # (... and meets the -0.0 awake)
        if not idle.any():
            idle[rng.integers(1, N)] = True
        if idle.all():
            idle[0] = False
        op = dict(kind='step_macro', macro=m, idle=idle.astype(np.uint8), hold=bool(hold))
        op.update(self.render(form))
        return op

    def _zeros(self, flat, mask):
        """inside the mask: a row that is all zero, a row that is all -0.0, a -0.0 in a row that is not zero"""
        pick = self.rng.permutation(np.flatnonzero(mask))
        if len(pick) >= 2:
            flat[pick[0]] = 0.0
        if len(pick) >= 3:
            flat[pick[1]] = np.float32(-0.0)
        flat[pick[-1], self.rng.integers(flat.shape[1])] = np.float32(-0.0)
        return pick

    def new(self, kind, unmasked=False, inplace=False, keep=None):
        """a record of one of C_MUTATORS.  `keep`: an env that a masked clearing call or detach must leave alone"""
        N, nobj, rng = self.N, self.nobj, self.rng
        op = dict(kind=kind)
        if kind == 'set_joint_torques':     # about +-5 N m on the arm, +-0.2 on the fingers
            t = np.concatenate([rng.uniform(-5.0, 5.0, (N, 7)), rng.uniform(-0.2, 0.2, (N, 4))], axis=1).astype(np.float32)
            mask = self.mask()
            self._zeros(t, mask)
            op.update(torques=t, mask=mask, inplace=bool(inplace))
        elif kind == 'set_external_wrenches':      # robot bodies: a few N, a few tenths of N m; objects: up to about their weight
            w = np.empty((N, N_WRENCH_ROWS, 6), np.float32)
            w[:, :11, :3], w[:, :11, 3:] = rng.uniform(-3.0, 3.0, (N, 11, 3)), rng.uniform(-0.3, 0.3, (N, 11, 3))
            w[:, 11:, :3], w[:, 11:, 3:] = rng.uniform(-4.0, 4.0, (N, 3, 3)), rng.uniform(-0.02, 0.02, (N, 3, 3))
            mask = self.mask()
            pick = self._zeros(w.reshape(N, -1), mask)
            if len(pick) >= 5:              # the zero rule holds per target: robot rows all zero, object rows all zero
                w[pick[2], :11], w[pick[3], 11:] = 0.0, 0.0
            op.update(wrenches=w, mask=mask, inplace=bool(inplace))
        elif kind in ('clear_joint_torques', 'clear_external_wrenches', 'macro_invalidate', 'detach'):
            mask = None if unmasked else self.mask()
            if mask is not None and keep is not None:
                mask[keep] = 0
                if not mask.any():
                    mask[(keep + 1) % N] = 1
            op.update(mask=mask)
        elif kind == 'torques_from_dynamics':
            op.update(mask=self.mask(), compared=True, inverse=False)
        elif kind in ('attach', 'attach_capture'):
            pool = np.array(FINGER_LINKS + ARM_LINKS, np.int32)
            links = pool[rng.integers(len(pool), size=(N, nobj))].astype(np.int32)
            links[rng.random((N, nobj)) < 0.3] = -1            # some objects stay free inside an attached env
            links[rng.random(N) < 0.2] = -1                    # some envs have no attachment
            mask = self.mask()
            e = int(np.flatnonzero(mask)[0])                   # (whatever the draw: a masked env that carries something)
            links[e, 0] = pool[rng.integers(len(pool))]
            if nobj > 1:
                links[e, 1] = -1
            op.update(links=links, mask=mask)
            if kind == 'attach':
                rel = np.empty((N, nobj, 7), np.float32)
                rel[..., :3] = rng.uniform(-0.12, 0.12, (N, nobj, 3))
                rel[..., 3:] = rng.normal(size=(N, nobj, 4)) * rng.uniform(0.5, 2.0, (N, nobj, 1))      # (the library normalises)
                op.update(rel=rel)
        else:
            assert kind == 'detach_all', kind
        return op

    def dynamics(self):
        """posture_dynamics: the present state and K in {1, 3, 32} take turns, and so do velocities, accelerations and inverse=True"""
        N, rng = self.N, self.rng
        n = self.n_pd
        self.n_pd += 1
        op = dict(kind='posture_dynamics', compared=self.compared('posture_dynamics'))
        draw = lambda K, s: np.ascontiguousarray(rng.uniform(-s, s, (N, K, 11)).astype(np.float32))
        if n % 4 == 0:
            op.update(postures=None, velocities=None, accelerations=draw(1, 5.0) if n % 8 else None, inverse=True)
        else:
            K, turn = int(Q_KS[n % 4 - 1]), n % 3
            op.update(postures=self.postures(K), velocities=draw(K, 1.0) if turn != 1 else None, accelerations=draw(K, 5.0) if turn != 0 else None,
                      inverse=turn == 2)
        return op

    def sweep(self, kind):
        """carried_sweep / swept_clearance_refused: K cycles, segments a quarter of the way between two postures"""
        K = int(Q_KS[(self.n_sweep + self.salt) % 3])
        self.n_sweep += 1
        a, b = self.postures(K), self.postures(K)
        seg = np.ascontiguousarray(np.stack([a, a + np.float32(0.25) * (b - a)], axis=2))
        return dict(kind=kind, compared=self.compared(kind), segments=seg, safety=float(np.float32((0.0, 0.01, 0.04)[self.n_sweep % 3])))


def _command_program(seed, N, nobj, length):
    """a command programme (the comment at C_MIN_LENGTH): its own generator and rng stream.  The ORDER of its units is written out
    below, phase by phase, so that every condition of check_command_conditions holds by construction; the seed decides the order of
    the state mutators within a phase, the order of the independent groups, every mask, index and value."""
    if length < C_MIN_LENGTH:
        raise ValueError("a command programme needs at least %d ops" % C_MIN_LENGTH)
    rng = np.random.default_rng([int(seed), int(N), int(nobj), int(length), 2])
    salt = int(seed) % 7
    d = _CDraw(rng, N, nobj, salt=int(seed) % 4)
    sit = Situation(N)
    ops = []
    n = dict(form=int(rng.integers(3)), carry=salt, any=salt, on=salt, off=salt, slot=0)

    def emit(*more):
        for op in more:
            if op is not None:
                sit.apply(op)
                ops.append(op)

    def form():
        n['form'] += 1
        return n['form'] % 3

    def step(f):
        return d.step_macro(form()) if f == 'm' else d.step(f)

    def state(kind):
        if kind in ('write_joints', 'write_poses'):
            return dict(kind='write_state', parts=W_JOINT_POS if kind == 'write_joints' else W_OBJ_POSE, reset=False, fresh=False, rows=d.rows(), mask=d.mask())
        op = d.mutator(kind)
        if kind == 'load_snapshot':
            op['slot'] = n['slot']          # (a slot that has been saved)
        return op

    def order():
        """the eight state mutators in a seeded order, the device reset in front of the auto-reset (it finds young clocks)"""
        o = [STATE_MUTATORS[i] for i in rng.permutation(len(STATE_MUTATORS))]
        i, j = o.index('reset_dev'), o.index('episode_reset')
        if i > j:
            o[i], o[j] = o[j], o[i]
        return o

    def carry():
        n['carry'] += 1
        k = CARRY_QUERIES[n['carry'] % 4]
        return d.query(k, d.compared(k))

    def table(kind):
        return dict(kind=kind, compared=d.compared(kind))

    def obs(which):
        """the next observer of a rota: 'any' needs nothing, 'on' attachments on, 'off' attachments off"""
        n[which] += 1
        i = n[which]
        if which == 'on':
            assert sit.attached
            return (lambda: d.sweep('carried_sweep'), lambda: d.sweep('swept_clearance_refused'), carry, carry)[i % 4]()
        if which == 'off':
            assert not sit.attached
            return d.sweep('carried_sweep') if i % 2 else d.dynamics()
        return (d.dynamics, lambda: table('joint_torques'), lambda: table('external_wrenches'), lambda: table('attachments'))[i % 4]()

    def pair(op, f, behind=None):
        emit(op)
        emit(step(f))
        if behind:
            emit(obs(behind))

    def keep(nz):
        return int(np.flatnonzero(nz)[0]) if nz.any() else None

    def clear(kind, **kw):
        return d.new(kind, keep=keep(sit.t_nz if kind == 'clear_joint_torques' else sit.w_nz), **kw)

    # 1. plans: step_macro behind plan_macro, four times in a row with the same requests
    emit(d.mutator('plan_macro'), *[d.step_macro(form(), hold=True) for _ in range(4)])
    # 2. both tables and the attachments on; a snapshot and two checkpoints (restore takes the one before last) while they are set
    pair(d.new('set_joint_torques'), 0, 'any')
    pair(d.new('set_external_wrenches'), 1, 'any')
    pair(d.new('attach'), 2, 'on')
    sv = d.mutator('save_snapshot')
    n['slot'] = sv['slot']
    pair(sv, form(), 'any')
    pair(dict(kind='checkpoint'), form(), 'on')
    pair(dict(kind='checkpoint'), form())
    emit(*[d.step(form()) for _ in range(length - C_MIN_LENGTH)])
    # 3. everything on: a new mutator, step_macro, a state mutator, a step -- the state mutator with both tables non-zero, with
    #    attachments on and directly behind a step_macro with plans in flight; the new mutator directly behind a step
    news = ['set_joint_torques', 'set_external_wrenches', 'clear_joint_torques', 'clear_external_wrenches', 'torques_from_dynamics', 'attach',
            'attach_capture', 'macro_invalidate']
    news = news[salt % 8:] + news[:salt % 8]
    for new, s in zip(news, order()):
        emit(clear(new) if new.startswith('clear') else d.new(new), carry() if new == 'attach_capture' else None)
        emit(step('m'), state(s), step(form()))
    # 4. step_macro directly behind each state mutator
    for i, s in enumerate(order()):
        pair(state(s), 'm', ('on', 'any')[i % 2] if i % 4 != 3 else None)
    # 5a. attach_capture directly behind five state mutators, a carry query directly behind every attach_capture
    for i, s in enumerate(CAPTURE_BEHIND):
        emit(state(s), d.new('attach_capture'), carry(), step(i % 3))
    # 5b. a carry query directly behind the same five
    for i, s in enumerate(CAPTURE_BEHIND):
        emit(state(s), carry(), step(form()), obs('on') if i % 2 else None)
    # 5c. independent groups in a seeded order; every group leaves both tables and the attachments on
    def g_dynamics():
        emit(state('fork_dev'), d.new('torques_from_dynamics'), step(0))
        pair(d.new('torques_from_dynamics'), 1, 'any')
        pair(d.new('torques_from_dynamics'), 2)

    def g_tables():
        pair(d.new('set_joint_torques', inplace=True), 1, 'any')
        pair(d.new('set_joint_torques'), 2)
        pair(d.new('set_external_wrenches', inplace=True), 0, 'on')
        pair(d.new('set_external_wrenches'), 2)

    def g_clear():
        pair(clear('clear_joint_torques'), 0, 'any')
        pair(clear('clear_external_wrenches'), 0)
        pair(clear('clear_joint_torques'), 1, 'on')
        pair(clear('clear_external_wrenches'), 1)

    def g_macro():
        pair(d.mutator('plan_macro'), 'm')       # (the mixed use: an env whose record equals its request keeps plan_macro's plan)
        emit(d.filler('step_plan', form()), d.step_macro(form(), hold=True))
        pair(d.new('macro_invalidate'), 0)
        pair(d.new('macro_invalidate', unmasked=True), 1, 'any')
        pair(d.new('macro_invalidate'), 2)

    def g_detach():
        for f in (0, 1, 2, 'm'):
            pair(d.new('detach', keep=keep(sit.att)), f, 'on' if f in (0, 2) else None)
        for k, f in enumerate((0, 1, 'm')):
            pair(d.new('detach_all'), f, 'off' if f != 'm' else None)
            if k < 2:
                pair(d.new('attach'), f, 'on')
        # the two float64 anchors: a given attach of every env, then the state a record defines
        emit(anchor_attach(N, nobj, 0), dict(d.mutator('set_state'), anchor=True), step(form()))
        emit(anchor_attach(N, nobj, 1), dict(kind='write_state', parts=15, reset=False, fresh=True, rows=d.rows(), mask=None, anchor=True), step(form()))

    groups = [g_dynamics, g_tables, g_clear, g_macro, g_detach]
    for i in rng.permutation(len(groups)):
        groups[i]()
    # 6. the feature-off road: the three unmasked clearing calls, then every state mutator once more
    pair(d.new('clear_joint_torques', unmasked=True), 2)
    pair(d.new('clear_external_wrenches', unmasked=True), 2)
    pair(d.new('detach_all'), 2, 'off')
    assert sit.all_off()
    for i, s in enumerate(order()):
        pair(state(s), form(), ('off', 'any')[i % 2] if i % 4 != 3 else None)
    assert len(ops) == length, (len(ops), length)
    return ops


def is_anchor(op):
    """behind this op the state of every env is compose_state(op['rows']), known on the CPU"""
    return op['kind'] == 'set_state' or (op['kind'] == 'write_state' and op['parts'] == 15 and op['fresh'] and op['mask'] is None)


def check_query_conditions(ops, length, nobj):
    """what a query programme drawn for a handle with `nobj` objects holds, asserted"""
    assert len(ops) == length >= Q_MIN_LENGTH
    kinds = [o['kind'] for o in ops]
    muts = set(MUTATORS) | set(Q_MUTATORS)
    assert set(kinds) <= set(STEP_KINDS) | muts | set(Q_OBSERVERS)
    for m in Q_MUTATORS:
        forms = [b['render'] for a, b in zip(ops, ops[1:]) if a['kind'] == m and b['kind'] == 'step']
        assert set(forms) == set(RENDER_FORMS) and len(forms) >= 3, (m, forms)
    around = [(p, o, n) for p, o, n in zip(ops, ops[1:], ops[2:]) if o['kind'] in Q_OBSERVERS]
    step_mut = {o['kind'] for p, o, n in around if p['kind'] in STEP_KINDS and n['kind'] in muts}
    assert step_mut == set(Q_OBSERVERS), set(Q_OBSERVERS) - step_mut
    for k in Q_OBSERVERS:
        front = [p['kind'] for p, o, n in around if o['kind'] == k and p['kind'] in muts and n['kind'] in STEP_KINDS]
        assert front and set(front) != {'write_state'}, (k, front)
        assert {o['compared'] for o in ops if o['kind'] == k} == {False, True}, k
    read = [(a, b['kind']) for a, b in zip(ops, ops[1:]) if b['kind'] in STATE_READERS]
    for m in READ_BEHIND:
        assert any(a['kind'] == m for a, _ in read), m
    assert any(a['kind'] == 'write_state' and a['parts'] & W_OBJ_POSE and not is_anchor(a) for a, _ in read)
    assert any(a['kind'] == 'write_state' and a['parts'] & W_JOINT_POS and not is_anchor(a) for a, _ in read)
    assert any(a['kind'] == 'set_distance_pairs' and b in PAIR_READERS for a, b in read)
    assert any(a['kind'] == 'set_kinematic_points' and b == 'posture_ik_present' for a, b in read)
    # the draws
    K = {o[key].shape[1] for o in ops for key in ('postures', 'segments', 'goals') if o['kind'] in Q_OBSERVERS and key in o}
    assert K == set(Q_KS), K
    tables = [o for o in ops if o['kind'] == 'set_distance_pairs']
    assert {o['cls'] for o in tables} == set(Q_PAIR_CLASSES)
    assert any(o['max_distance'] is None for o in tables) and any(o['max_distance'] is not None for o in tables)
    assert all(o['max_distance'] is None or 0.05 <= o['max_distance'] <= 0.25 for o in tables)
    for o in tables:
        want = {'one': 1, 'full': 96}.get(o['cls'])
        assert (o['pairs'] == 'collision') == (o['cls'] == 'collision') and (o['cls'] != 'default' or o['pairs'] == default_pairs(nobj))
        assert want is None or len(o['pairs']) == want
        if o['pairs'] != 'collision':
            assert all(a != b and {a, b} <= set(ROBOT_SHAPES + STATIC_SHAPES + OBJECT_SHAPES[:nobj]) for a, b in o['pairs'])
    points = [o for o in ops if o['kind'] == 'set_kinematic_points']
    assert all(1 <= len(o['links']) <= 8 and o['local'].shape == (len(o['links']), 3) and (np.abs(o['local']) >= 0.01).all() for o in points)
    assert any(set(o['links'].tolist()) & set(FINGER_LINKS) for o in points) and any(set(o['links'].tolist()) & set(ARM_LINKS) for o in points)
    assert any(o['links'][-1] in FINGER_LINKS for o in points) and any(o['links'][-1] in ARM_LINKS for o in points)
    rays = [o for o in ops if o['kind'] == 'set_rays']
    assert {len(o['links']) for o in rays} == set(Q_RAY_COUNTS)
    assert any((o['links'] < 0).any() and (o['links'] >= 0).any() for o in rays)
    for key, kind in (('safety', 'swept_clearance'), ('margin', 'signed_distance_gradient'), ('position_only', 'posture_ik'), ('clamp', 'posture_ik')):
        assert len({o[key] for o in ops if o['kind'] in (kind, kind + '_present')}) >= 2, key
    # what a unit needs, and the anchors: the state a record defines, with the default table in force
    for i, k in enumerate(kinds):
        assert k != 'restore' or 'checkpoint' in kinds[:i]
        assert k != 'episode_reset' or 'reset_dev' in kinds[:i]
        assert k != 'load_snapshot' or any(o['kind'] == 'save_snapshot' and o['slot'] == ops[i]['slot'] for o in ops[:i])
    table, n_anchor = ('default', None), set()
    for o in ops:
        if o['kind'] == 'set_distance_pairs':
            table = (o['cls'], o['max_distance'])
        if is_anchor(o):
            assert table == ('default', None), table
            n_anchor.add(o['kind'])
        for key in ('mask', 'flags'):
            if o.get(key) is not None:
                assert np.asarray(o[key]).any(), (o['kind'], key)
    assert n_anchor == {'set_state', 'write_state'}
    return dict(count={m: kinds.count(m) for m in muts | set(Q_OBSERVERS)})


def check_command_conditions(ops, length, N, nobj):
    """what a command programme drawn for a handle of N envs and `nobj` objects holds, asserted from the records alone.  A `step`
    below is a step or a step_macro unless a render form is asked for; `directly` means the neighbouring record.  One exception is
    forced by the conditions themselves: a carry query stands directly behind EVERY attach_capture, so the step that follows an
    attach_capture follows it behind that one read-only record."""
    assert len(ops) == length >= C_MIN_LENGTH
    kinds = [o['kind'] for o in ops]
    muts = set(MUTATORS) | set(C_MUTATORS)
    assert set(kinds) <= set(C_STEP_KINDS) | muts | set(C_OBSERVERS), set(kinds) - set(C_STEP_KINDS) - muts - set(C_OBSERVERS)
    sit = Situation(N)
    before, after = [], []                  # the situation in front of and behind every record
    snap = lambda: dict(tables=sit.tables(), carrying=sit.carrying(), attached=sit.attached, in_flight=sit.in_flight(), off=sit.all_off(),
                        t_on=sit.t_on, w_on=sit.w_on)
    for o in ops:
        before.append(snap())
        sit.apply(o)
        after.append(snap())
    nxt = lambda i: ops[i + 1] if i + 1 < len(ops) else dict(kind=None)
    is_carry = lambda i: kinds[i] in CARRY_QUERIES and before[i]['attached']
    # every new mutator: directly followed by a step of each render form, and by a step_macro
    for m in C_MUTATORS:
        forms, macro = set(), False
        for i, k in enumerate(kinds):
            if k != m:
                continue
            j = i + 2 if m == 'attach_capture' and i + 1 < len(ops) and is_carry(i + 1) else i + 1
            if j < len(ops) and kinds[j] == 'step':
                forms.add(ops[j]['render'])
            macro = macro or (j < len(ops) and kinds[j] == 'step_macro')
        assert forms == set(RENDER_FORMS) and macro, (m, forms, macro)
    for k in ('clear_joint_torques', 'clear_external_wrenches', 'macro_invalidate'):
        assert {o['mask'] is None for o in ops if o['kind'] == k} == {False, True}, k
    # the state mutators, each time directly followed by a step: with both tables non-zero, with attachments on, directly behind a
    # step_macro with plans in flight, and once more with every feature off behind the unmasked clearing calls
    seen = {s: set() for s in STATE_MUTATORS}
    for i, o in enumerate(ops):
        s = state_kind(o)
        if s is None or nxt(i)['kind'] not in ('step', 'step_macro'):
            continue
        b = before[i]
        seen[s] |= {name for name, ok in (('tables', b['tables']), ('carrying', b['carrying']), ('off', b['off'] and nxt(i)['kind'] == 'step'),
                                          ('in_flight', i > 0 and kinds[i - 1] == 'step_macro' and b['in_flight']),
                                          ('macro_behind', nxt(i)['kind'] == 'step_macro')) if ok}
    for s, got in seen.items():
        assert got == {'tables', 'carrying', 'in_flight', 'off', 'macro_behind'}, (s, got)
    assert all(any(k == c for k in kinds[:max(i for i, a in enumerate(after) if a['off'])]) for c in ('clear_joint_torques', 'clear_external_wrenches', 'detach_all'))
    # a carry query and an attach_capture directly behind five state mutators and a step; a carry query behind every attach_capture
    behind = {'carry': set(), 'attach_capture': set()}
    for i in range(1, len(ops)):
        what = 'carry' if is_carry(i) else kinds[i] if kinds[i] == 'attach_capture' else None
        if what:
            behind[what].add('step' if kinds[i - 1] in C_STEP_KINDS else state_kind(ops[i - 1]))
        if kinds[i - 1] == 'attach_capture':
            assert is_carry(i), i
    for what, got in behind.items():
        assert got >= set(CAPTURE_BEHIND) | {'step'}, (what, got)
    assert {kinds[i] for i in range(len(ops)) if is_carry(i)} == set(CARRY_QUERIES)
    # carried_sweep with attachments on and off; swept_clearance refuses only while they are on; every observer compared and silent
    assert {before[i]['attached'] for i, k in enumerate(kinds) if k == 'carried_sweep'} == {False, True}
    assert all(before[i]['attached'] for i, k in enumerate(kinds) if k == 'swept_clearance_refused') and 'swept_clearance' not in kinds
    for k in C_OBSERVERS:
        assert {o['compared'] for o in ops if o['kind'] == k} == {False, True}, k
    pd = [o for o in ops if o['kind'] == 'posture_dynamics']
    assert {None if o['postures'] is None else o['postures'].shape[1] for o in pd} == {None} | set(Q_KS)
    assert any(o['velocities'] is not None for o in pd) and any(o['accelerations'] is not None for o in pd) and {o['inverse'] for o in pd} == {False, True}
    assert all(o['velocities'] is None for o in pd if o['postures'] is None)
    # torques_from_dynamics directly behind a step and directly behind a fork_dev
    tfd = {kinds[i - 1] for i, k in enumerate(kinds) if k == 'torques_from_dynamics'}
    assert 'fork_dev' in tfd and tfd & set(C_STEP_KINDS), tfd
    # step_macro: behind plan_macro, behind macro_invalidate, directly behind each state mutator (above), three times in a row unchanged
    sm = [i for i, k in enumerate(kinds) if k == 'step_macro']
    assert any(kinds[i - 1] == 'plan_macro' for i in sm if i) and any(kinds[i - 1] == 'plan_macro' and before[i - 1]['in_flight'] for i in sm if i)
    assert any(kinds[i - 1] == 'macro_invalidate' for i in sm if i) and any(kinds[i - 1] == 'step_plan' for i in sm if i)
    same = lambda a, b: np.array_equal(a['macro'].view(np.uint32), b['macro'].view(np.uint32))
    assert any(kinds[i + 1] == kinds[i + 2] == 'step_macro' and same(ops[i], ops[i + 1]) and same(ops[i], ops[i + 2]) for i in sm if i + 2 < len(ops))
    assert any(np.isnan(ops[i]['macro']).any() for i in sm) and {ops[i]['render'] for i in sm} == set(RENDER_FORMS)
    # ... a -0.0 where the record has 0.0 in an env that is not idle, and it does not re-plan
    model, negzero = MacroModel(N), 0
    for o in ops:
        if o['kind'] == 'step_macro':
            hit = (np.signbit(o['macro']) & (o['macro'] == 0) & (model.record == 0) & ~np.signbit(model.record)).any(axis=1) & (o['idle'] == 0)
        model.apply(o)
        if o['kind'] == 'step_macro':
            negzero += int((hit & (model.replanned == 0)).sum())
    assert negzero > 0
    # snapshots and checkpoints while tables, attachments and records are set; loads and restores after those have changed
    changed = lambda i, j: any(k in C_MUTATORS or k == 'step_macro' for k in kinds[i + 1:j])
    for save, load in (('save_snapshot', 'load_snapshot'), ('checkpoint', 'restore')):
        at = [i for i, k in enumerate(kinds) if k == save]
        assert at and all(before[i]['tables'] and before[i]['carrying'] and before[i]['in_flight'] for i in at), save
        for j, k in enumerate(kinds):
            if k == load:
                prev = [i for i in at if i < j and (save == 'checkpoint' or ops[i]['slot'] == ops[j]['slot'])]
                assert prev and changed(prev[-1], j), (load, j)
    assert kinds.count('checkpoint') >= 2 and min(i for i, k in enumerate(kinds) if k == 'restore') > sorted(i for i, k in enumerate(kinds) if k == 'checkpoint')[1]
    for i, k in enumerate(kinds):
        assert k != 'episode_reset' or 'reset_dev' in kinds[:i]
    # the draws: masks are never all-clear; zero and -0.0 rows inside the mask; wrench rows for objects a smaller handle lacks; the
    # in-place write once per table, with the feature on; links on finger and arm links, free objects, envs without attachment
    for o in ops:
        for key in ('mask', 'flags', 'idle'):
            if o.get(key) is not None:
                assert np.asarray(o[key]).any(), (o['kind'], key)
    for kind, key, on in (('set_joint_torques', 'torques', 't_on'), ('set_external_wrenches', 'wrenches', 'w_on')):
        recs = [(i, o) for i, o in enumerate(ops) if o['kind'] == kind]
        assert sum(o['inplace'] for _, o in recs) == 1 and all(before[i][on] for i, o in recs if o['inplace'])
        rows = [o[key][o['mask'] != 0].reshape(int((o['mask'] != 0).sum()), -1) for _, o in recs]
        assert any((r == 0).all(axis=1).any() for r in rows) and any(np.signbit(r).any() for r in rows) and all(np.isfinite(r).all() for r in rows)
        top = max(float(np.abs(o[key]).max()) for _, o in recs)
        assert top <= 5.0, (kind, top)
    assert all(o['wrenches'].shape == (N, N_WRENCH_ROWS, 6) and o['wrenches'][:, 11 + nobj:].any() == (nobj < 3) for o in ops if o['kind'] == 'set_external_wrenches')
    att = [o for o in ops if o['kind'] in ('attach', 'attach_capture')]
    pool = set(FINGER_LINKS + ARM_LINKS)
    assert all(o['links'].shape == (N, nobj) and set(o['links'][o['links'] >= 0].tolist()) <= pool for o in att)
    used = set().union(*[set(o['links'][o['links'] >= 0].tolist()) for o in att])
    assert used & set(FINGER_LINKS) and used & set(ARM_LINKS)
    assert any((o['links'] < 0).all(axis=1).any() for o in att) and (nobj == 1 or any(((o['links'] < 0).any(axis=1) & (o['links'] >= 0).any(axis=1)).any() for o in att))
    assert all(('rel' in o) == (o['kind'] == 'attach') for o in att)
    # the anchors: a set_state and a full write_state, each directly behind its attach of every env
    anchors = [i for i, o in enumerate(ops) if is_command_anchor(o)]
    assert {kinds[i] for i in anchors} == {'set_state', 'write_state'} and len(anchors) == 2
    assert all(ops[i - 1].get('anchor') and kinds[i - 1] == 'attach' and ops[i - 1]['mask'] is None for i in anchors)
    return dict(count={k: kinds.count(k) for k in sorted(set(kinds))})


def program(seed, N, nobj, length, queries=False, commands=False):
    """list of `length` op records (dicts with a 'kind'); the same arguments give the same programme"""
    assert not (queries and commands)
    if queries:
        return _query_program(seed, N, nobj, length)
    if commands:
        return _command_program(seed, N, nobj, length)
    if length < MIN_LENGTH:
        raise ValueError("a programme needs at least %d ops" % MIN_LENGTH)
    rng = np.random.default_rng([int(seed), int(N), int(nobj), int(length)])
    units = _ordered(_units(rng), rng)
    spare = length - sum(2 + (u[1] is not None) + (u[3] is not None) + 2 * u[4] for u in units)
    assert spare >= 3, (length, spare)
    bare = [i for i, u in enumerate(units) if u[3] is None and i + 1 < len(units)] or [0]
    fill = {}
    kinds = ['step_refused', 'render', 'step_plan', 'step']
    first_plan = min(i for i, u in enumerate(units) if u[0] == 'plan_macro')
    planned = [i for i in bare if i >= first_plan] or [first_plan]           # (a step_plan needs a plan)
    for k in range(spare):
        what = kinds[k % 3] if k < 6 else kinds[k % 4]
        where = planned if what == 'step_plan' else bare
        fill.setdefault(where[int(rng.integers(len(where)))], []).append(what)
    draw = _Draw(rng, N, nobj, salt=int(seed) % 4)
    ops = []
    for i, (mut, before, form, behind, launch) in enumerate(units):
        op = draw.mutator(mut)
        if launch:                          # the object of this set_object_home leaves the bounds one step before the call
            env = int(rng.integers(N)) if op['env'] is None else op['env']
            ops += [draw.launch(env, op['obj']), draw.step(0)]
        ops.append(op)
        if before is not None:
            ops.append(draw.observer(before))
        ops.append(draw.step(form))
        for what in fill.get(i, ()):
            ops.append(draw.filler(what, int(rng.integers(3))))
        if behind is not None:
            ops.append(draw.observer(behind))
    assert len(ops) == length
    return ops


def is_step(op):
    return op['kind'] in C_STEP_KINDS


def render_form(op):
    return None if op['kind'] == 'render' else op.get('render')


def check_conditions(ops, length):
    """what every programme holds, asserted"""
    assert len(ops) == length >= MIN_LENGTH
    kinds = [o['kind'] for o in ops]
    assert set(kinds) <= set(STEP_KINDS) | set(MUTATORS) | set(OBSERVERS)
    count = {m: kinds.count(m) for m in MUTATORS}
    followed = {m: set() for m in MUTATORS}
    for a, b in zip(ops, ops[1:]):
        if a['kind'] in MUTATORS and b['kind'] == 'step':
            followed[a['kind']].add(b['render'])
    step_mut = {k for p, k, n in zip(kinds, kinds[1:], kinds[2:]) if k in OBSERVERS and p in STEP_KINDS and n in MUTATORS}
    mut_step = {k for p, k, n in zip(kinds, kinds[1:], kinds[2:]) if k in OBSERVERS and p in MUTATORS and n in STEP_KINDS}
    assert min(count.values()) >= 3, count
    assert all(f == set(RENDER_FORMS) for f in followed.values()), followed
    assert mut_step == set(OBSERVERS), set(OBSERVERS) - mut_step
    assert step_mut == set(OBSERVERS), set(OBSERVERS) - step_mut
    writes = [o for o in ops if o['kind'] == 'write_state']
    assert {o['parts'] for o in writes} == set(range(16))
    assert {(o['reset'], o['fresh']) for o in writes} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(o['parts'] == 0 and o['reset'] and not o['fresh'] for o in writes) or any(o['parts'] == 0 and o['fresh'] for o in writes)
    assert any(o['parts'] == 4 and not o['reset'] and not o['fresh'] for o in writes)            # == rr_set_object_poses
    assert any(o['parts'] == 4 and o['reset'] and not o['fresh'] for o in writes)                # == the auto-reset's pair
    assert any(o['parts'] == 15 and o['fresh'] and not o['reset'] and o['mask'] is None for o in writes)      # == rr_set_state
    # a set_object_home whose object a write has thrown out of bounds one step before
    assert any(a['kind'] == 'write_state' and a['parts'] == 12 and b['kind'] == 'step' and c['kind'] == 'set_object_home' and d['kind'] == 'step'
               and a['mask'].sum() == 1 and c['env'] in (None, int(np.flatnonzero(a['mask'])[0])) for a, b, c, d in zip(ops, ops[1:], ops[2:], ops[3:]))
    for k in ('restore', 'load_snapshot'):
        at = max(i for i, x in enumerate(kinds) if x == k)
        assert any(x.startswith('fork') for x in kinds[:at]) and 'reset_dev' in kinds[:at], k
    n_ckpt = 1                                                          # (the set-up's)
    for k in kinds:
        n_ckpt += k == 'checkpoint'
        assert k != 'restore' or n_ckpt >= 2
    planned = False
    for o in ops:
        planned = planned or o['kind'] == 'plan_macro'
        assert o['kind'] != 'step_plan' or planned
        for key in ('mask', 'flags', 'idle', 'refused'):
            if o.get(key) is not None:
                assert np.asarray(o[key]).any(), (o['kind'], key)
    for what in ('step_refused', 'render', 'step_plan'):
        assert kinds.count(what) >= 2, what
    assert {o['device'] for o in ops if o['kind'] == 'step'} == {False, True}
    return dict(count=count)


# ------------------------------------------------------------------------------------------------------------------ execution
def compose_state(rows, nobj):
    """float32 [N, 61] of a recipe of _Draw.rows (the columns of objects the handle does not have stay zero)"""
    N = len(rows['q'])
    s = np.zeros((N, 61), np.float32)
    s[:, :11], s[:, 11:22] = rows['q'], rows['qd']
    for o in range(nobj):
        s[:, 22 + 13 * o:25 + 13 * o] = BASE[o] + rows['off'][:, o]
        s[:, 25 + 13 * o:29 + 13 * o] = rows['quat'][:, o]
        s[:, 29 + 13 * o:35 + 13 * o] = rows['twist'][:, o]
    return s


def part_columns(parts, nobj):
    cols = (list(range(0, 11)) if parts & W_JOINT_POS else []) + (list(range(11, 22)) if parts & W_JOINT_VEL else [])
    for o in range(nobj):
        cols += list(range(22 + 13 * o, 29 + 13 * o)) if parts & W_OBJ_POSE else []
        cols += list(range(29 + 13 * o, 35 + 13 * o)) if parts & W_OBJ_VEL else []
    return np.array(cols)


def goal_table(nobj, W, H, seed=5):
    """(start_poses, final_pos, flags, rgb) of N_GOALS goals around BASE: every mix of scored / start-pose bits, NaN where a bit is
    clear (the table of tests/test_gpu_episode.py, for any number of objects)"""
    rng = np.random.default_rng(seed)
    flags = np.array([[3, 3, 3], [0, 1, 2], [1, 1, 1], [3, 2, 2], [1, 0, 3]], np.uint8)[:, :nobj].copy()
    flags[1, 0] = 3 if nobj == 1 else flags[1, 0]
    start = np.zeros((N_GOALS, nobj, 7), np.float32)
    start[..., :3] = BASE[:nobj] + rng.uniform([-0.04, -0.04, 0.02], [0.04, 0.04, 0.05], (N_GOALS, nobj, 3))
    start[..., 6] = 1.0
    final = (BASE[:nobj] + rng.uniform(-0.08, 0.08, (N_GOALS, nobj, 3)) * [1, 1, 0]).astype(np.float32)
    start[(flags & 2) == 0] = np.nan
    final[(flags & 1) == 0] = np.nan
    return start, final, flags, rng.integers(1, 256, size=(N_GOALS, H, W, 3), dtype=np.uint8)


def torch_device(a):
    """a numpy array -> CUDA torch tensor, complete before the library's stream can read it"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def torch_copy_in_place(env, name, table, mask):
    """the rows of `table` (a CUDA tensor) whose mask byte is set (None: all) into the handle's zero-copy view `name`, in the
    library's stream order: behind everything the library has enqueued, complete before its next call"""
    import torch
    env.sync()
    view = torch.from_dlpack(getattr(env, name))
    if mask is None:
        view.copy_(table)
    else:
        on = mask != 0
        view[on] = table[on]
    torch.cuda.synchronize()


class Session:
    """One handle that executes op records along a road.  `to_device` turns a numpy array into device memory (a CUDA torch tensor;
    the recording fake of the CPU test passes its own marker).  Device arguments are kept alive until `release()`: the library
    reads them in place on its stream."""

    def __init__(self, env, road, to_device=torch_device):
        assert road in ('device', 'host', 'written')
        self.env, self.road, self.dev = env, road, to_device
        self.N, self.nobj = env.N, env.n_objects
        self.keep, self.ckpts = [], []
        self.sel = 7
        self.refused = 0
        self.episode = np.zeros(self.N, np.int32)        # the host route's count of auto-resets per env
        self.final_obs = np.zeros((self.N, 13 + 7 * self.nobj + 1), np.float32)
        # the query tables in force, as the Session has set them (a fresh handle: the gripper base at its origin, no pairs, no rays)
        self.points = (np.array([8], np.int32), np.zeros((1, 3), np.float32))
        self.max_distance, self.n_rays = None, 0
        self.last = {}                      # result buffers (FAMILY) -> the query record whose call wrote them last
        # the command programmes: whether the attachments are on, the macro model (record, position, replanned) with the envs that
        # the last op re-planned, the arrays of the compared table read-backs, the refusals met; `copy_in_place` writes rows through
        # a zero-copy view, `strict`: the handle is a real one (a fake refuses nothing and has no buffers)
        self.attached, self.macro, self.macro_now = False, MacroModel(self.N), np.zeros(self.N, np.uint8)
        self.read, self.refusals, self.commands = {}, 0, False      # (`commands`: a comparison looks at the tables and the macro buffers too)
        self.copy_in_place, self.strict = torch_copy_in_place, to_device is torch_device

    def setup(self):
        """what both handles get behind the warm-up: the ray table, snapshot slots, goals, the episode rule, a first checkpoint"""
        from real_robots_amd import _native as nat
        env = self.env
        seg = np.zeros((N_WORLD_RAYS + N_LINK_RAYS, 6), np.float32)
        seg[:N_WORLD_RAYS] = [[BASE[o % 3][0], BASE[o % 3][1], 1.0, BASE[o % 3][0], BASE[o % 3][1], 0.2] for o in range(N_WORLD_RAYS)]
        seg[N_WORLD_RAYS:, 5] = 0.4
        env.set_rays([-1] * N_WORLD_RAYS + [nat.EE_LINK] * N_LINK_RAYS, seg)
        self.n_rays = N_WORLD_RAYS + N_LINK_RAYS
        env.snapshot_slots(N_SLOTS)
        self.goals = goal_table(self.nobj, env.W, env.H)
        env.set_goals(*self.goals)
        self.goal_index = (np.arange(self.N) % (N_GOALS + 1) - 1).astype(np.int32)
        env.set_env_goals(self.goal_index)
        env.set_episode(HORIZON, GOAL_STRIDE)
        self.ckpts.append(env.checkpoint())
        env.set_distance_pairs(default_pairs(self.nobj))   # (a setting of the handle: resets, forks and restore keep it)

    def release(self):
        self.keep.clear()

    def _on_device(self, op):
        return self.road == 'device' or (self.road == 'written' and op.get('device', False))

    def _d(self, a):
        t = self.dev(a)
        self.keep.append(t)
        return t

    def _ptr(self, t):
        return int(t.data_ptr())

    def apply(self, op):
        self.macro_now = np.zeros(self.N, np.uint8)      # (the envs that THIS op re-plans: a step_macro sets them)
        getattr(self, '_' + op['kind'])(op)

    # ---- steps
    def _render_arg(self, op):
        return op['flags'] if op['render'] == 2 else bool(op['render'])

    def _step(self, op):
        if self._on_device(op):
            self.env.step(render=self._render_arg(op), device_ptr=self._ptr(self._d(op['cmd'])))
        else:
            self.env.step(op['cmd'], render=self._render_arg(op))

    def _step_refused(self, op):
        """the Python layer refuses a non-finite host command before the library sees it (robot.py:189): the host road hands it to
        rr_step itself, which stages it like any other and leaves the refusal to the solve kernel, as with a device command"""
        if self._on_device(op):
            return self._step(op)
        from real_robots_amd import _native as nat
        flags = np.ascontiguousarray(op['flags'], dtype=np.uint8) if op['render'] == 2 else None
        cmd = np.ascontiguousarray(op['cmd'], dtype=np.float32)
        nat.check(self.env.L.rr_step(self.env.h, cmd.ctypes.data, 0, int(op['render']), flags.ctypes.data if flags is not None else None))

    def _step_plan(self, op):
        self.macro.apply(op)
        self.env.step_plan(self._render_arg(op), idle=op['idle'])

    def _render(self, op):
        self.env.render()

    # ---- mutators
    def _reset_host(self, op):
        self.env.reset(self._d(op['mask']) if self._on_device(op) else op['mask'])

    _reset_dev = _reset_host

    def _set_state(self, op):
        s = compose_state(op['rows'], self.nobj)
        if self.road == 'device' and self.nobj == 3:     # (bitwise rr_set_state on a handle with three objects only)
            self.env.write_state(self._d(s), None, joint_pos=True, joint_vel=True, obj_pose=True, obj_vel=True, fresh=True)
        else:
            self.env.state = s

    def _write_state(self, op):
        env, nobj, parts = self.env, self.nobj, op['parts']
        full = compose_state(op['rows'], nobj)
        on = np.ones(self.N, bool) if op['mask'] is None else op['mask'] != 0
        cols = part_columns(parts, nobj)
        T = None                                         # (no column group: no tensor)
        if parts:
            T = np.full((self.N, 61), np.nan, np.float32)    # NaN in everything the call must not read
            T[np.ix_(on, cols)] = full[np.ix_(on, cols)]
        kw = dict(joint_pos=bool(parts & 1), joint_vel=bool(parts & 2), obj_pose=bool(parts & 4), obj_vel=bool(parts & 8),
                  reset=op['reset'], fresh=op['fresh'])
        if self.road != 'host':
            env.write_state(None if T is None else self._d(T), None if op['mask'] is None else self._d(op['mask']), **kw)
            return
        if parts == 0 and not op['fresh']:                 # parts == RR_W_RESET == rr_reset
            env.reset(op['mask'])
            return
        poses = np.stack([full[:, 22 + 13 * o:29 + 13 * o] for o in range(nobj)], axis=1)
        if parts == W_OBJ_POSE and not op['fresh']:      # RR_W_OBJ_POSE == rr_set_object_poses; with RR_W_RESET: rr_reset first
            if op['reset']:
                env.reset(op['mask'])
            env.set_object_poses(poses, op['mask'])
        elif parts == 15 and op['fresh'] and not op['reset'] and op['mask'] is None and nobj == 3:
            env.state = full                             # 15 | RR_W_FRESH with a NULL mask == rr_set_state
        else:
            env.write_state(T, op['mask'], **kw)

    def _pose7(self, op):
        return np.concatenate([BASE[op['obj']] + op['off'], op['quat']]).astype(np.float32)

    def _set_object_pose(self, op):
        self.env.set_object_pose(op['env'], op['obj'], self._pose7(op))

    def _set_object_poses(self, op):
        full = compose_state(op['rows'], self.nobj)
        self.env.set_object_poses(np.stack([full[:, 22 + 13 * o:29 + 13 * o] for o in range(self.nobj)], axis=1), op['mask'])

    def _set_object_home(self, op):
        self.env.set_object_home(op['env'], op['obj'], self._pose7(op))

    def _set_object_dynamics(self, op):
        self.env.set_object_dynamics(mass=op['mass'], friction=op['friction'], env_mask=op['mask'])

    def _set_env_actuators(self, op):
        self.env.set_env_actuators(kp=op['kp'], max_force=op['max_force'], damping=op['damping'], env_mask=op['mask'])

    def _index(self, op):
        if op['index'] is None:
            return None
        return self._d(op['index']) if self._on_device(op) else op['index']

    def _fork_host(self, op):
        self.env.fork(self._index(op))

    _fork_dev = _fork_host

    def _save_snapshot(self, op):
        self.env.save_snapshot(op['slot'], self._index(op))

    def _load_snapshot(self, op):
        self.env.load_snapshot(op['slot'], self._index(op))

    def _checkpoint(self, op):
        self.ckpts.append(self.env.checkpoint())

    def _restore(self, op):
        self.env.restore(self.ckpts[-2])                 # the checkpoint before last

    def _plan_macro(self, op):
        self.macro.apply(op)
        self.env.plan_macro(op['macro'], op['mask'])

    def _set_env_goals(self, op):
        self.env.set_env_goals(op['index'], op['mask'])
        self.goal_index = np.where(op['mask'] != 0, op['index'], self.goal_index).astype(np.int32)

    def _episode_reset(self, op):
        """The device road: one launch.  The host road is the one of tests/test_gpu_episode.py (test_auto_reset_equals_the_host_route_
        bit_for_bit): the update without reset, then rr_reset + rr_set_object_poses of the done envs into the next goal's start poses
        and rr_set_env_goals for the new index and the re-based score.  The episode counter and the final observation have no host
        call: the Session keeps what they must be (`episode`, `final_obs`)."""
        from real_robots_amd import _native as nat
        env = self.env
        if self.road != 'host':
            env.episode_update(True)
            return
        env.episode_update(False)
        done = env.episode_buffer('done', host=True) != 0
        if not done.any():
            return
        score = env.episode_buffer('score', host=True)
        obs = np.concatenate([env.host(nat.F_JOINTS), env.host(nat.F_TOUCH), env.host(nat.F_OBJ_POSE).reshape(self.N, -1), score[:, None]], axis=1)
        self.final_obs[done] = obs[done]
        self.episode[done] += 1
        start, _, flags, _ = self.goals
        nxt = np.where(self.goal_index >= 0, (self.goal_index + GOAL_STRIDE) % N_GOALS, -1).astype(np.int32)
        self.goal_index = np.where(done, nxt, self.goal_index).astype(np.int32)
        m = done.astype(np.uint8)
        env.reset(m)
        poses = env.host(nat.F_OBJ_POSE)
        for e in np.flatnonzero(done):
            if self.goal_index[e] >= 0:
                named = (flags[self.goal_index[e]] & 2) != 0
                poses[e, named] = start[self.goal_index[e], named]
        env.set_object_poses(poses, m)
        env.set_env_goals(self.goal_index, m)

    def _camera(self, eye, target, fov):
        from real_robots_amd.mathutil import look_at, perspective
        return (np.asarray(look_at(tuple(eye), tuple(target), (0.0, 0.0, 1.0)), np.float32),
                np.asarray(perspective(float(fov), self.env.W / self.env.H, 0.1, 100.0), np.float32))

    def _set_camera(self, op):
        self.env.set_camera(*self._camera(op['eye'], op['target'], op['fov']))

    def _set_camera_default(self, op):
        self.env.set_camera(None, None)

    def _set_env_cameras(self, op):
        cams = [self._camera(op['eye'][i], op['target'][i], op['fov'][i]) for i in range(self.N)]
        self.env.set_env_cameras(np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), op['mask'])

    def _set_env_appearance(self, op):
        self.env.set_env_appearance(colours=op['tint'][:, None, :], light_dirs=op['light'], env_mask=op['mask'])

    def _select_image_mirror(self, op):
        sel = op['sel']
        self.env.select_image_mirror(rgb=bool(sel & 1), depth=bool(sel & 2), mask=bool(sel & 4))
        self.sel = sel

    # ---- observers: the device road calls them where the programme says; the host road only where a comparison needs them.  An
    # episode update without reset is the exception: it moves the previous score, which the next reward reads, so every road makes it
    def _observe(self, op):
        return self.road != 'host'

    def _ray_table(self, op):
        if self._observe(op):
            self.env.ray_cast()

    def _ray_dev(self, op):
        if self._observe(op):
            self.env.ray_cast(self._d(op['segments']))

    def _kinematic_observations(self, op):
        if self._observe(op):
            self.env.kinematic_observations()

    def _contact_observations(self, op):
        if self._observe(op):
            self.env.contact_observations()

    def _read_state(self, op):
        if self._observe(op):
            self.env.read_state()

    def _link_poses(self, op):
        if self._observe(op):
            self.env.link_poses()

    def _evaluate_goals(self, op):
        if self._observe(op):
            self.env.evaluate_goals(op['goal_pos'], op['goal_mask'])

    def _episode_peek(self, op):
        self.env.episode_update(False)

    def _contacts(self, op):
        if self._observe(op):
            self.env.contacts(op['env'])

    def _sync(self, op):
        if self._observe(op):
            self.env.sync()

    def _sync_observations(self, op):
        if self._observe(op):
            self.env.sync_observations()

    # ---- the query tables: settings of the handle, host calls on every road
    def _set_distance_pairs(self, op):
        self.env.set_distance_pairs(op['pairs'], op['max_distance'])
        self.max_distance = op['max_distance']
        for f in ('dist', 'pc', 'sd', 'sg', 'sw'):      # (laid out by the Q in force: an earlier record's results can no longer be read)
            self.last.pop(f, None)

    def _set_kinematic_points(self, op):
        self.env.set_kinematic_points(op['links'].tolist(), op['local'])
        self.points = (op['links'], op['local'])
        self.last.pop('pk', None)                       # (laid out by the P in force)

    def _set_rays(self, op):
        self.env.set_rays(op['links'].tolist(), op['segments'])
        self.n_rays = len(op['links'])

    # ---- query observers: A makes every call, with device tensors; B the compared ones, with host arrays
    def _asks(self, op):
        """whether this road makes the record's call; notes which result buffers it writes"""
        if self.road == 'host' and not op['compared']:
            return False
        for f in FAMILY[op['kind']]:
            self.last[f] = op
        return True

    def _q(self, a):
        return a if self.road == 'host' else self._d(a)

    def margin(self, m):
        """a gradient's margin may not exceed the cull of the table in force"""
        return m if self.max_distance is None else min(m, self.max_distance)

    def ik_targets(self, goals):
        """float32 [N, K, 7]: the float64 tool pose (tests/numpy_pik.py) of the goal postures at the LAST point in force"""
        from tests import numpy_pik as npk
        from tests.numpy_kinematics import mat_to_quat
        Re, x, _ = npk.tool_frame(goals.astype(np.float64), int(self.points[0][-1]), self.points[1][-1].astype(np.float64))
        return np.ascontiguousarray(np.concatenate([x, mat_to_quat(Re)], -1).astype(np.float32))

    def _closest_points(self, op):
        if self._asks(op):
            self.env.closest_points()

    def _posture_clearance(self, op):
        if self._asks(op):
            self.env.posture_clearance(self._q(op['postures']))

    def _signed_distance(self, op):
        if self._asks(op):
            self.env.signed_distance()

    def _signed_distance_at(self, op):
        if self._asks(op):
            self.env.signed_distance(self._q(op['postures']))

    def _signed_distance_gradient(self, op):
        if self._asks(op):
            self.env.signed_distance_gradient(self._q(op['postures']), margin=self.margin(op['margin']))

    def _swept_clearance(self, op):
        if self._asks(op):
            self.env.swept_clearance(self._q(op['segments']), safety=op['safety'])

    def _posture_kinematics(self, op):
        if self._asks(op):
            self.env.posture_kinematics(self._q(op['postures']))

    def _posture_ik(self, op):
        if self._asks(op):
            seeds = self._q(op['seeds']) if 'seeds' in op else None
            self.env.posture_ik(self._q(self.ik_targets(op['goals'])), seeds, point=len(self.points[0]) - 1, max_iterations=op['max_iterations'],
                                position_only=op['position_only'], clamp=op['clamp'])

    _posture_ik_present = _posture_ik

    # ---- the command programmes: tables, attachments, macro actions decided on the device
    def _mask_arg(self, op):
        return None if op['mask'] is None else op['mask'] if self.road == 'host' else self._d(op['mask'])

    def _set_table(self, op, key, call, buffer):
        """A: a CUDA tensor and a device mask, or (`inplace`) the same rows written through the zero-copy view of the table, in the
        library's stream order; B: host arrays"""
        env = self.env
        if self.road == 'host':
            getattr(env, call)(op[key], op['mask'])
        elif op['inplace']:
            self.copy_in_place(env, buffer, self._d(op[key]), self._mask_arg(op))
        else:
            getattr(env, call)(self._d(op[key]), self._mask_arg(op))

    def _set_joint_torques(self, op):
        self._set_table(op, 'torques', 'set_joint_torques', 'joint_torque_buffer')

    def _set_external_wrenches(self, op):
        self._set_table(op, 'wrenches', 'set_external_wrenches', 'external_wrench_buffer')

    def _clear_joint_torques(self, op):
        self.env.set_joint_torques(None, self._mask_arg(op))

    def _clear_external_wrenches(self, op):
        self.env.set_external_wrenches(None, self._mask_arg(op))

    def _torques_from_dynamics(self, op):
        """A: the [N, 1, 11] bias view of posture_dynamics() straight into set_joint_torques -- no copy, no wait; B: the host array"""
        self._asks(op)
        if self.road == 'host':
            self.env.set_joint_torques(self.env.posture_dynamics(host=True)['bias'][:, 0], op['mask'])
        else:
            self.env.set_joint_torques(self.env.posture_dynamics()['bias'], self._mask_arg(op))

    def _attach(self, op):
        self.env.attach_objects(op['links'], op['rel'], op['mask'])
        self.attached = True

    def _attach_capture(self, op):
        self.env.attach_objects(op['links'], None, op['mask'])
        self.attached = True

    def _detach(self, op):
        self.env.detach_objects(op['mask'])

    def _detach_all(self, op):
        self.env.detach_objects()
        self.attached = False

    def _macro_invalidate(self, op):
        self.macro.apply(op)
        self.env.macro_invalidate(self._mask_arg(op))

    def _step_macro(self, op):
        self.macro.apply(op)
        self.macro_now = self.macro.replanned.copy()
        if self.road == 'host':
            self.env.step_macro_device(op['macro'], idle=op['idle'], render=self._render_arg(op))
        else:
            self.env.step_macro_device(self._d(op['macro']), idle=self._d(op['idle']), render=self._render_arg(op))

    def _posture_dynamics(self, op):
        if self._asks(op):
            arg = lambda a: None if a is None else self._q(a)
            self.env.posture_dynamics(arg(op['postures']), arg(op['velocities']), arg(op['accelerations']), inverse=op['inverse'])

    def _carried_sweep(self, op):
        if self._asks(op):
            self.env.carried_sweep(self._q(op['segments']), safety=op['safety'])

    def _sweep_bytes(self):
        return [np.asarray(self.env.sweep_buffer(i, host=True)).tobytes() for i in range(4)] if self.strict else None

    def _swept_clearance_refused(self, op):
        """while attachments are on the call raises RR_EINVAL and changes no buffer (`strict`: on a real handle)"""
        if not self._asks(op):
            return
        before = self._sweep_bytes()
        try:
            self.env.swept_clearance(self._q(op['segments']), safety=op['safety'])
        except RuntimeError as e:
            assert 'error -1' in str(e) and 'attach' in str(e), e
            self.refusals += 1
        else:
            assert not self.strict, "swept_clearance did not refuse while attachments are on"
        assert self._sweep_bytes() == before, "a refused swept_clearance changed a sweep buffer"

    def _read_back(self, op):
        """the table read-backs: a compared record's arrays are kept for the comparison (`read`)"""
        if self._asks(op):
            got = getattr(self.env, op['kind'])()
            self.read[op['kind']] = (op, got if isinstance(got, tuple) else (got,))

    _joint_torques = _external_wrenches = _attachments = _read_back


ANCHOR_ENVS = 4


def anchor_references(op, nobj, probe_q):
    """The float64 restatements on the state a record defines (is_anchor), for the first ANCHOR_ENVS envs, the
    default pair table and the probe's arguments: (state, pairs, reference at the present joints, reference at the probe's
    postures).  tests/test_session_program.py asserts the decided share of both for the very records of q70 and q5."""
    from tests import numpy_distance as nd
    from tests import numpy_posture as npo
    names = nd.names()
    pairs = np.array([(names[x], names[y]) for x, y in default_pairs(nobj)], np.int32)
    st = compose_state(op['rows'], nobj)[:ANCHOR_ENVS]
    return st, pairs, nd.reference(st, pairs), nd.reference(npo.rows(st, probe_q['postures'][:len(st)]), pairs)


def command_anchor_references(attach, op, nobj, probe_q, rel=None):
    """The float64 restatements behind an anchor of a command programme (is_command_anchor), for the first ANCHOR_ENVS envs, the
    default pair table, the attach record in force and the probe's postures.  `rel`: the poses the handle reads back (attachments();
    None: the record's own, the quaternion normalised).  Returns the state, the pairs, the links and poses padded to three objects,
    numpy_distance.reference on the carried rows (tests/numpy_carry.py) at the present joints and at the postures, which items have a
    shape of an attached object, and the numpy_dynamics.reference of the present-state form."""
    from tests import numpy_carry as nc
    from tests import numpy_distance as nd
    from tests import numpy_dynamics as ndy
    names = nd.names()
    pairs = np.array([(names[x], names[y]) for x, y in default_pairs(nobj)], np.int32)
    st = compose_state(op['rows'], nobj)[:ANCHOR_ENVS]
    n = len(st)
    links = np.full((n, 3), -1, np.int32)
    links[:, :nobj] = attach['links'][:n]
    given = np.asarray(attach['rel'] if rel is None else rel, np.float64)[:n]
    rel3 = np.zeros((n, 3, 7))
    rel3[..., 6] = 1.0
    rel3[:, :nobj] = given
    rel3[..., 3:] /= np.linalg.norm(rel3[..., 3:], axis=-1, keepdims=True)
    po = probe_q['postures'][:n]
    now = np.ascontiguousarray(st[:, None, :11])
    return dict(state=st, pairs=pairs, links=links, rel=rel3,
                now=nd.reference(nc.carried_rows(st, now, links, rel3), pairs), po=nd.reference(nc.carried_rows(st, po, links, rel3), pairs),
                att_now=nc.attached_items(links, pairs, 1), att_po=nc.attached_items(links, pairs, po.shape[1]),
                dynamics=ndy.reference(now, np.ascontiguousarray(st[:, None, 11:22])))


def probe_arguments(N, nobj):
    """the fixed arguments of the queries a comparison calls (tests/test_gpu_session.py), as host arrays: K = 2 postures, 2 segments
    and 2 IK targets per env -- the tool poses of two postures at the point of a fresh handle -- with their seeds"""
    from tests import numpy_pik as npk
    from tests.numpy_kinematics import mat_to_quat
    d = _Draw(np.random.default_rng([98, N]), N, nobj)
    po, goals = d.postures(PROBE_K), d.postures(PROBE_K)
    seg = np.ascontiguousarray(np.stack([d.postures(PROBE_K), d.postures(PROBE_K)], axis=2))
    seg[:, :, 1] = seg[:, :, 0] + np.float32(0.25) * (seg[:, :, 1] - seg[:, :, 0])      # the first quarter of the way: the advancement's
    seeds = goals.copy()                                                                 # steps are most of the probe's time
    seeds[..., :7] += d.rng.uniform(-0.3, 0.3, seeds[..., :7].shape).astype(np.float32)
    Re, x, _ = npk.tool_frame(goals.astype(np.float64))
    targets = np.ascontiguousarray(np.concatenate([x, mat_to_quat(Re)], -1).astype(np.float32))
    # (drawn behind everything above: the probe of the sessions from before the command programmes is what it was)
    qd, qdd = (np.ascontiguousarray(d.rng.uniform(-s, s, po.shape).astype(np.float32)) for s in (1.0, 5.0))
    return dict(postures=po, segments=seg, targets=targets, seeds=seeds, velocities=qd, accelerations=qdd)


def run(env, ops, road, to_device=torch_device, setup=True):
    """executes a programme on a handle and returns its Session"""
    s = Session(env, road, to_device)
    if setup:
        s.setup()
    for op in ops:
        s.apply(op)
    return s
