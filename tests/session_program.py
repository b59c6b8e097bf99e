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

# the sessions of tests/test_gpu_session.py: name -> (seed, N, objects, width, height, ops); the seed was fixed once, for the
# coverage the device reports (NOTEBOOK.md), and is never changed to make a comparison pass
Q_LENGTH = 74                               # what the conditions of a query programme cost (below)
SESSIONS = {'n70': (20261, 70, 3, 64, 64, 200), 'n5': (20262, 5, 1, 96, 64, 200), 'n1100': (20263, 1100, 3, 32, 32, 200),
            'q70': (20264, 70, 3, 64, 64, Q_LENGTH), 'q5': (20265, 5, 1, 96, 64, Q_LENGTH)}
QUERY_SESSIONS = ('q70', 'q5')              # drawn with program(..., queries=True)

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


def program(seed, N, nobj, length, queries=False):
    """list of `length` op records (dicts with a 'kind'); the same arguments give the same programme"""
    if queries:
        return _query_program(seed, N, nobj, length)
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
    return op['kind'] in STEP_KINDS


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
    return dict(postures=po, segments=seg, targets=targets, seeds=seeds)


def run(env, ops, road, to_device=torch_device, setup=True):
    """executes a programme on a handle and returns its Session"""
    s = Session(env, road, to_device)
    if setup:
        s.setup()
    for op in ops:
        s.apply(op)
    return s
