"""GPU tests (-m gpu) of the handle's bookkeeping across calls: seeded programmes of interleaved API calls (tests/session_program.py,
whose coverage tests/test_session_program.py asserts) run on the default handle and on a twin that takes the plainest road the
library has, compared BIT FOR BIT after every call.  No tolerance anywhere: both sides run the same kernels on the same inputs.

Handle A: the default handle (look-ahead, heavy / light split on side streams, persistent images), the device road for every op --
device masks, indices, command buffers and state tensors --, mapped observation and image mirrors, observers wherever the programme
has one.  Handle B: RR_NO_LOOKAHEAD, RR_NO_SPLIT and RR_FULL_COPY, host masks, indices and commands, for write_state the matching
reset / set_object_poses / state = calls where the header names them bitwise equal, for the auto-reset the host route of
tests/test_gpu_episode.py; observers only where a comparison makes them.

After every step-kind op: state, touch, contact count, every env's contacts(i), error flags, clock, joints, object poses; rgb, depth
and mask; every episode buffer; the outputs of every observer, called on both handles there; A's mapped mirrors against A's own
device buffers.  After every mutator the same without B's images: a mutator does not render, so A's images equal A's own of before.
Not compared: RR_F_ENV_CLASS, RR_F_PREP, the fragment lists and counts, timing -- they differ between the roads by design.

Three things are not a plain A == B:
* episode_update(reset_done=False) is an observer of the state but not of the episode record -- "the previous score becomes the
  score" (include/realrobot.h) --, so B makes that call where the programme has it, like A;
* B's host route of the auto-reset has no call that counts episodes or writes the final observation: A's `episode` and `final_obs`
  are compared with what the route's own host arithmetic says they must be (session_program.Session._episode_reset);
* at 1100 envs contacts(i) is called for the 16 envs whose images are compared; the rows of all envs are compared through
  contact_observations, whose `contacts` field is those rows for the whole batch.
Both handles start from the 60-step run of tests/test_gpu_fork.py, which has contact history.

Beside the three sizes: the 70-env programme twice on the default handle for one digest per op; once more with no wait of the test's
between comparisons; and, for every mutator kind, the proof that the compared fields move when the call is made.

The read-only batch queries.  Every comparison -- of all of the above -- also makes the nine query calls on the handle (QUERIES:
closest_points, posture_clearance, signed_distance at the present state and at postures, signed_distance_gradient, swept_clearance,
posture_kinematics, posture_ik with and without seeds) with small fixed arguments (session_program.probe_arguments: 2 postures, 2
segments, 2 targets per env, 8 IK iterations; CUDA tensors on the device road, host arrays on the host road), the pair, point and ray
tables whatever the handle has at that moment, and compares every output column.  Two more sessions, q70 and q5, run a QUERY
programme: the three tables change in the middle of the run, and query records with their own arguments (1, 3 or 32 rows per env)
stand directly behind device-side forks, snapshot loads, masked writes, resets, auto-resets and restores and directly in front of the
next step.  A `compared` record is made by B too, from host arrays, and the result buffers are compared as that call left them; a
silent one is A's alone, and the next comparison shows that it changed nothing.  What a bit compare cannot see -- an error both roads
share -- the float64 anchor does: behind a set_state and a full write_state the state is known on the CPU, and A's probe outputs
are held against the float64 restatements of tests/numpy_distance.py, numpy_posture.py, numpy_kinematics.py and numpy_pik.py within
the bounds of their own GPU tests (`_anchor`).  Invariants asserted on the way: the candidate queries (posture_kinematics, posture_ik
with seeds) give the same bits at every comparison between two set_kinematic_points; posture_ik without seeds changes only in envs
whose joints changed; the three table mutators move query and ray outputs and nothing else; a write of the object poses alone, or of
the joints alone, moves every probe output that reads them.

The command-side state.  Two more sessions, c70 and c5, run a COMMAND programme (session_program.program(..., commands=True), 212
ops): the joint torque and external wrench tables -- set from CUDA tensors with device masks, once per table through the zero-copy
view, cleared under a mask and without one, and `torques_from_dynamics`: the bias view of posture_dynamics() passed straight into
set_joint_torques with no copy and no wait --, the attachments (given poses, the capture kernel, masked detach, the unmasked detach)
and the device-resident macro actions (step_macro with device requests and idle masks, macro_invalidate) stand between the steps of
the default handle; B gets host arrays.  Each of reset, fork, load_snapshot, restore, the auto-reset, set_state and the masked
writes of the joints and of the object poses stands with both tables non-zero, with attachments on and directly behind a step_macro
with plans in flight, with a step_macro behind it, and once more behind the three unmasked clearing calls (the feature-off road).  A
comparison of a command session looks at everything above and at the three tables, the macro request record, positions and
`replanned` bytes, the plans of the envs that the op re-planned and of four others, posture_dynamics at the present state and at the
probe's rows, and carried_sweep; while attachments are on the probe's posture_clearance, signed_distance and gradient run their
_carry kernels and swept_clearance, which refuses then, is left out (`swept_clearance_refused` records assert the refusal and that no
buffer changed).  With attachments off a carried_sweep record's four buffers are compared with a swept_clearance of the same
segments on the same handle.  A and B both run k_macro_decide, so A's record, positions and `replanned` bytes are ALSO held against
the Session's numpy model of the header's decision rule, behind every compared op: a record that followed the source env of a fork
would differ from it.  The float64 anchor of a command session (`_command_anchor`): behind a set_state and a full write_state, each
directly behind an attach of known poses, posture_dynamics() against tests/numpy_dynamics.py and the carried posture_clearance and
signed_distance against tests/numpy_carry.py, within the bounds of those modules' own GPU tests."""
import hashlib
import time

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests import session_program as sp

pytestmark = pytest.mark.gpu

PLAIN = {'RR_NO_LOOKAHEAD': '1', 'RR_NO_SPLIT': '1', 'RR_FULL_COPY': '1'}
T_WARM = 60
STATE_FIELDS = dict(touch=nat.F_TOUCH, count=nat.F_CONTACT_COUNT, errflags=nat.F_ERRFLAGS, timestep=nat.F_TIMESTEP, joints=nat.F_JOINTS,
                    obj_pose=nat.F_OBJ_POSE)
IMAGE_FIELDS = dict(rgb=nat.F_RGB, depth=nat.F_DEPTH, mask=nat.F_MASK)
_cache = {}
_spent = {'queries': 0.0}     # wall time of the query probes of the comparisons, reported beside every session's time


def _make(monkeypatch, env_vars, *args, **kw):
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    try:
        return BatchedREALRobotEnv(*args, **kw)
    finally:
        for k in env_vars:
            monkeypatch.delenv(k, raising=False)


def _program(name):
    if name not in _cache:
        seed, N, nobj, _, _, length = sp.SESSIONS[name]
        _cache[name] = sp.program(seed, N, nobj, length, queries=name in sp.QUERY_SESSIONS, commands=name in sp.COMMAND_SESSIONS)
    return _cache[name]


def _took(t0):
    q, _spent['queries'] = _spent['queries'], 0.0
    return "%.1f s, %.1f s of it in the query probes of the comparisons" % (time.perf_counter() - t0, q)


def _silent(op):
    """an observer that B does not make: no comparison behind it, the next one shows whether A's call changed anything"""
    if op['kind'] in sp.Q_OBSERVERS + sp.C_OBSERVERS:
        return not op['compared']
    return op['kind'] in sp.OBSERVERS and op['kind'] != 'episode_peek'


def _warm_up(envs, N):
    """the run of tests/test_gpu_fork.py: commands keyed by env id, a frame every seventh step"""
    for t in range(T_WARM):
        cmd = synthetic_actions(range(N), t, seed=5).astype(np.float32)
        for e in envs:
            e.step(cmd, render=(t % 7 == 0))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _differing(x, y):
    """envs (first axis) at which x and y differ in a bit; a list of per-env arrays compares row by row"""
    if isinstance(x, list):
        return np.flatnonzero([a.shape != b.shape or not np.array_equal(_bits(a), _bits(b)) for a, b in zip(x, y)])
    x, y = _bits(x), _bits(y)
    assert x.shape == y.shape, (x.shape, y.shape)
    return np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))


class _Probe:
    """the fixed arguments of the observers a comparison calls"""

    def __init__(self, N, nobj):
        d = sp._Draw(np.random.default_rng([99, N]), N, nobj)
        self.segments = d.observer('ray_dev')['segments']
        self.segments_dev = sp.torch_device(self.segments)
        g = d.observer('evaluate_goals')
        self.goal_pos, self.goal_mask = g['goal_pos'], (np.arange(N * nobj).reshape(N, nobj) % 3 != 0).astype(np.uint8)
        # per-env segments for every size of the ray table a programme sets: the four above, their first, sixteen shifted copies
        wide = np.tile(self.segments, (1, 16, 1)) + (np.arange(64) // 4 * np.float32(0.004)).astype(np.float32)[None, :, None]
        self.rays = {1: np.ascontiguousarray(self.segments[:, :1]), 4: self.segments, 64: np.ascontiguousarray(wide.astype(np.float32))}
        self.rays_dev = {R: self.segments_dev if R == 4 else sp.torch_device(a) for R, a in self.rays.items()}
        self.q = sp.probe_arguments(N, nobj)
        self.q_dev = {k: sp.torch_device(a) for k, a in self.q.items()}


QUERIES = ('closest_points()', 'posture_clearance(po)', 'signed_distance()', 'signed_distance(po)', 'signed_distance_gradient(po)',
           'swept_clearance(seg)', 'posture_kinematics(po)', 'posture_ik(targets, seeds)', 'posture_ik(targets)')
READS_JOINTS = ('closest_points()', 'signed_distance()', 'posture_ik(targets)')
# the fields that the query tables move: the nine above, the rays, and the points of the kinematic observations
TABLE_FIELDS = QUERIES + ('ray_cast', 'kinematic.point_', 'kinematic.jacobian')


def _queries(env, sess, probe):
    """the nine query calls with the probe's arguments -- device tensors on the device road, host arrays on the host road --, the
    tables whatever the handle has at the moment, the IK at the last point: {'call.column': host array}"""
    q = probe.q if sess.road == 'host' else probe.q_dev
    ik = dict(point=len(sess.points[0]) - 1, max_iterations=sp.PROBE_ITERATIONS, host=True)
    grad = lambda: {k: v for k, v in env.signed_distance_gradient(q['postures'], margin=sess.margin(sp.PROBE_MARGIN), host=True).items()
                    if k in ('gradient', 'cost', 'cost_gradient', 'pair_distance')}      # (the rest are signed_distance's bytes once more)
    calls = (lambda: env.closest_points(host=True), lambda: env.posture_clearance(q['postures'], host=True), lambda: env.signed_distance(host=True),
             lambda: env.signed_distance(q['postures'], host=True), grad, lambda: env.swept_clearance(q['segments'], host=True),
             lambda: env.posture_kinematics(q['postures'], host=True), lambda: env.posture_ik(q['targets'], q['seeds'], **ik),
             lambda: env.posture_ik(q['targets'], **ik))
    # (a command session: swept_clearance refuses while attachments are on -- carried_sweep, below, is the edge check then -- and the
    # three posture queries of this probe run their _carry kernels)
    return {name + '.' + k: np.array(v) for name, call in zip(QUERIES, calls) if not (sess.attached and name == 'swept_clearance(seg)')
            for k, v in call().items()}


C_QUERIES = ('posture_dynamics()', 'posture_dynamics(po, qd, qdd, inverse)', 'carried_sweep(seg)')


def _command_fields(env, sess, probe):
    """what a comparison of a command session looks at besides: the three tables, the macro buffers -- the plans of the envs that this
    op re-planned (the Session's model says which) and of the first ANCHOR_ENVS --, and the probe of the new queries"""
    q = probe.q if sess.road == 'host' else probe.q_dev
    d = {'table.joint_torques': env.joint_torques(), 'table.external_wrenches': env.external_wrenches()}
    d['table.attach_links'], d['table.attach_rel'] = env.attachments()
    for name in ('request', 'position', 'replanned'):
        d['macro.' + name] = env.macro_buffer(name, host=True)
    sel = np.union1d(np.flatnonzero(sess.macro_now), np.arange(min(sess.N, sp.ANCHOR_ENVS)))
    d['macro.plan'] = env.macro_buffer('plan', host=True)[sel]
    t0 = time.perf_counter()
    calls = (lambda: env.posture_dynamics(host=True), lambda: env.posture_dynamics(q['postures'], q['velocities'], q['accelerations'], inverse=True, host=True),
             lambda: env.carried_sweep(q['segments'], host=True))
    d.update({name + '.' + k: np.array(v) for name, call in zip(C_QUERIES, calls) for k, v in call().items()})
    _spent['queries'] += time.perf_counter() - t0
    return d


_RAW = {'dist': ('distance_buffer', nat.DIST_FIELDS), 'pc': ('posture_buffer', nat.PC_FIELDS), 'sd': ('signed_buffer', nat.SD_FIELDS),
        'sg': ('signed_gradient_buffer', nat.SG_FIELDS), 'sw': ('sweep_buffer', nat.SW_FIELDS), 'pk': ('posture_kinematics_buffer', nat.PK_FIELDS),
        'pik': ('posture_ik_buffer', nat.PIK_FIELDS), 'pd': ('posture_dynamics_buffer', nat.PD_FIELDS)}


def _results(env, sess, families):
    """the result buffers of the query records that wrote them last, as their own calls left them: {'family.buffer': host array}.
    Two buffers are written at the present state only (RR_SD_POINTS, RR_SG_PAIR_GRADIENT): they are read behind such a call alone."""
    d = {}
    for f in families:
        present = sess.last[f]['kind'] == 'signed_distance'
        for name in _RAW[f][1]:
            if (f, name) == ('pd', 'mass_inverse') and not sess.last[f]['inverse']:
                continue                    # (written with inverse=True only: else it holds an earlier call's bytes, and A makes more calls than B)
            if (f, name) not in (('sd', 'points'), ('sg', 'pair_gradient')) or (f == 'sd' and present):
                d[f + '.' + name] = getattr(env, _RAW[f][0])(name, host=True)
    return d


def _collect(env, sess, probe, img_envs, contact_envs, images=True):
    """everything a comparison looks at, as host arrays: {field: [N, ...] array or list per env}"""
    import torch
    d = {'state': env.state}
    for k, f in STATE_FIELDS.items():
        d[k] = env.host(f)
    d['contacts(i)'] = [env.contacts(int(i)) for i in contact_envs]
    for name in nat.EP_NAMES:
        d['episode.' + name] = env.episode_buffer(name, host=True)
    if sess.road == 'host':                 # (the host route's own count and final observation: the module's docstring)
        d['episode.episode'], d['episode.final_obs'] = sess.episode.copy(), sess.final_obs.copy()
    for k, v in env.ray_cast(host=True).items():
        d['ray_cast().' + k] = v
    for k, v in env.ray_cast((probe.rays if sess.road == 'host' else probe.rays_dev)[sess.n_rays], host=True).items():
        d['ray_cast(rays).' + k] = v
    t0 = time.perf_counter()
    d.update(_queries(env, sess, probe))
    _spent['queries'] += time.perf_counter() - t0
    if sess.commands:
        d.update(_command_fields(env, sess, probe))
    for k, v in env.kinematic_observations(host=True).items():
        d['kinematic.' + k] = v
    for k, v in env.contact_observations(host=True).items():
        d['contact_obs.' + k] = v
    view = torch.from_dlpack(env.read_state())
    env.sync()
    d['read_state'] = view.cpu().numpy()
    d['link_poses'] = env.link_poses()
    d['evaluate_goals'] = env.evaluate_goals(probe.goal_pos, probe.goal_mask)
    if images:
        for k, f in IMAGE_FIELDS.items():
            d['image.' + k] = env.host(f)[img_envs]
    return d


def _digest(d):
    h = hashlib.blake2b(digest_size=16)
    for k in sorted(d):
        for a in (d[k] if isinstance(d[k], list) else [d[k]]):
            h.update(k.encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _where(i, ops):
    return "op %d (%s); the last five ops: %s" % (i, ops[i]['kind'], ', '.join("%d %s" % (j, ops[j]['kind']) for j in range(max(0, i - 4), i + 1)))


def _assert_equal(a, b, i, ops, what, envs_of=None, skip=()):
    for k in a:
        if k in skip or k not in b:
            continue
        if not isinstance(a[k], list) and a[k].shape != b[k].shape:        # (a table of another size on one side)
            raise AssertionError("%s: %s: field %s has shape %s against %s" % (_where(i, ops), what, k, a[k].shape, b[k].shape))
        bad = _differing(a[k], b[k])
        if bad.size:
            sel = envs_of.get(k) if envs_of else None
            envs = (np.asarray(sel)[bad] if sel is not None else bad)[:16].tolist()
            raise AssertionError("%s: %s: field %s differs in envs %s" % (_where(i, ops), what, k, envs))


def _check_mirrors(A, sess, mirror, img_mirror, a, img_envs, i, ops):
    """A's mapped mirrors against A's own device buffers, as the comparison has just read them into `a` (valid after sync)"""
    A.sync()
    for k in ('joints', 'touch', 'obj_pose', 'timestep', 'errflags'):
        bad = _differing(mirror[k].copy(), a[k])
        assert bad.size == 0, "%s: the mapped observation mirror: %s differs from the device buffer in envs %s" % (_where(i, ops), k, bad[:16].tolist())
    for bit, k in enumerate(IMAGE_FIELDS):
        if sess.sel >> bit & 1:
            bad = _differing(img_mirror[bit][img_envs], a['image.' + k])
            assert bad.size == 0, "%s: the mapped image mirror: %s differs from the device buffer in envs %s" % (_where(i, ops), k, img_envs[bad][:16].tolist())


class _Twin:
    """the default handle A with its mirrors and the plain-road twin B (or A alone), warmed up and set up"""

    def __init__(self, monkeypatch, name, road_a='device', twin=True):
        _, N, nobj, W, H, _ = sp.SESSIONS[name]
        self.name, self.N, self.ops = name, N, _program(name)
        self.A = BatchedREALRobotEnv(N, objects=nobj, width=W, height=H)
        self.B = _make(monkeypatch, PLAIN, N, objects=nobj, width=W, height=H) if twin else None
        self.envs = [e for e in (self.A, self.B) if e is not None]
        _warm_up(self.envs, N)
        self.sa = sp.Session(self.A, road_a)
        self.sb = sp.Session(self.B, 'host') if twin else None
        self.commands = name in sp.COMMAND_SESSIONS
        for s in (self.sa, self.sb):
            if s is not None:
                s.commands = self.commands
                s.setup()
        self.mirror, self.img_mirror = self.A.map_observations(), self.A.map_images()
        self.probe = _Probe(N, nobj)
        self.img_envs = np.arange(N) if N <= 128 else np.unique(np.concatenate([np.arange(6), [63, 64, 65, 511, 512, 1023, 1024], np.arange(N - 3, N)]))
        self.contact_envs = np.arange(N) if N <= 128 else self.img_envs
        self.envs_of = {'contacts(i)': self.contact_envs, **{'image.' + k: self.img_envs for k in IMAGE_FIELDS}}

    def close(self):
        self.mirror = self.img_mirror = None
        for e in self.envs:
            e.close()

    def collect_a(self):
        return _collect(self.A, self.sa, self.probe, self.img_envs, self.contact_envs)

    def collect_b(self, images):
        return _collect(self.B, self.sb, self.probe, self.img_envs, self.contact_envs, images=images)


def _anchor(tw, op, a, i, figures):
    """Behind a set_state, and behind a write_state of all four column groups with `fresh` and no mask, the state of every env is
    compose_state(rows), known on the CPU: A's probe outputs of the first four envs against the float64 restatements the project has,
    within the bounds of those restatements' own GPU tests (imported, not restated).  The default pair table is in force there
    (check_query_conditions).  The recipe states hold no overlapping pair -- the objects hang 3 to 15 cm above the table, 30 cm apart
    --: the overlapping regime stays with tests/test_gpu_signed_distance.py and with the bit compare against the twin.  The only
    omission is what the reference leaves undecided (within numpy_distance.DECIDE of touching); at least 95 % are decided."""
    from tests import numpy_distance as nd
    from tests import numpy_kinematics as nk
    from tests import numpy_pik as npk
    from tests import numpy_posture as npo
    from tests.test_gpu_distance import TOL as TOL_DISTANCE
    from tests.test_gpu_kinematic_obs import TOL_JV, TOL_JW, TOL_POS, TOL_QUAT, _align
    from tests.test_gpu_posture_ik import TOL_Q
    from tests.test_gpu_posture_kinematics import _figures as pk_figures, _reference as pk_reference
    from tests.test_gpu_posture_query import TOL as TOL_POSTURE
    where, n, nobj = _where(i, tw.ops), min(sp.ANCHOR_ENVS, tw.N), tw.sa.nobj
    assert (tw.A.distance_pairs()[1] == 0.0) and len(tw.A.distance_pairs()[0]) == len(sp.default_pairs(nobj)), where
    st, pairs, ref, ref_po = sp.anchor_references(op, nobj, tw.probe.q)
    cols = sp.part_columns(15, nobj)
    assert (_bits(a['state'][:, cols]) == _bits(sp.compose_state(op['rows'], nobj)[:, cols])).all(), "%s: the state is not the record's" % where
    fig = {}

    def judge(name, f, fails, decided, items):
        print("anchor %s %s %s: %s %s" % (tw.name, where.split(';')[0], name, {k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in f.items()}, fails))
        assert not fails, (where, name, fails)
        assert decided >= 0.95 * items and f.get('overlapping', 0) == 0, (where, name, decided, items)
        fig[name] = f['distance_error']
    cut = lambda call, **keys: {k: a[call + '.' + v][:n] for k, v in keys.items()}
    same = {k: k for k in ('distance', 'lower', 'point_a', 'point_b', 'normal', 'status')}
    f, fails = nd.compare(cut('closest_points()', **same), ref, TOL_DISTANCE, pairs)
    judge('closest_points', f, fails, f['decided'], f['items'])
    f, fails = nd.compare(cut('signed_distance()', distance='pair_distance', lower='pair_bound', point_a='pair_point_a', point_b='pair_point_b',
                              normal='pair_normal', status='pair_status'), ref, TOL_DISTANCE, pairs)
    judge('signed_distance', f, fails, f['decided'], f['items'])
    out = {k[len('posture_clearance(po).'):]: v[:n].reshape((-1,) + v.shape[2:]) for k, v in a.items() if k.startswith('posture_clearance(po).')}
    f, fails = npo.compare(out, ref_po, TOL_POSTURE, pairs)
    judge('posture_clearance', f, fails, f['decided'], f['items'])
    # link poses of the present state and of the candidates, the points in force
    links, local = tw.sa.points[0].tolist(), tw.sa.points[1].astype(np.float64)
    kin = nk.observations(st, links, local)
    lp = a['kinematic.link_pose'][:n].astype(np.float64)
    fig['link_pos'] = float(np.abs(lp[..., :3] - kin['link_pos']).max())
    fig['link_quat'] = float(np.abs(_align(lp[..., 3:], kin['link_quat']) - kin['link_quat']).max())
    fig['point_pos'] = float(np.abs(a['kinematic.point_pos'][:n] - kin['point_pos']).max())
    pk = pk_figures({k: a['posture_kinematics(po).' + k][:n] for k in nat.PK_FIELDS}, pk_reference(tw.probe.q['postures'][:n], links, local))
    fig.update({'pk_' + k: float(v) for k, v in pk.items()})
    assert fig['link_pos'] < TOL_POS and fig['point_pos'] < TOL_POS and fig['link_quat'] < TOL_QUAT, (where, fig)
    assert fig['pk_link_pos'] < TOL_POS and fig['pk_point_pos'] < TOL_POS and fig['pk_link_quat'] < TOL_QUAT, (where, fig)
    assert fig['pk_jac_lin'] < TOL_JV and fig['pk_jac_ang'] < TOL_JW, (where, fig)
    # the IK lands where the float64 iteration lands: rows with the same number of updates, and the clear-cut rows converge
    K = tw.probe.q['targets'].shape[1]
    present = np.ascontiguousarray(np.broadcast_to(st[:, None, :11], (n, K, 11)))
    for call, seeds in (('posture_ik(targets, seeds)', tw.probe.q['seeds'][:n]), ('posture_ik(targets)', present)):
        want = npk.solve(tw.probe.q['targets'][:n].reshape(-1, 7), seeds.reshape(-1, 11), links[-1], local[-1], max_iterations=sp.PROBE_ITERATIONS)
        q, status, it = (a[call + '.' + k][:n].reshape((n * K,) + a[call + '.' + k].shape[2:]) for k in ('posture', 'status', 'iterations'))
        clear = (want['status'] == 0) & (want['iterations'] <= npk.CLEAR_CUT)
        count = it == want['iterations']
        assert count.any() and (status[clear] == 0).all(), (where, call, status, want['status'])
        fig[call] = float(np.abs(q.astype(np.float64) - want['posture']).max(-1)[count].max())
        assert fig[call] <= TOL_Q, (where, call, fig[call])
    print("anchor %s %s: %s" % (tw.name, where.split(';')[0], {k: float('%.3g' % v) for k, v in fig.items()}))
    for k, v in fig.items():
        figures[k] = max(figures.get(k, 0.0), v)
    figures['anchors'] = figures.get('anchors', 0) + 1


def _compare_results(tw, i, what):
    """the result buffers that the same query record wrote last on A and on B (a compared record: A from device tensors, B from
    host arrays), bit for bit, before the probe's calls of a comparison overwrite them"""
    both = [f for f in tw.sa.last if tw.sb.last.get(f) is tw.sa.last[f]]
    if both:
        _assert_equal(_results(tw.A, tw.sa, both), _results(tw.B, tw.sb, both), i, tw.ops,
                      "%s, the buffers of %s" % (what, ', '.join(sorted({tw.sa.last[f]['kind'] for f in both}))))
    tw.sa.last.clear()
    tw.sb.last.clear()


def _compare_read_backs(tw, i):
    """the arrays of a compared table read-back (joint_torques, external_wrenches, attachments), as the record's own calls returned them"""
    for kind, (op, got) in tw.sa.read.items():
        if kind in tw.sb.read and tw.sb.read[kind][0] is op:
            _assert_equal({'%s[%d]' % (kind, j): x for j, x in enumerate(got)}, {'%s[%d]' % (kind, j): x for j, x in enumerate(tw.sb.read[kind][1])},
                          i, tw.ops, "A against B, the read-back of the record")
    tw.sa.read.clear()
    tw.sb.read.clear()


def _forwards_to_swept_clearance(tw, op, i):
    """With attachments off rr_carried_sweep IS rr_swept_clearance: the four buffers of the record's call against those of a
    swept_clearance of the same segments on the same handle, bit for bit."""
    A = tw.A
    mine = [A.sweep_buffer(j, host=True) for j in range(len(nat.SW_FIELDS))]
    A.swept_clearance(tw.sa._q(op['segments']), safety=op['safety'])
    for name, x, y in zip(nat.SW_FIELDS, mine, [A.sweep_buffer(j, host=True) for j in range(len(nat.SW_FIELDS))]):
        bad = _differing(x, y)
        assert bad.size == 0, "%s: carried_sweep with attachments off: buffer %s differs from swept_clearance's in envs %s" % (_where(i, tw.ops), name, bad[:16].tolist())


def _against_the_macro_model(tw, a, i):
    """A's request record, plan positions and `replanned` bytes against the Session's numpy model of the header's decision rule (A and
    B both run k_macro_decide: the model is the independent reference), behind every compared op -- no state mutator may move them"""
    m = tw.sa.macro
    for name, want in (('request', m.record), ('position', m.position), ('replanned', m.replanned)):
        bad = _differing(a['macro.' + name], want)
        assert bad.size == 0, "%s: A's RR_MACRO_%s differs from the model of the decision rule in envs %s: %s against %s" % (
            _where(i, tw.ops), name.upper(), bad[:16].tolist(), a['macro.' + name][bad[:4]].tolist(), want[bad[:4]].tolist())


def _command_anchor(tw, attach, op, a, i, figures):
    """Behind the set_state and the full write_state of a command programme the state is the record's and the attach record in front
    of it is in force: for the first ANCHOR_ENVS envs, posture_dynamics() against tests/numpy_dynamics.py within that module's
    ceilings (a ratio of at most 1), and the probe's carried posture_clearance(po), signed_distance(po) and signed_distance() against
    tests/numpy_carry.py on the poses the handle reads back -- items with a shape of an attached object within test_gpu_carry.CEIL_D,
    the others within the siblings' bounds, every status the reference's.  No item is set aside: the reference decides them all
    (tests/test_session_program.py)."""
    from tests import numpy_dynamics as ndy
    from tests.test_gpu_carry import CEIL_D
    from tests.test_gpu_distance import TOL as TOL_DISTANCE
    from tests.test_gpu_posture_query import TOL as TOL_POSTURE
    from tests.test_gpu_signed_distance import TOL_SD
    where, n, nobj = _where(i, tw.ops), min(sp.ANCHOR_ENVS, tw.N), tw.sa.nobj
    assert attach.get('anchor') and attach['kind'] == 'attach' and (a['table.attach_links'] == attach['links']).all(), where
    assert (tw.A.distance_pairs()[1] == 0.0) and len(tw.A.distance_pairs()[0]) == len(sp.default_pairs(nobj)), where
    cols = sp.part_columns(15, nobj)
    assert (_bits(a['state'][:, cols]) == _bits(sp.compose_state(op['rows'], nobj)[:, cols])).all(), "%s: the state is not the record's" % where
    r = sp.command_anchor_references(attach, op, nobj, tw.probe.q, rel=a['table.attach_rel'])
    fig = {}
    scale = ndy.scales(r['dynamics'])
    for k in ('mass_matrix', 'gravity', 'bias', 'torque'):
        fig['dynamics_' + k] = float(ndy.row_ratios(a['posture_dynamics().' + k][:n], r['dynamics'], scale, k).max())
        assert fig['dynamics_' + k] <= 1.0, (where, k, fig)
    for call, key, clip in (('posture_clearance(po)', 'po', True), ('signed_distance(po)', 'po', False), ('signed_distance()', 'now', False)):
        ref, att = r[key], r['att_' + key]
        assert ref['decided'].all() and att.any() and not att.all(), (where, call)
        d = a[call + '.pair_distance'][:n].reshape(att.shape).astype(np.float64)
        err = np.abs(d - (np.maximum(ref['d'], 0.0) if clip else ref['d']))
        fig[call + ' attached'], fig[call + ' others'] = float(err[att].max()), float(err[~att].max())
        wrong = int((a[call + '.pair_status'][:n].reshape(att.shape) != ref['expect']).sum())
        print("anchor %s %s %s: attached items %d, error %.3g (bound %.3g); others %d, error %.3g (bound %.3g); status mismatches %d"
              % (tw.name, where.split(';')[0], call, att.sum(), err[att].max(), CEIL_D, (~att).sum(), err[~att].max(), max(TOL_POSTURE, TOL_SD, TOL_DISTANCE), wrong))
        assert err[att].max() <= CEIL_D and err[~att].max() <= max(TOL_POSTURE, TOL_SD, TOL_DISTANCE) and wrong == 0, (where, call, fig, wrong)
    print("anchor %s %s: %s" % (tw.name, where.split(';')[0], {k: float('%.3g' % v) for k, v in fig.items()}))
    for k, v in fig.items():
        figures[k] = max(figures.get(k, 0.0), v)
    figures['anchors'] = figures.get('anchors', 0) + 1


def _run_twin(tw, counts=None, figures=None):
    """the programme on A and B with a comparison behind every op; returns the number of comparisons"""
    ops, compared = tw.ops, 0
    before = tw.collect_a()
    _assert_equal(before, tw.collect_b(True), 0, ops, "before the programme, A against B", tw.envs_of)
    since_points = before
    for i, op in enumerate(ops):
        tw.sa.apply(op)
        tw.sb.apply(op)
        if op['kind'] == 'carried_sweep' and not tw.sa.attached:
            _forwards_to_swept_clearance(tw, op, i)
        if _silent(op):
            continue                        # B made no call: the next comparison shows whether A's changed anything
        _compare_results(tw, i, "A against B")
        _compare_read_backs(tw, i)
        a = tw.collect_a()
        if tw.commands:
            _against_the_macro_model(tw, a, i)
            if counts is not None and op['kind'] == 'step_macro':
                counts['replans'] += int(a['macro.replanned'].sum())
            if figures is not None and sp.is_command_anchor(op):
                _command_anchor(tw, ops[i - 1], op, a, i, figures)
        stepped = sp.is_step(op)
        _assert_equal(a, tw.collect_b(stepped), i, ops, "A against B", tw.envs_of)
        if not stepped:
            _assert_equal(a, before, i, ops, "A's images against A's own of before the call", tw.envs_of, skip=[k for k in a if not k.startswith('image.')])
        _check_mirrors(tw.A, tw.sa, tw.mirror, tw.img_mirror, a, tw.img_envs, i, ops)
        # what the header says of the candidate queries: tensors, model and points alone; without seeds, the joints besides
        if op['kind'] == 'set_kinematic_points':
            since_points = a
        _assert_equal(a, since_points, i, ops, "a candidate query against its own output since the last set_kinematic_points", None,
                      skip=[k for k in a if not k.startswith(('posture_kinematics(po).', 'posture_ik(targets, seeds).'))])
        if op['kind'] != 'set_kinematic_points':
            same = ~(_bits(a['state'][:, :11]) != _bits(before['state'][:, :11])).any(axis=1)
            for k in a:
                if k.startswith('posture_ik(targets).') and same.any():
                    bad = _differing(a[k][same], before[k][same])
                    assert bad.size == 0, "%s: %s changed in envs whose joints did not: %s" % (_where(i, ops), k, np.flatnonzero(same)[bad][:16].tolist())
        if figures is not None and sp.is_anchor(op) and not tw.commands:
            _anchor(tw, op, a, i, figures)
        compared += 1
        before = a
        for s in (tw.sa, tw.sb):
            s.release()
        if counts is not None and stepped and op['kind'] != 'render':
            counts['heavy'] += int((tw.A.host(nat.F_ENV_CLASS) > 0).sum())
            if op['kind'] == 'step_refused':
                flagged = (a['errflags'] & 2) != 0
                frozen = (a['errflags'] & 5) != 0           # (a frozen env is not stepped: its command is not looked at)
                assert (flagged | frozen)[op['refused']].all() and not flagged[~op['refused']].any(), _where(i, ops)
                counts['refused'] += int(flagged.sum())
        if counts is not None and op['kind'] == 'episode_reset':
            done = int((a['episode.done'] != 0).sum())
            counts['auto_resets'] += done
            counts['partial_auto_resets'] += int(0 < done < tw.N)
    if counts is not None:
        assert counts['auto_resets'] == int(tw.A.episode_buffer('episode', host=True).sum())
    return compared


def test_n70_against_the_plain_twin(monkeypatch):
    """70 envs, 3 objects, 64 x 64, 200 ops: a partial second group of 64 for k_state_rw and k_fork, ragged for the 4- and 8-env
    workgroups of rays and kinematics, above SMALL_N_MAX (the three-stream split and the bounded run-ahead are live).
    The device reports the coverage: envs in a heavy class at compared steps, device auto-resets, auto-resets of a part of the
    batch, refused commands, all > 0."""
    t0 = time.perf_counter()
    counts = dict(heavy=0, refused=0, auto_resets=0, partial_auto_resets=0)
    tw = _Twin(monkeypatch, 'n70')
    n = _run_twin(tw, counts)
    tw.close()
    print("session n70: coverage %s; %d compared ops; %s" % (counts, n, _took(t0)))
    assert counts['heavy'] > 0 and counts['auto_resets'] > 0 and counts['refused'] > 0 and counts['partial_auto_resets'] > 0, counts


def _run_alone(monkeypatch, road):
    """the 70-env programme on a fresh default handle alone, with the reads of a comparison behind every compared op: its digests"""
    tw = _Twin(monkeypatch, 'n70', road_a=road, twin=False)
    digests = []
    for i, op in enumerate(tw.ops):
        tw.sa.apply(op)
        if _silent(op):
            continue
        digests.append((i, _digest(tw.collect_a())))
        tw.sa.release()
    tw.close()
    return digests


def test_n70_twice_the_same(monkeypatch):
    """The 70-env programme on a fresh default handle along the device road, and once more on another fresh default handle with
    its calls made as the records are written (host and device forms mixed): the digest of every compared op -- state-like fields,
    contact lists, episode buffers, observer outputs, images -- is the same.  A race between a side stream and a call on the main
    stream shows as a difference here or against B."""
    t0 = time.perf_counter()
    first = _run_alone(monkeypatch, 'device')
    again = _run_alone(monkeypatch, 'written')
    assert len(first) == len(again)
    ops = _program('n70')
    for (i, want), (j, got) in zip(first, again):
        assert i == j and got == want, "%s: the second run of the default handle differs from the first" % _where(j, ops)
    print("session n70, the second run: %d digests; %s" % (len(again), _took(t0)))


def test_n5_one_chain_placement_one_object_wide_image(monkeypatch):
    """5 envs, 1 object, 96 x 64, 200 ops: the one-chain placement, P.nobj < 3 (state = s on both roads: the device form is bitwise
    rr_set_state on three objects only), an image that is not square."""
    t0 = time.perf_counter()
    tw = _Twin(monkeypatch, 'n5')
    n = _run_twin(tw)
    tw.close()
    print("session n5: %d compared ops; %s" % (n, _took(t0)))


def test_n1100_packed_solve(monkeypatch):
    """1100 envs, 3 objects, 32 x 32, 200 ops: above COOP_ALL_MAX -- the packed solve and the side-by-side step without camera.
    Images and contacts(i) of 16 envs (both ends, around the groups of 64 and 512); everything else of all envs."""
    t0 = time.perf_counter()
    tw = _Twin(monkeypatch, 'n1100')
    n = _run_twin(tw)
    tw.close()
    print("session n1100: %d compared ops; %s" % (n, _took(t0)))


def _query_session(monkeypatch, name):
    t0 = time.perf_counter()
    figures = {}
    tw = _Twin(monkeypatch, name)
    n = _run_twin(tw, figures=figures)
    tw.close()
    made = {k: sum(o['kind'] == k and o['compared'] for o in tw.ops) for k in sp.Q_OBSERVERS}
    print("session %s: %d compared ops, compared query records %s; anchors: worst figures %s; %s"
          % (name, n, made, {k: float('%.3g' % v) for k, v in figures.items()}, _took(t0)))
    assert figures['anchors'] == sum(sp.is_anchor(o) for o in tw.ops) >= 2


def test_q70_against_the_plain_twin(monkeypatch):
    """70 envs, 3 objects, 64 x 64, the query programme: the pair table, the kinematic points and the ray table change in the middle of
    the run (1, 14, 92 and 96 pairs, with and without a cull; 1 to 8 points; 1, 4 and 64 rays), and the nine query calls stand directly
    behind device-side forks, snapshot loads, masked writes, resets, auto-resets and restores and directly in front of the step after
    them, with 1, 3 and 32 rows per env.  A compared record is made by B too, from host arrays, and its result buffers are compared bit
    for bit as the call left them; a silent one by A alone.  Behind the set_state and the full write_state: the float64 anchor."""
    _query_session(monkeypatch, 'q70')


def test_q5_against_the_plain_twin(monkeypatch):
    """5 envs, 1 object, 96 x 64, the query programme: the one-chain placement, tables that may only name the one object."""
    _query_session(monkeypatch, 'q5')


def _command_session(monkeypatch, name):
    t0 = time.perf_counter()
    figures = {}
    counts = dict(heavy=0, refused=0, auto_resets=0, partial_auto_resets=0, replans=0)
    tw = _Twin(monkeypatch, name)
    n = _run_twin(tw, counts, figures)
    refusals = (tw.sa.refusals, tw.sb.refusals)
    tw.close()
    print("session %s: coverage %s; %d compared ops of %d; swept_clearance refused %d times on A, %d on B; anchors: worst figures %s; %s"
          % (name, counts, n, len(tw.ops), refusals[0], refusals[1], {k: float('%.3g' % v) for k, v in figures.items()}, _took(t0)))
    assert figures['anchors'] == sum(sp.is_command_anchor(o) for o in tw.ops) == 2
    assert counts['auto_resets'] > 0 and counts['replans'] > 0 and refusals[0] > 0 and refusals[1] > 0, (counts, refusals)
    return counts


def test_c70_against_the_plain_twin(monkeypatch):
    """70 envs, 3 objects, 64 x 64, the command programme: joint torques, external wrenches, attachments, the capture, macro requests
    and macro_invalidate between the steps of the default handle -- device tables, masks, requests and idle masks, the bias view of
    posture_dynamics() straight into set_joint_torques, once per table a write through the zero-copy view -- against host arrays on
    the plain road.  Every state mutator stands with both tables non-zero, attachments on and plans in flight, and once more with
    every feature off.  A's macro record, positions and `replanned` bytes are held against the numpy model of the decision rule behind
    every compared op; behind the set_state and the full write_state: the float64 anchor of posture_dynamics() and the carried queries.
    The device reports the coverage: envs in a heavy class, auto-resets and re-plans, all > 0."""
    counts = _command_session(monkeypatch, 'c70')
    assert counts['heavy'] > 0, counts


def test_c5_against_the_plain_twin(monkeypatch):
    """5 envs, 1 object, 96 x 64, the command programme: the one-chain placement; wrench rows for objects the handle does not have;
    only the one object can be attached."""
    _command_session(monkeypatch, 'c5')


class _NullEnv:
    """takes every call and does nothing: a dry run of a Session shows which device arguments a programme needs, in order"""

    def __init__(self, env):
        self.N, self.n_objects, self.W, self.H = env.N, env.n_objects, env.W, env.H

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        if name == 'posture_dynamics':      # (torques_from_dynamics passes the bias on)
            return lambda *a, **kw: {'bias': _NoMemory()}
        return lambda *a, **kw: None


class _NoMemory:
    def data_ptr(self):
        return 0


@pytest.mark.parametrize('name', ['n70', 'q70', 'c70'])
def test_free_running_between_comparisons(monkeypatch, name):
    """The comparisons above wait for the device behind every op, and B's host road waits inside its calls.  Here A runs the same
    70-env programme as a training loop would: every device argument is uploaded before the first op, and A makes the ops of a chunk
    -- up to the eighth compared op -- back to back before B makes its own, so A's calls on the library's stream follow each other
    with no wait but the library's own (a device-road write, fork, reset, observer or episode update is enqueued while the side
    streams still work on the step before).  A call that relied on a wait would differ from B at the end of the chunk.
    q70: every posture, segment, target and seed tensor of every query record is uploaded beforehand too, the device road of a query
    reads it in place and does not wait, and the result buffers that the chunk's last compared record of a kind wrote are compared."""
    t0 = time.perf_counter()
    tw = _Twin(monkeypatch, name)
    staged = []
    dry = sp.Session(_NullEnv(tw.A), 'device', to_device=lambda a: staged.append(np.array(a)) or _NoMemory())
    dry.copy_in_place = lambda *a: None
    dry.setup()
    for op in tw.ops:
        dry.apply(op)
    staged = [(a, sp.torch_device(a)) for a in staged]

    def take(a):
        want, t = staged.pop(0)
        assert want.shape == np.shape(a) and np.array_equal(want, a, equal_nan=True)
        return t
    tw.sa.dev = take
    compared, flushed, chunk = 0, 0, []
    for i, op in enumerate(tw.ops):
        chunk.append(op)
        compared += not _silent(op)
        if compared - flushed >= 8 or i == len(tw.ops) - 1:
            flushed = compared
            for o in chunk:
                tw.sa.apply(o)
            for o in chunk:
                tw.sb.apply(o)
            chunk = []
            _compare_results(tw, i, "A (free running) against B")
            _compare_read_backs(tw, i)
            a = tw.collect_a()
            if tw.commands:
                _against_the_macro_model(tw, a, i)
            _assert_equal(a, tw.collect_b(True), i, tw.ops, "A (free running) against B", tw.envs_of)
            _check_mirrors(tw.A, tw.sa, tw.mirror, tw.img_mirror, a, tw.img_envs, i, tw.ops)
    assert not staged
    tw.close()
    print("session %s, free running: %d compared ops, a comparison behind every eighth; %s" % (name, compared, _took(t0)))


def _first(ops, kind, **want):
    return next(o for o in ops if o['kind'] == kind and all(o.get(k) == v for k, v in want.items()))


def test_every_mutator_moves_the_next_step():
    """For each mutator kind, once (its first record of the 70-env programme): the same prefix with and without the op, then a
    step with the camera of every env and an episode update -- the compared fields differ, so a dropped invalidation behind that
    mutator would be visible to the comparisons above.  Prefix: step, checkpoint, plan_macro, set_camera, step.  Four kinds move
    something only through a later call, which both sides then make: set_object_home a reset; save_snapshot a step and a
    load_snapshot of its slot; checkpoint a step, a checkpoint and a restore (of the checkpoint before last); plan_macro 101
    step_plan calls in place of the step -- rows 0..99 of every plan go to the same posture whatever the macro action, so a new plan
    shows from row 100 on (in the programmes above a plan_macro is therefore a call that must change nothing yet).
    select_image_mirror moves A's mapped image mirror: the deselected block keeps the old frame.
    The three table mutators (their first records of the q70 programme; for set_distance_pairs the first that is not the default
    table) are a class of their own: every field they move is a query or ray output, at least one of their own calls moves, and no
    state or image field does.  Last, on one of the two handles: _state_writes_move_the_probe; and the kinds of the command programmes
    with the invariants the header gives them: _command_mutators_move."""
    name = 'n70'
    _, N, nobj, W, H, _ = sp.SESSIONS[name]
    ops = _program(name)
    X, Y = (BatchedREALRobotEnv(N, objects=nobj, width=W, height=H) for _ in range(2))
    _warm_up((X, Y), N)
    base = X.checkpoint()
    probe = _Probe(N, nobj)
    mirrors = [e.map_images() for e in (X, Y)]
    step = [o for o in ops if o['kind'] == 'step' and o['render'] == 1]
    plan = dict(_first(ops, 'plan_macro'), mask=np.ones(N, np.uint8))
    camera = [o for o in ops if o['kind'] == 'set_camera'][1]           # (not the record that is the op under test)
    prefix = [step[0], dict(kind='checkpoint'), plan, camera, step[1]]
    step_plan = dict(kind='step_plan', idle=np.zeros(N, np.uint8), render=1, flags=None)
    everyone = np.arange(N)
    q_ops = _program('q70')                 # (the same handle size: the records of the three table mutators come from there)
    for kind in sp.MUTATORS + sp.Q_MUTATORS:
        op = _first(ops, kind) if kind in sp.MUTATORS else next(o for o in q_ops if o['kind'] == kind and o.get('cls') != 'default')
        got = []
        for env, with_op, mir in ((X, True, mirrors[0]), (Y, False, mirrors[1])):
            env.restore(base)
            env.set_env_appearance()
            env.set_kinematic_points([nat.EE_LINK])       # (the tables are settings: a restore keeps them; setup puts back the other two)
            s = sp.Session(env, 'device')
            s.setup()
            env.set_episode(24, sp.GOAL_STRIDE)           # (every env is past it: an auto-reset here resets them all)
            s.apply(dict(kind='select_image_mirror', sel=7))
            for p in prefix:
                s.apply(p)
            if with_op:
                s.apply(op)
            tail = {'set_object_home': [dict(kind='reset_host', mask=np.ones(N, np.uint8)), step[2]],
                    'save_snapshot': [step[2], dict(kind='load_snapshot', slot=op.get('slot'), index=None), step[3]],
                    'checkpoint': [step[2], dict(kind='checkpoint'), dict(kind='restore'), step[3]],
                    'plan_macro': [dict(step_plan, render=0)] * 100 + [step_plan]}.get(kind, [step[2]])
            for p in tail:
                s.apply(p)
            s.apply(dict(kind='episode_peek'))
            d = _collect(env, s, probe, everyone, everyone)
            env.sync()
            for bit, k in enumerate(IMAGE_FIELDS):
                d['mirror.' + k] = mir[bit].copy()
            got.append(d)
            s.release()
        # (the episode counter and the final observation outlive the set-up: X alone has the auto-reset of an earlier kind in them)
        reshaped = lambda k: not isinstance(got[0][k], list) and got[0][k].shape != got[1][k].shape      # (a table of another size)
        moved = [k for k in got[0] if (reshaped(k) or _differing(got[0][k], got[1][k]).size)
                 and (kind == 'episode_reset' or k not in ('episode.episode', 'episode.final_obs'))]
        assert moved, "%s moves none of the compared fields" % kind
        if kind in sp.IMAGE_ONLY:
            assert all(k.startswith(('image.', 'mirror.')) for k in moved), (kind, moved)
        elif kind in sp.Q_MUTATORS:             # a class of their own: query and ray outputs move, no state or image field does
            assert all(k.startswith(TABLE_FIELDS) for k in moved), (kind, moved)
            own = {'set_distance_pairs': QUERIES[:6], 'set_kinematic_points': QUERIES[6:] + ('kinematic.point_',), 'set_rays': ('ray_cast',)}[kind]
            assert any(k.startswith(own) for k in moved), (kind, moved)
        elif kind not in ('set_env_goals',):
            assert 'state' in moved or 'contacts(i)' in moved, (kind, moved)
    _state_writes_move_the_probe(X, N, nobj, probe, base)
    _command_mutators_move(X, Y, N, nobj, W, H, probe, base, step)
    for e in (X, Y):
        e.close()


CARRY_FIELDS = ('posture_clearance(po).', 'signed_distance().', 'signed_distance(po).', 'signed_distance_gradient(po).')


def _command_mutators_move(X, Y, N, nobj, W, H, probe, base, step):
    """The new kinds of the command programmes (their first records of c70), each with the invariant the header gives it.
    * set_joint_torques, set_external_wrenches: the next step's state moves in the masked envs whose row has a non-zero entry (and
      that are not frozen) and in NO other env -- the zero-row rule, -0.0 included.
    * the unmasked clearing call: the next step is, bit for bit, the step of a handle that never had the feature -- a third handle
      restored from the same checkpoint.
    * attach: the outputs of the carry queries move in envs that carry something, and nothing else moves: no state field before the
      step and none behind it.
    * macro_invalidate: nothing moves before the next step_macro, and there `replanned` is set in exactly the masked envs that are
      not idle."""
    c = _program('c70')
    Z = BatchedREALRobotEnv(N, objects=nobj, width=W, height=H)
    everyone = np.arange(N)

    def fresh(env):
        env.restore(base)                   # (a restore keeps the tables, the attachments and the macro record: settings of the handle)
        env.set_joint_torques(None)
        env.set_external_wrenches(None)
        env.detach_objects()
        env.macro_invalidate()
        env.set_kinematic_points([nat.EE_LINK])
        s = sp.Session(env, 'device')
        s.setup()
        return s

    def fields(env):
        d = {'state': env.state}
        d.update({k: env.host(f) for k, f in STATE_FIELDS.items()})
        d['contacts(i)'] = [env.contacts(int(i)) for i in everyone]
        return d
    for kind, key, clear in (('set_joint_torques', 'torques', 'clear_joint_torques'), ('set_external_wrenches', 'wrenches', 'clear_external_wrenches')):
        op = _first(c, kind, inplace=False)
        sx, sy, sz = fresh(X), fresh(Y), fresh(Z)
        sx.apply(op)
        sz.apply(op)
        sz.apply(dict(kind=clear, mask=None))
        for s in (sx, sy, sz):
            s.apply(step[2])
        fx, fy, fz = fields(X), fields(Y), fields(Z)
        rows = op[key].reshape(N, -1)[:, :11 * (1 if key == 'torques' else 6) + (0 if key == 'torques' else 6 * nobj)]
        want = np.flatnonzero((op['mask'] != 0) & (rows != 0).any(axis=1) & ((fy['errflags'] & 5) == 0))
        moved = _differing(fx['state'], fy['state'])
        assert want.size and np.array_equal(moved, want), "%s moves the next step's state in envs %s, its masked non-zero rows are %s" % (kind, moved.tolist(), want.tolist())
        for k in fx:
            bad = _differing(fx[k], fy[k])
            assert np.isin(bad, want).all(), "%s moves %s in envs %s outside its masked non-zero rows" % (kind, k, bad[~np.isin(bad, want)].tolist())
            assert _differing(fz[k], fy[k]).size == 0, "behind %s the next step's %s differs from a handle that never had the feature" % (clear, k)
        for s in (sx, sy, sz):
            s.release()
    # attach
    op = next(o for o in c if o['kind'] == 'attach' and not o.get('anchor'))
    sx, sy = fresh(X), fresh(Y)
    sx.apply(op)
    carrying = np.flatnonzero((op['mask'] != 0) & (op['links'] >= 0).any(axis=1))
    dx, dy = (_collect(e, s, probe, everyone, everyone, images=False) for e, s in ((X, sx), (Y, sy)))
    # (the episode counter and the final observation outlive a restore: X and Y have the auto-resets of earlier kinds in them)
    moved = [k for k in dx if k in dy and k not in ('episode.episode', 'episode.final_obs') and _differing(dx[k], dy[k]).size]
    assert moved and all(k.startswith(CARRY_FIELDS) for k in moved), ('attach', moved)
    assert {k[:k.index('.') + 1] for k in moved} == set(CARRY_FIELDS), ('attach', moved)
    for k in moved:
        assert np.isin(_differing(dx[k], dy[k]), carrying).all(), ('attach', k, _differing(dx[k], dy[k]).tolist(), carrying.tolist())
    for s in (sx, sy):
        s.apply(step[2])
    fx, fy = fields(X), fields(Y)
    assert all(_differing(fx[k], fy[k]).size == 0 for k in fx), "attach moves a field of the step"
    for s in (sx, sy):
        s.release()
    # macro_invalidate
    go = dict(_first(c, 'step_macro'), render=0, flags=None)
    op = next(o for o in c if o['kind'] == 'macro_invalidate' and o['mask'] is not None)
    sx, sy = fresh(X), fresh(Y)
    for s in (sx, sy):
        s.apply(go)
        s.apply(go)
    macro = lambda env: {name: env.macro_buffer(name, host=True) for name in nat.MACRO_NAMES}
    awake = go['idle'] == 0                 # (an idle env keeps the position an earlier part of this test left it)
    assert not macro(X)['replanned'].any() and (macro(X)['position'][awake] == 2).all()
    sx.apply(op)
    fx, fy, mx, my = fields(X), fields(Y), macro(X), macro(Y)
    assert all(_differing(fx[k], fy[k]).size == 0 for k in fx) and all(_differing(mx[k], my[k]).size == 0 for k in ('position', 'replanned', 'plan'))
    assert np.array_equal(np.isnan(mx['request']).all(axis=1)[awake], (op['mask'] != 0)[awake]) and not np.isnan(my['request'][awake]).any()
    for s in (sx, sy):
        s.apply(go)
    want = ((op['mask'] != 0) & (go['idle'] == 0)).astype(np.uint8)
    assert want.any() and np.array_equal(macro(X)['replanned'], want) and not macro(Y)['replanned'].any()
    assert np.array_equal(macro(X)['replanned'], sx.macro.replanned) and np.array_equal(macro(X)['position'][awake], sx.macro.position[awake])
    for s in (sx, sy):
        s.release()
    Z.close()


def _state_writes_move_the_probe(env, N, nobj, probe, base):
    """The probe's table and postures are not culled or saturated into blindness: a write_state of the object poses alone, with no
    step, moves every probe output that reads the objects -- the six hull-distance calls --, and one of the joint positions alone
    moves every one that reads the present joints: closest_points, signed_distance() and posture_ik without seeds (the candidate
    forms replace the joints by their tensors, and the IK reads no object, so neither write has to move those)."""
    env.restore(base)
    env.set_kinematic_points([nat.EE_LINK])
    s = sp.Session(env, 'device')
    s.setup()
    rows = sp._Draw(np.random.default_rng([97, N]), N, nobj).rows()
    everyone = np.arange(N)
    for parts, must in ((sp.W_OBJ_POSE, QUERIES[:6]), (sp.W_JOINT_POS, READS_JOINTS)):
        d0 = _collect(env, s, probe, everyone, everyone, images=False)
        s.apply(dict(kind='write_state', parts=parts, reset=False, fresh=False, rows=rows, mask=None))
        d1 = _collect(env, s, probe, everyone, everyone, images=False)
        moved = [k for k in d0 if _differing(d0[k], d1[k]).size]
        for call in must:
            assert any(k.startswith(call + '.') for k in moved), (parts, call, moved)
        assert not any(k.startswith(('posture_kinematics(po).', 'posture_ik(targets, seeds).')) for k in moved), (parts, moved)
        s.release()
