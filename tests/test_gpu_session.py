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
between comparisons; and, for every mutator kind, the proof that the compared fields move when the call is made."""
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
        _cache[name] = sp.program(seed, N, nobj, length)
    return _cache[name]


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
    for k, v in env.ray_cast(probe.segments if sess.road == 'host' else probe.segments_dev, host=True).items():
        d['ray_cast(rays).' + k] = v
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
        self.N, self.ops = N, _program(name)
        self.A = BatchedREALRobotEnv(N, objects=nobj, width=W, height=H)
        self.B = _make(monkeypatch, PLAIN, N, objects=nobj, width=W, height=H) if twin else None
        self.envs = [e for e in (self.A, self.B) if e is not None]
        _warm_up(self.envs, N)
        self.sa = sp.Session(self.A, road_a)
        self.sb = sp.Session(self.B, 'host') if twin else None
        for s in (self.sa, self.sb):
            if s is not None:
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


def _run_twin(tw, counts=None):
    """the programme on A and B with a comparison behind every op; returns the number of comparisons"""
    ops, compared = tw.ops, 0
    before = tw.collect_a()
    _assert_equal(before, tw.collect_b(True), 0, ops, "before the programme, A against B", tw.envs_of)
    for i, op in enumerate(ops):
        tw.sa.apply(op)
        tw.sb.apply(op)
        if op['kind'] in sp.OBSERVERS and op['kind'] != 'episode_peek':
            continue                        # B made no call: the next comparison shows whether A's changed anything
        a = tw.collect_a()
        stepped = sp.is_step(op)
        _assert_equal(a, tw.collect_b(stepped), i, ops, "A against B", tw.envs_of)
        if not stepped:
            _assert_equal(a, before, i, ops, "A's images against A's own of before the call", tw.envs_of, skip=[k for k in a if not k.startswith('image.')])
        _check_mirrors(tw.A, tw.sa, tw.mirror, tw.img_mirror, a, tw.img_envs, i, ops)
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
    print("session n70: coverage %s; %d compared ops; %.1f s" % (counts, n, time.perf_counter() - t0))
    assert counts['heavy'] > 0 and counts['auto_resets'] > 0 and counts['refused'] > 0 and counts['partial_auto_resets'] > 0, counts


def _run_alone(monkeypatch, road):
    """the 70-env programme on a fresh default handle alone, with the reads of a comparison behind every compared op: its digests"""
    tw = _Twin(monkeypatch, 'n70', road_a=road, twin=False)
    digests = []
    for i, op in enumerate(tw.ops):
        tw.sa.apply(op)
        if op['kind'] in sp.OBSERVERS and op['kind'] != 'episode_peek':
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
    print("session n70, the second run: %d digests; %.1f s" % (len(again), time.perf_counter() - t0))


def test_n5_one_chain_placement_one_object_wide_image(monkeypatch):
    """5 envs, 1 object, 96 x 64, 200 ops: the one-chain placement, P.nobj < 3 (state = s on both roads: the device form is bitwise
    rr_set_state on three objects only), an image that is not square."""
    t0 = time.perf_counter()
    tw = _Twin(monkeypatch, 'n5')
    n = _run_twin(tw)
    tw.close()
    print("session n5: %d compared ops; %.1f s" % (n, time.perf_counter() - t0))


def test_n1100_packed_solve(monkeypatch):
    """1100 envs, 3 objects, 32 x 32, 200 ops: above COOP_ALL_MAX -- the packed solve and the side-by-side step without camera.
    Images and contacts(i) of 16 envs (both ends, around the groups of 64 and 512); everything else of all envs."""
    t0 = time.perf_counter()
    tw = _Twin(monkeypatch, 'n1100')
    n = _run_twin(tw)
    tw.close()
    print("session n1100: %d compared ops; %.1f s" % (n, time.perf_counter() - t0))


class _NullEnv:
    """takes every call and does nothing: a dry run of a Session shows which device arguments a programme needs, in order"""

    def __init__(self, env):
        self.N, self.n_objects, self.W, self.H = env.N, env.n_objects, env.W, env.H

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        return lambda *a, **kw: None


class _NoMemory:
    def data_ptr(self):
        return 0


def test_n70_free_running_between_comparisons(monkeypatch):
    """The comparisons above wait for the device behind every op, and B's host road waits inside its calls.  Here A runs the same
    70-env programme as a training loop would: every device argument is uploaded before the first op, and A makes the ops of a chunk
    -- up to the eighth compared op -- back to back before B makes its own, so A's calls on the library's stream follow each other
    with no wait but the library's own (a device-road write, fork, reset, observer or episode update is enqueued while the side
    streams still work on the step before).  A call that relied on a wait would differ from B at the end of the chunk."""
    t0 = time.perf_counter()
    tw = _Twin(monkeypatch, 'n70')
    staged = []
    dry = sp.Session(_NullEnv(tw.A), 'device', to_device=lambda a: staged.append(np.array(a)) or _NoMemory())
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
        compared += not (op['kind'] in sp.OBSERVERS and op['kind'] != 'episode_peek')
        if compared - flushed >= 8 or i == len(tw.ops) - 1:
            flushed = compared
            for o in chunk:
                tw.sa.apply(o)
            for o in chunk:
                tw.sb.apply(o)
            chunk = []
            a = tw.collect_a()
            _assert_equal(a, tw.collect_b(True), i, tw.ops, "A (free running) against B", tw.envs_of)
            _check_mirrors(tw.A, tw.sa, tw.mirror, tw.img_mirror, a, tw.img_envs, i, tw.ops)
    assert not staged
    tw.close()
    print("session n70, free running: %d compared ops, a comparison behind every eighth; %.1f s" % (compared, time.perf_counter() - t0))


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
    select_image_mirror moves A's mapped image mirror: the deselected block keeps the old frame."""
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
    for kind in sp.MUTATORS:
        op = _first(ops, kind)
        got = []
        for env, with_op, mir in ((X, True, mirrors[0]), (Y, False, mirrors[1])):
            env.restore(base)
            env.set_env_appearance()
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
        moved = [k for k in got[0] if _differing(got[0][k], got[1][k]).size
                 and (kind == 'episode_reset' or k not in ('episode.episode', 'episode.final_obs'))]
        assert moved, "%s moves none of the compared fields" % kind
        if kind in sp.IMAGE_ONLY:
            assert all(k.startswith(('image.', 'mirror.')) for k in moved), (kind, moved)
        elif kind not in ('set_env_goals',):
            assert 'state' in moved or 'contacts(i)' in moved, (kind, moved)
    for e in (X, Y):
        e.close()
