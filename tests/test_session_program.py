"""CPU tests of the programmes that tests/test_gpu_session.py runs (tests/session_program.py): the coverage of the interleaving
does not depend on luck.  For the very seeds and sizes of the GPU test (session_program.SESSIONS), n70, n5 and n1100 -- whose
programmes are pinned by a digest taken from the generator as it was before the query programmes existed --:

* the same arguments give the same programme, another seed another one;
* every mutator kind at least 3 times, each directly followed at least once by a step without camera, with the camera of every env
  and with per-env flags; every observer kind at least once directly between a step and a mutator and at least once directly
  between a mutator and a step;
* write_state with each of the 16 subsets of its column groups (the empty one: reset or fresh alone), all four combinations of reset
  and fresh, and the three forms the header names bitwise equal to rr_set_object_poses, the auto-reset's pair and rr_set_state; over
  the three programmes every subset meets three of the four combinations;
* a set_object_home whose object a write has thrown out of bounds one step before: the one place where the look-ahead has used the
  home pose;
* restore and load_snapshot each after a fork and after a device reset; a restore always has a checkpoint before last; a step_plan
  has a plan; no mask, flag set or idle set is all-clear; refused steps, render(), step_plan and both command roads occur.

23 mutator kinds, three times each, directly followed by a step, are 138 ops: a programme has 200, whatever the number of envs.

The query programmes of q70 and q5 (3 more mutator kinds, 9 query observer kinds; 74 ops): the conditions of
`check_query_conditions`, spelled out at test_conditions_of_the_query_programmes_the_gpu_test_runs; a negative case for each kind of
condition; and, for the very anchor records of the GPU test, that the float64 reference decides at least 95 % of the items, so that
the anchor cannot silently compare nothing.

A recording fake of BatchedREALRobotEnv shows which calls each road issues, for the query kinds too.

The command programmes of c70 and c5 (10 more mutator kinds, the step kind step_macro, 10 observer kinds; 212 ops; q70 and q5 are
pinned by digest from before they existed): the conditions of `check_command_conditions` for the very programmes the GPU test runs,
a negative case for each kind of condition, the calls of both roads on the fake, the numpy model of the macro decision rule on a
hand-made case, and that the float64 reference decides EVERY item of the two anchors."""
import numpy as np
import pytest

from tests import session_program as sp


OLD = [name for name in sp.SESSIONS if name not in sp.QUERY_SESSIONS + sp.COMMAND_SESSIONS]
assert OLD == ['n70', 'n5', 'n1100']
# the three programmes from before the query programmes, as the parent commit's `program` drew them: blake2b-128 over every record's
# kind and its keys in sorted order -- arrays (and the arrays of a recipe) by dtype, shape and bytes, everything else by its repr
PINNED = {'n70': '0814dd1c46894a9a7d1660a2d276ee18', 'n5': '0fc90cd75a5fb425940149d1ff46cee7', 'n1100': '3c819adaf090f39665680cb5ccced3c7'}
# ... and the two query programmes as the parent commit's `program` drew them, taken before the command programmes existed
PINNED_QUERIES = {'q70': 'e07b2a5d05f54e7ed94080040d72e45c', 'q5': '34625be5378176b4b8806694589cd2fd'}


@pytest.fixture(scope='module')
def programmes():
    return {name: sp.program(seed, N, nobj, length, queries=name in sp.QUERY_SESSIONS, commands=name in sp.COMMAND_SESSIONS)
            for name, (seed, N, nobj, _, _, length) in sp.SESSIONS.items()}


def _digest(ops):
    import hashlib
    h = hashlib.blake2b(digest_size=16)
    for o in ops:
        h.update(o['kind'].encode())
        for k in sorted(o):
            v = o[k]
            if isinstance(v, dict):
                for kk in sorted(v):
                    a = np.asarray(v[kk])
                    h.update(('%s.%s%s%s' % (k, kk, a.dtype.str, a.shape)).encode() + np.ascontiguousarray(a).tobytes())
            elif isinstance(v, np.ndarray):
                h.update(('%s%s%s' % (k, v.dtype.str, v.shape)).encode() + np.ascontiguousarray(v).tobytes())
            else:
                h.update(('%s=%r' % (k, v)).encode())
    return h.hexdigest()


@pytest.mark.parametrize('name', OLD)
def test_the_programmes_from_before_the_queries_are_unchanged(programmes, name):
    assert _digest(programmes[name]) == PINNED[name]


@pytest.mark.parametrize('name', sp.QUERY_SESSIONS)
def test_the_query_programmes_are_unchanged(programmes, name):
    assert _digest(programmes[name]) == PINNED_QUERIES[name]


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    return type(a) is type(b) and a == b


@pytest.mark.parametrize('name', OLD)
def test_the_same_arguments_give_the_same_programme(programmes, name):
    seed, N, nobj, _, _, length = sp.SESSIONS[name]
    again = sp.program(seed, N, nobj, length)
    assert len(again) == length and all(_same(a, b) for a, b in zip(programmes[name], again))
    other = sp.program(seed + 1, N, nobj, length)
    assert not all(_same(a, b) for a, b in zip(programmes[name], other))


def test_the_module_imports_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys; from tests import session_program as sp; sp.program(1, 5, 1, 200); "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('torch', 'real_robots_amd')], sys.modules.keys()")
    subprocess.check_call([sys.executable, '-c', code], cwd=str(__import__('pathlib').Path(__file__).resolve().parents[1]))


@pytest.mark.parametrize('name', OLD)
def test_conditions_of_the_programmes_the_gpu_test_runs(programmes, name):
    length = sp.SESSIONS[name][5]
    assert length == 200
    sp.check_conditions(programmes[name], length)
    with pytest.raises(ValueError):
        sp.program(1, 5, 1, 120)            # (too short for the conditions: refused, not thinned)


def test_every_subset_meets_reset_and_fresh_with_and_without(programmes):
    seen = {}
    for ops in programmes.values():
        for o in ops:
            if o['kind'] == 'write_state':
                seen.setdefault(o['parts'], set()).add((o['reset'], o['fresh']))
    assert set(seen) == set(range(16))
    for parts, combos in seen.items():
        assert len(combos) >= (3 if parts else 2), (parts, combos)         # (no columns, no reset, no fresh is no call)
        assert {c[0] for c in combos} == {False, True} and {c[1] for c in combos} == {False, True}, (parts, combos)


@pytest.mark.parametrize('name', OLD)
def test_the_conditions_spelled_out(programmes, name):
    """the conditions once more, from the list of kinds alone (not through check_conditions)"""
    ops = programmes[name]
    kinds = [o['kind'] for o in ops]
    assert len(set(sp.MUTATORS)) == 23 and len(set(sp.OBSERVERS)) == 11
    for m in sp.MUTATORS:
        at = [i for i, k in enumerate(kinds) if k == m]
        assert len(at) >= 3, m
        forms = {ops[i + 1]['render'] for i in at if i + 1 < len(ops) and kinds[i + 1] == 'step'}
        assert forms == {0, 1, 2}, (m, forms)
    steps = set(sp.STEP_KINDS)
    for o in sp.OBSERVERS:
        at = [i for i, k in enumerate(kinds) if k == o and 0 < i < len(kinds) - 1]
        assert any(kinds[i - 1] in steps and kinds[i + 1] in sp.MUTATORS for i in at), o
        assert any(kinds[i - 1] in sp.MUTATORS and kinds[i + 1] in steps for i in at), o
    for m in ('restore', 'load_snapshot'):
        assert any(kinds[i] == m and any(k.startswith('fork') for k in kinds[:i]) and 'reset_dev' in kinds[:i] for i in range(len(kinds))), m
    assert kinds.count('step_plan') >= 2 and kinds.count('step_refused') >= 2 and kinds.count('render') >= 2
    flags = [o['flags'] for o in ops if o.get('render') == 2]
    assert flags and all(f.any() and not f.all() for f in flags)


def test_a_condition_that_fails_is_noticed(programmes):
    ops = [o for o in programmes['n70'] if o['kind'] != 'sync']
    ops += [dict(kind='render')] * (200 - len(ops))
    with pytest.raises(AssertionError):
        sp.check_conditions(ops, 200)
    ops = [dict(o, parts=3) if o['kind'] == 'write_state' and o['parts'] == 12 else o for o in programmes['n5']]
    with pytest.raises(AssertionError):
        sp.check_conditions(ops, 200)       # (no write throws an object out of bounds in front of a set_object_home)
    # the query programmes: each of these breaks one condition and nothing else
    _, _, nobj, _, _, length = sp.SESSIONS['q70']
    q = programmes['q70']
    sp.check_query_conditions(q, length, nobj)
    at = next(i for i, o in enumerate(q) if o['kind'] == 'fork_dev')
    assert q[at + 1]['kind'] in sp.STATE_READERS
    broken = [
        [dict(o, compared=True) if o['kind'] == 'swept_clearance' else o for o in q],                 # a kind that is never silent
        q[:at + 1] + [dict(q[at + 1], kind='posture_kinematics')] + q[at + 2:],                      # no state reader behind the fork
        [dict(o, cls='one') if o['kind'] == 'set_distance_pairs' and o['cls'] == 'full' else o for o in q],      # no table of 96 pairs
        [dict(o, max_distance=0.1) if o['kind'] == 'set_distance_pairs' and o['cls'] == 'default' else o for o in q],   # a cull at the anchors
        [dict(o, links=np.full_like(o['links'], 8)) if o['kind'] == 'set_kinematic_points' else o for o in q],   # the gripper base only
        [o for o in q if o['kind'] != 'set_rays' or len(o['links']) != 64] + [dict(kind='render')],   # no table of 64 rays
    ]
    broken[-1] += [dict(kind='render')] * (length - len(broken[-1]))
    for ops in broken:
        assert len(ops) == length
        with pytest.raises(AssertionError):
            sp.check_query_conditions(ops, length, nobj)


# ---------------------------------------------------------------------------------------------------- the query programmes
@pytest.mark.parametrize('name', sp.QUERY_SESSIONS)
def test_conditions_of_the_query_programmes_the_gpu_test_runs(programmes, name):
    """q70 and q5: the three table mutators with every render form; each of the nine query observers directly between a step and a
    mutator and directly between a mutator -- not a write_state every time -- and a step, compared and silent; a state-reading query
    directly behind each of write_state (poses, joints), fork_dev, load_snapshot, reset_dev, restore, set_object_poses, episode_reset,
    set_distance_pairs and set_kinematic_points; K in {1, 3, 32}; tables of 1, the default, 92 / 80 ('collision') and 96 pairs with
    and without a cull; points on a finger link and below joint 7 with offsets; 1, 4 and 64 world and link rays; the two anchors with
    the default table in force."""
    seed, N, nobj, _, _, length = sp.SESSIONS[name]
    ops = programmes[name]
    assert length == sp.Q_LENGTH
    sp.check_query_conditions(ops, length, nobj)
    again = sp.program(seed, N, nobj, length, queries=True)
    assert all(_same(a, b) for a, b in zip(ops, again))
    assert not all(_same(a, b) for a, b in zip(ops, sp.program(seed + 1, N, nobj, length, queries=True)))
    with pytest.raises(ValueError):
        sp.program(seed, N, nobj, length - 1, queries=True)       # (too short for the conditions: refused, not thinned)
    longer = sp.program(seed, N, nobj, length + 5, queries=True)
    sp.check_query_conditions(longer, length + 5, nobj)
    kinds = [o['kind'] for o in ops]
    for k in sp.Q_OBSERVERS:                                       # once more, from the list of kinds alone
        at = [i for i, x in enumerate(kinds) if x == k]
        assert any(kinds[i - 1] == 'step' and kinds[i + 1] in sp.MUTATORS + sp.Q_MUTATORS for i in at), k
        assert any(kinds[i - 1] in sp.MUTATORS + sp.Q_MUTATORS and kinds[i - 1] != 'write_state' and kinds[i + 1] == 'step' for i in at), k


def test_the_shape_and_link_names_are_the_models():
    from real_robots_amd import _native as nat
    from real_robots_amd.batched import BatchedREALRobotEnv
    rows = BatchedREALRobotEnv.collision_shapes()
    by_body = lambda ok: tuple(r['name'] for r in rows if ok(r['body']))
    assert sp.STATIC_SHAPES == by_body(lambda b: b < 0) and sp.ROBOT_SHAPES == by_body(lambda b: 0 <= b < 16) and sp.OBJECT_SHAPES == by_body(lambda b: b >= 16)
    assert len(nat.LINK_NAMES) == sp.N_LINKS and all(nat.LINK_NAMES[l].startswith(('finger', 'skin')) for l in sp.FINGER_LINKS)
    assert [nat.LINK_NAMES[l] for l in sp.ARM_LINKS] == ['lbr_iiwa_link_%d' % l for l in range(1, 7)]
    for nobj in (1, 2, 3):
        pairs = sp.default_pairs(nobj)
        n, a, b, md = BatchedREALRobotEnv._distance_arg(pairs, None, nobj)           # (only objects the handle has)
        assert 10 <= n == len(pairs) <= 14 and md == 0.0
        kind = lambda x: 'o' if x in sp.OBJECT_SHAPES else 's' if x in sp.STATIC_SHAPES else 'r'
        mixes = {''.join(sorted(kind(x) + kind(y))) for x, y in pairs}
        assert mixes >= {'or', 'rs', 'rr', 'os'} and (('oo' in mixes) == (nobj > 1))


@pytest.mark.parametrize('name', sp.QUERY_SESSIONS)
def test_the_anchors_are_decided(programmes, name):
    """The float64 anchor of the GPU test may omit only what the reference leaves undecided: for the very anchor records of q70 and
    q5, the first four envs, the default table and the probe's postures, at least 95 % of the (env, pair) and (env, posture, pair)
    items are decided, none overlaps, and the nearest pair of nearly every row is decided too."""
    from tests import numpy_posture as npo
    _, N, nobj, _, _, _ = sp.SESSIONS[name]
    anchors = [o for o in programmes[name] if sp.is_anchor(o)]
    assert {o['kind'] for o in anchors} == {'set_state', 'write_state'}
    q = sp.probe_arguments(N, nobj)
    assert q['postures'].shape == (N, sp.PROBE_K, 11) and q['segments'].shape == (N, 2, 2, 11) and q['targets'].shape == (N, 2, 7)
    for o in anchors:
        st, pairs, ref, ref_po = sp.anchor_references(o, nobj, q)
        n = min(N, sp.ANCHOR_ENVS)
        assert ref['decided'].shape == (n, len(pairs)) and ref_po['decided'].shape == (n * sp.PROBE_K, len(pairs))
        for r in (ref, ref_po):
            assert r['decided'].sum() >= 0.95 * r['decided'].size and (r['d'] > 0).all(), (o['kind'], r['decided'].sum(), r['d'].min())
        assert npo.nearest(ref_po)[1].sum() >= 0.75 * n * sp.PROBE_K
        assert ref['d'].min() < sp.PROBE_MARGIN                    # (the probe's gradient has a cost to report)


def test_written_values_are_what_the_calls_get():
    rows = sp._Draw(np.random.default_rng(1), 6, 3).rows()
    s = sp.compose_state(rows, 1)
    assert s.shape == (6, 61) and s.dtype == np.float32 and not s[:, 35:].any() and np.isfinite(s).all()
    assert np.allclose(np.linalg.norm(s[:, 25:29], axis=1), 1.0, atol=1e-6)
    assert sp.part_columns(15, 3).size == 61 and sp.part_columns(4, 1).tolist() == list(range(22, 29))
    assert sp.part_columns(1 | 8, 2).tolist() == list(range(11)) + list(range(29, 35)) + list(range(42, 48))
    start, final, flags, rgb = sp.goal_table(1, 8, 4)
    assert start.shape == (5, 1, 7) and np.isnan(start[(flags & 2) == 0]).all() and np.isfinite(start[(flags & 2) != 0]).all()
    assert np.isfinite(final[(flags & 1) != 0]).all() and rgb.shape == (5, 4, 8, 3)


# ---------------------------------------------------------------------------------------------------- the roads, on a fake
class _Dev:
    """device memory of the fake"""

    def __init__(self, a):
        self.a = a

    def data_ptr(self):
        return id(self)


class _Lib:
    def __init__(self, log):
        self.log = log

    def rr_step(self, h, ptr, on_device, mode, flags):
        self.log.append(('rr_step', 'device' if on_device else 'host', mode))
        return 0


class FakeEnv:
    """records (call, where its array arguments live)"""

    def __init__(self, N, nobj, W=8, H=4):
        self.N, self.n_objects, self.W, self.H, self.h = N, nobj, W, H, None
        self.log = []
        self.L = _Lib(self.log)

    @staticmethod
    def _side(args, kw):
        vals = [v for v in list(args) + list(kw.values()) if isinstance(v, (np.ndarray, _Dev))]
        sides = {'device' if isinstance(v, _Dev) else 'host' for v in vals}
        assert len(sides) <= 1, "arguments on both sides"
        return sides.pop() if sides else None

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)

        def call(*args, **kw):
            side = self._side(args, {'idle': kw.get('idle')} if name == 'step_macro_device' else kw)      # (render flags are host memory on every road)
            if name == 'step':
                side = 'device' if kw.get('device_ptr') is not None else 'host'
            flags = tuple(k for k in ('joint_pos', 'joint_vel', 'obj_pose', 'obj_vel', 'reset', 'fresh') if kw.get(k))
            self.log.append((name, side) + ((flags,) if name == 'write_state' else ()))
            if name == 'checkpoint':
                return np.zeros(4, np.uint8)
            if name == 'posture_dynamics':      # (the bias is what torques_from_dynamics passes on: a device view, or a host array)
                return {'bias': np.zeros((self.N, 1, 11), np.float32) if kw.get('host') else _Dev(None)}
            if name == 'episode_buffer':
                return (np.arange(self.N) % 2).astype(np.uint32) if args[0] == 'done' else np.zeros(self.N, np.float32)
            if name == 'host':
                from real_robots_amd import _native as nat
                shape = {nat.F_JOINTS: (self.N, 9), nat.F_TOUCH: (self.N, 4), nat.F_OBJ_POSE: (self.N, self.n_objects, 7)}[args[0]]
                return np.zeros(shape, np.float32)
            return None
        return call

    @property
    def state(self):
        raise AssertionError("the programme does not read the state")

    @state.setter
    def state(self, s):
        assert isinstance(s, np.ndarray) and s.shape == (self.N, 61)
        self.log.append(('state=', 'host'))


def _run(ops, road, N, nobj):
    env = FakeEnv(N, nobj)
    s = sp.Session(env, road, to_device=_Dev)
    s.copy_in_place = lambda e, name, table, mask: e.log.append(('in_place ' + name, e._side((table, mask), {})))
    s.setup()
    env.log.clear()
    per_op = []
    for op in ops:
        n = len(env.log)
        s.apply(op)
        per_op.append(env.log[n:])
    return per_op, s


@pytest.mark.parametrize('name', OLD)
def test_both_roads_issue_the_calls_they_should(programmes, name):
    _, N, nobj, _, _, _ = sp.SESSIONS[name]
    ops = programmes[name]
    dev, _ = _run(ops, 'device', N, nobj)
    host, hs = _run(ops, 'host', N, nobj)
    wr, _ = _run(ops, 'written', N, nobj)
    for op, d, h, w in zip(ops, dev, host, wr):
        k = op['kind']
        names_d, names_h = [c[0] for c in d], [c[0] for c in h]
        assert all(c[1] != 'device' for c in h), (k, h)              # the twin never passes device memory
        if k in ('step', 'step_refused'):
            assert d == [('step', 'device')]
            assert h == ([('step', 'host')] if k == 'step' else [('rr_step', 'host', op['render'])])
            assert w[0][1] == ('device' if op['device'] else 'host')
        elif k in ('reset_host', 'reset_dev'):
            assert d == [('reset', 'device')] and h == [('reset', 'host')]
            assert w == [('reset', 'device' if op['device'] else 'host')]
        elif k in ('fork_host', 'fork_dev'):
            assert d == [('fork', 'device')] and h == [('fork', 'host')] and w == [('fork', 'device' if op['device'] else 'host')]
        elif k == 'set_state':
            assert h == [('state=', 'host')]
            assert d == ([('write_state', 'device', ('joint_pos', 'joint_vel', 'obj_pose', 'obj_vel', 'fresh'))] if nobj == 3 else h)
        elif k == 'write_state':
            assert names_d == ['write_state'] and d[0][1] == 'device'
            assert bool(op['reset']) == ('reset' in d[0][2]) and bool(op['fresh']) == ('fresh' in d[0][2])
            if op['parts'] == 0 and not op['fresh']:
                assert h == [('reset', None if op['mask'] is None else 'host')]
            elif op['parts'] == 4 and not op['fresh']:
                assert names_h == (['reset'] if op['reset'] else []) + ['set_object_poses']
            elif op['parts'] == 15 and op['fresh'] and not op['reset'] and op['mask'] is None and nobj == 3:
                assert names_h == ['state=']
            else:
                assert h == [('write_state', 'host', d[0][2])]
        elif k == 'episode_reset':
            assert names_d == ['episode_update']
            assert names_h[:2] == ['episode_update', 'episode_buffer'] and names_h[-3:] == ['host', 'set_object_poses', 'set_env_goals']
            assert 'reset' in names_h
        elif k == 'episode_peek':
            assert names_d == names_h == ['episode_update']
        elif k in sp.OBSERVERS:
            assert len(d) == 1 and h == [], (k, d, h)                # the twin observes at the comparisons only
        elif k in ('load_snapshot', 'save_snapshot'):
            assert names_d == names_h == [k] and d[0][1] == (None if op['index'] is None else 'device')
        else:
            assert names_d == names_h and len(names_d) == 1, (k, d, h)
    assert hs.episode.tolist() == ((np.arange(N) % 2) * sum(o['kind'] == 'episode_reset' for o in ops)).tolist()
    wrote = [op for op in ops if op['kind'] == 'write_state']
    # (the matching host calls are really exercised, at every size)
    assert any(o['parts'] == 4 and not o['fresh'] and not o['reset'] for o in wrote) and any(o['parts'] == 4 and o['reset'] for o in wrote)
    assert any(o['parts'] == 15 and o['fresh'] and not o['reset'] and o['mask'] is None for o in wrote)
    assert any(o['parts'] == 0 for o in wrote)


@pytest.mark.parametrize('name', sp.QUERY_SESSIONS)
def test_both_roads_issue_the_query_calls_they_should(programmes, name):
    """The table mutators are host calls on every road.  A query record: A calls with device tensors; B calls only where the record
    is compared, with host arrays; a call without a tensor has no side.  The IK's point is the last of the table in force."""
    _, N, nobj, _, _, _ = sp.SESSIONS[name]
    ops = programmes[name]
    dev, sd = _run(ops, 'device', N, nobj)
    host, sh = _run(ops, 'host', N, nobj)
    call = {'closest_points': 'closest_points', 'posture_clearance': 'posture_clearance', 'signed_distance': 'signed_distance',
            'signed_distance_at': 'signed_distance', 'signed_distance_gradient': 'signed_distance_gradient', 'swept_clearance': 'swept_clearance',
            'posture_kinematics': 'posture_kinematics', 'posture_ik': 'posture_ik', 'posture_ik_present': 'posture_ik'}
    for op, d, h in zip(ops, dev, host):
        k = op['kind']
        assert all(c[1] != 'device' for c in h), (k, h)
        if k in sp.Q_MUTATORS:
            assert [c[0] for c in d] == [c[0] for c in h] == [k] and d[0][1] == h[0][1] != 'device'
        elif k in sp.Q_OBSERVERS:
            side = None if k in ('closest_points', 'signed_distance') else 'device'
            assert d == [(call[k], side)], (k, d)
            assert h == ([(call[k], side and 'host')] if op['compared'] else []), (k, h)
    assert sd.n_rays == sh.n_rays == len([o for o in ops if o['kind'] == 'set_rays'][-1]['links'])
    assert (sd.points[0] == [o for o in ops if o['kind'] == 'set_kinematic_points'][-1]['links']).all()
    assert sd.max_distance == sh.max_distance == [o for o in ops if o['kind'] == 'set_distance_pairs'][-1]['max_distance']
    # the recipe of an IK record resolves to unit quaternions at the point in force, the same on both roads
    goals = next(o for o in ops if o['kind'] == 'posture_ik')['goals']
    t = sd.ik_targets(goals)
    assert t.shape == goals.shape[:2] + (7,) and t.dtype == np.float32 and np.allclose(np.linalg.norm(t[..., 3:], axis=-1), 1.0, atol=1e-6)
    assert np.array_equal(t, sh.ik_targets(goals))
    assert sd.margin(0.3) == (0.3 if sd.max_distance is None else sd.max_distance) and sp.Session(FakeEnv(N, nobj), 'host').margin(0.3) == 0.3


def test_run_is_the_session_over_the_whole_programme(programmes):
    _, N, nobj, _, _, _ = sp.SESSIONS['n5']
    env = FakeEnv(N, nobj)
    s = sp.run(env, programmes['n5'], 'written', to_device=_Dev)
    per_op, _ = _run(programmes['n5'], 'written', N, nobj)
    calls = [c for c in env.log]
    assert calls[-sum(len(p) for p in per_op):] == [c for p in per_op for c in p]
    assert [c[0] for c in calls[:6]] == ['set_rays', 'snapshot_slots', 'set_goals', 'set_env_goals', 'set_episode', 'checkpoint']
    assert len(s.ckpts) == 1 + sum(o['kind'] == 'checkpoint' for o in programmes['n5']) and len(s.keep) > 0


# ---------------------------------------------------------------------------------------------------- the command programmes
@pytest.mark.parametrize('name', sp.COMMAND_SESSIONS)
def test_conditions_of_the_command_programmes_the_gpu_test_runs(programmes, name):
    """c70 and c5: the conditions of `check_command_conditions` for the very programmes the GPU test runs -- every new mutator
    directly followed by a step of each render form and by a step_macro; each of the eight state mutators directly followed by a step
    with both tables non-zero, with attachments on, directly behind a step_macro with plans in flight, with a step_macro behind it, and
    once more with every feature off; a carry query and an attach_capture directly behind five of them and behind a step; carried_sweep
    with attachments on and off; snapshots while everything is set and loads after it has changed; the draws.  The same arguments
    give the same programme, another seed another one; a shorter programme is refused, a longer one holds the conditions too."""
    seed, N, nobj, _, _, length = sp.SESSIONS[name]
    ops = programmes[name]
    assert length == sp.C_LENGTH == sp.C_MIN_LENGTH
    found = sp.check_command_conditions(ops, length, N, nobj)
    assert all(found['count'].get(k, 0) >= 4 for k in sp.C_MUTATORS) and found['count']['step_macro'] >= 20
    again = sp.program(seed, N, nobj, length, commands=True)
    assert all(_same(a, b) for a, b in zip(ops, again))
    assert not all(_same(a, b) for a, b in zip(ops, sp.program(seed + 1, N, nobj, length, commands=True)))
    with pytest.raises(ValueError):
        sp.program(seed, N, nobj, length - 1, commands=True)
    sp.check_command_conditions(sp.program(seed, N, nobj, length + 5, commands=True), length + 5, N, nobj)
    # once more, from the list of kinds alone
    kinds = [o['kind'] for o in ops]
    for m in sp.C_MUTATORS:
        at = [i for i, k in enumerate(kinds) if k == m]
        skip = lambda i: i + 2 if m == 'attach_capture' and kinds[i + 1] in sp.CARRY_QUERIES else i + 1
        assert {ops[skip(i)]['render'] for i in at if kinds[skip(i)] == 'step'} == {0, 1, 2}, m
        assert any(kinds[skip(i)] == 'step_macro' for i in at), m
    assert all(kinds[i + 1] in sp.CARRY_QUERIES for i, k in enumerate(kinds) if k == 'attach_capture')
    for s in ('fork_dev', 'load_snapshot', 'reset_dev', 'restore'):
        assert any(kinds[i + 1] == 'attach_capture' for i, k in enumerate(kinds) if k == s), s
        assert any(kinds[i + 1] in sp.CARRY_QUERIES for i, k in enumerate(kinds) if k == s), s
        assert any(kinds[i + 1] == 'step_macro' for i, k in enumerate(kinds) if k == s) and any(kinds[i - 1] == 'step_macro' for i, k in enumerate(kinds) if k == s), s


def test_a_broken_command_condition_is_noticed(programmes):
    """each of these breaks one condition of a command programme and nothing else"""
    _, N, nobj, _, _, length = sp.SESSIONS['c70']
    c = programmes['c70']
    kinds = [o['kind'] for o in c]
    fork = next(i for i, k in enumerate(kinds) if k == 'fork_dev' and kinds[i + 1] == 'attach_capture')
    off = max(i for i, k in enumerate(kinds) if k == 'detach_all')
    broken = [
        [dict(o, render=0, flags=None) if o['kind'] == 'step' and c[i - 1]['kind'] == 'detach' else o for i, o in enumerate(c)],       # detach meets one render form only
        c[:fork] + [dict(kind='checkpoint')] + c[fork + 1:],                                            # no attach_capture directly behind a fork
        [dict(o, compared=True) if o['kind'] == 'carried_sweep' else o for o in c],                     # a kind that is never silent
        [dict(o, mask=np.ones(N, np.uint8)) if o['kind'] == 'clear_joint_torques' else o for o in c],   # the torque feature never goes off
        c[:off] + [dict(c[off], kind='detach', mask=np.ones(N, np.uint8))] + c[off + 1:],               # no feature-off road: the attachments stay on
        [dict(o, macro=np.abs(o['macro'])) if o['kind'] == 'step_macro' else o for o in c],             # no request with a -0.0
        [dict(o, inplace=False) if o['kind'] == 'set_external_wrenches' else o for o in c],             # no in-place write of the wrench table
        [o for o in c if not o.get('anchor') or o['kind'] != 'attach'] + [dict(kind='render')] * 2,     # an anchor without its attach
    ]
    for ops in broken:
        assert len(ops) == length
        with pytest.raises(AssertionError):
            sp.check_command_conditions(ops, length, N, nobj)


def test_the_macro_model_is_the_rule_of_the_header():
    """idle: nothing moves; need = a request that differs from the record (IEEE ==) or an exhausted plan; a needing env stores the
    request and starts at row 0; every env that is not idle advances"""
    m = sp.MacroModel(4)
    req = np.array([[0.0, 0.1, 0.2, 0.3]] * 4, np.float32)
    assert m.step_macro(req, np.array([0, 0, 0, 1], np.uint8)).tolist() == [True, True, True, False]      # (the record starts NaN)
    assert m.position.tolist() == [1, 1, 1, 0] and np.isnan(m.record[3]).all() and m.replanned.tolist() == [1, 1, 1, 0]
    req[0, 0], req[1, 2], req[2, 3] = -0.0, np.nan, 0.31
    assert m.step_macro(req, None).tolist() == [False, True, True, True]                                  # (-0.0 equals 0.0; a NaN equals nothing)
    assert m.position.tolist() == [2, 1, 1, 1] and not np.signbit(m.record[0, 0]) and np.isnan(m.record[1, 2])
    assert m.step_macro(req, None).tolist() == [False, True, False, False]                                # (... on every step)
    m.position[2] = sp.PLAN_LEN
    m.invalidate(np.array([0, 0, 0, 1], np.uint8))
    m.plan(np.array([1, 0, 0, 0], np.uint8))
    assert m.position.tolist() == [0, 1, sp.PLAN_LEN, 2] and np.isnan(m.record[3]).all()
    assert m.step_macro(req, None).tolist() == [False, True, True, True] and m.position.tolist() == [1, 1, 1, 1]
    m.step_plan(np.array([1, 0, 0, 0], np.uint8))
    assert m.position.tolist() == [1, 2, 2, 2]


@pytest.mark.parametrize('name', sp.COMMAND_SESSIONS)
def test_both_roads_issue_the_command_calls_they_should(programmes, name):
    """A: device tables and masks, once per table the in-place write; the bias view straight into set_joint_torques; device requests
    and idle masks.  B: host arrays throughout.  The attachment calls take host arguments on both roads.  An observer is A's, and B's
    only where the record is compared."""
    _, N, nobj, _, _, _ = sp.SESSIONS[name]
    ops = programmes[name]
    dev, sd = _run(ops, 'device', N, nobj)
    host, sh = _run(ops, 'host', N, nobj)
    seen = set()
    for op, d, h in zip(ops, dev, host):
        k = op['kind']
        assert all(c[1] != 'device' for c in h), (k, h)
        if k in ('set_joint_torques', 'set_external_wrenches'):
            buf = {'set_joint_torques': 'joint_torque_buffer', 'set_external_wrenches': 'external_wrench_buffer'}[k]
            assert d == [('in_place ' + buf if op['inplace'] else k, 'device')] and h == [(k, 'host')], (k, d, h)
        elif k in ('clear_joint_torques', 'clear_external_wrenches'):
            call = k.replace('clear', 'set')
            assert d == [(call, None if op['mask'] is None else 'device')] and h == [(call, None if op['mask'] is None else 'host')]
        elif k == 'torques_from_dynamics':
            assert d == [('posture_dynamics', None), ('set_joint_torques', 'device')] and h == [('posture_dynamics', None), ('set_joint_torques', 'host')]
        elif k in ('attach', 'attach_capture'):
            assert d == h == [('attach_objects', 'host')]
        elif k in ('detach', 'detach_all'):
            assert d == h == [('detach_objects', None if k == 'detach_all' else 'host')]
        elif k == 'macro_invalidate':
            assert d == [(k, None if op['mask'] is None else 'device')] and h == [(k, None if op['mask'] is None else 'host')]
        elif k == 'step_macro':
            assert d == [('step_macro_device', 'device')] and h == [('step_macro_device', 'host')]
        elif k in sp.C_OBSERVERS:
            call = {'signed_distance_at': 'signed_distance', 'swept_clearance_refused': 'swept_clearance'}.get(k, k)
            assert [c[0] for c in d] == [call], (k, d)
            assert [c[0] for c in h] == ([call] if op['compared'] else []), (k, h)
        seen.add(k)
    assert seen >= set(sp.C_MUTATORS) | set(sp.C_OBSERVERS) | {'step_macro'}
    # both Sessions end with the same model, the one of the records alone
    model = sp.MacroModel(N)
    for op in ops:
        model.apply(op)
    for s in (sd, sh):
        assert np.array_equal(s.macro.position, model.position) and np.array_equal(s.macro.record, model.record, equal_nan=True) and not s.attached
    assert sd.read.keys() >= sh.read.keys() and set(sd.read) == {'joint_torques', 'external_wrenches', 'attachments'}


def test_written_command_values_are_what_the_calls_get():
    """the records' arrays reach the calls as they are: a recording env keeps the arguments"""
    _, N, nobj, _, _, length = sp.SESSIONS['c5']
    ops = sp.program(sp.SESSIONS['c5'][0], N, nobj, length, commands=True)
    got = []

    class Keep(FakeEnv):
        def __getattr__(self, name):
            inner = FakeEnv.__getattr__(self, name)

            def call(*args, **kw):
                got.append((name, args, kw))
                return inner(*args, **kw)
            return call
    for road in ('host', 'device'):
        env = Keep(N, nobj)
        s = sp.Session(env, road, to_device=_Dev)
        s.copy_in_place = lambda e, name, table, mask: got.append((name, (table, mask), {}))
        s.setup()
        val = lambda a: a.a if isinstance(a, _Dev) else a
        for op in ops:
            del got[:]
            s.apply(op)
            k = op['kind']
            if k in ('set_joint_torques', 'set_external_wrenches'):
                _, args, _ = got[-1]
                assert val(args[0]) is op['torques' if k == 'set_joint_torques' else 'wrenches'] and val(args[1]) is op['mask']
            elif k == 'attach':
                assert got[-1][1][0] is op['links'] and got[-1][1][1] is op['rel'] and got[-1][1][2] is op['mask']
            elif k == 'attach_capture':
                assert got[-1][1][0] is op['links'] and got[-1][1][1] is None
            elif k == 'step_macro':
                _, args, kw = got[-1]
                assert val(args[0]) is op['macro'] and val(kw['idle']) is op['idle']
                assert (kw['render'] is op['flags']) if op['render'] == 2 else kw['render'] == bool(op['render'])
            elif k in sp.C_OBSERVERS and not got:
                assert road == 'host' and not op['compared']          # (a silent record is A's alone)
            elif k == 'posture_dynamics':
                _, args, kw = got[-1]
                assert all(val(a) is b for a, b in zip(args, (op['postures'], op['velocities'], op['accelerations']))) and kw['inverse'] == op['inverse']
            elif k == 'carried_sweep':
                assert val(got[-1][1][0]) is op['segments'] and got[-1][2]['safety'] == op['safety']
    # the ranges of the issue: the arm stays in range
    t = np.concatenate([o['torques'] for o in ops if o['kind'] == 'set_joint_torques'])
    w = np.concatenate([o['wrenches'] for o in ops if o['kind'] == 'set_external_wrenches'])
    assert np.abs(t[:, :7]).max() <= 5.0 and np.abs(t[:, 7:]).max() <= 0.2 and np.abs(w[..., :3]).max() <= 4.0 and np.abs(w[:, :11, 3:]).max() <= 0.3
    req = np.concatenate([o['macro'] for o in ops if o['kind'] == 'step_macro'])
    assert (req[np.isfinite(req).all(axis=1)] >= sp.MACRO_LO).all() and (req[np.isfinite(req).all(axis=1)] <= sp.MACRO_HI).all()


def test_the_module_still_imports_neither_torch_nor_the_library_for_a_command_programme():
    import subprocess
    import sys
    code = ("import sys; from tests import session_program as sp; seed, N, nobj = sp.SESSIONS['c5'][:3]; "
            "sp.check_command_conditions(sp.program(seed, N, nobj, sp.C_LENGTH, commands=True), sp.C_LENGTH, N, nobj); "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('torch', 'real_robots_amd')], sys.modules.keys()")
    subprocess.check_call([sys.executable, '-c', code], cwd=str(__import__('pathlib').Path(__file__).resolve().parents[1]))


@pytest.mark.parametrize('name', sp.COMMAND_SESSIONS)
def test_the_command_anchors_are_decided(programmes, name):
    """The float64 anchor of the GPU test sets NO item aside: for the very anchor records of c70 and c5, the first four envs, the
    default table, the anchor's attach and the probe's postures, the reference decides every (env, pair) and (env, posture, pair) item,
    at the present joints and at the postures; a good share of the items has a shape of an attached object, and they are more than a
    centimetre from where the state alone would put them (a query that ignored the attachments would miss the bound)."""
    from tests import numpy_distance as nd
    from tests import numpy_posture as npo
    _, N, nobj, _, _, _ = sp.SESSIONS[name]
    ops = programmes[name]
    at = [i for i, o in enumerate(ops) if sp.is_command_anchor(o)]
    assert [ops[i]['kind'] for i in at] in (['set_state', 'write_state'], ['write_state', 'set_state'])
    q = sp.probe_arguments(N, nobj)
    n = min(N, sp.ANCHOR_ENVS)
    for i in at:
        attach = ops[i - 1]
        assert attach['kind'] == 'attach' and attach['mask'] is None and (attach['links'][:n] >= 0).any(axis=1).sum() >= n - 1
        r = sp.command_anchor_references(attach, ops[i], nobj, q)
        for key, rows in (('now', n), ('po', n * sp.PROBE_K)):
            ref, att = r[key], r['att_' + key]
            assert ref['decided'].shape == att.shape == (rows, len(r['pairs'])) and ref['decided'].all(), (name, i, key, np.argwhere(~ref['decided']).tolist())
            assert att.sum() >= 0.25 * att.size
        left = nd.reference(npo.rows(r['state'], q['postures'][:n]), r['pairs'])
        moved = np.abs(left['d'] - r['po']['d'])[r['att_po']]
        assert (moved > 0.01).mean() > 0.9 and not np.abs(left['d'] - r['po']['d'])[~r['att_po']].any()
        assert all(np.isfinite(v).all() for v in r['dynamics'].values())
