"""CPU tests of the programmes that tests/test_gpu_session.py runs (tests/session_program.py): the coverage of the interleaving
does not depend on luck.  For the very seeds and sizes of the GPU test (session_program.SESSIONS), all three of them:

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

A recording fake of BatchedREALRobotEnv shows which calls each road issues."""
import numpy as np
import pytest

from tests import session_program as sp


@pytest.fixture(scope='module')
def programmes():
    return {name: sp.program(seed, N, nobj, length) for name, (seed, N, nobj, _, _, length) in sp.SESSIONS.items()}


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    return type(a) is type(b) and a == b


@pytest.mark.parametrize('name', list(sp.SESSIONS))
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


@pytest.mark.parametrize('name', list(sp.SESSIONS))
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


@pytest.mark.parametrize('name', list(sp.SESSIONS))
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
            side = self._side(args, kw)
            if name == 'step':
                side = 'device' if kw.get('device_ptr') is not None else 'host'
            flags = tuple(k for k in ('joint_pos', 'joint_vel', 'obj_pose', 'obj_vel', 'reset', 'fresh') if kw.get(k))
            self.log.append((name, side) + ((flags,) if name == 'write_state' else ()))
            if name == 'checkpoint':
                return np.zeros(4, np.uint8)
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
    s.setup()
    env.log.clear()
    per_op = []
    for op in ops:
        n = len(env.log)
        s.apply(op)
        per_op.append(env.log[n:])
    return per_op, s


@pytest.mark.parametrize('name', list(sp.SESSIONS))
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


def test_run_is_the_session_over_the_whole_programme(programmes):
    _, N, nobj, _, _, _ = sp.SESSIONS['n5']
    env = FakeEnv(N, nobj)
    s = sp.run(env, programmes['n5'], 'written', to_device=_Dev)
    per_op, _ = _run(programmes['n5'], 'written', N, nobj)
    calls = [c for c in env.log]
    assert calls[-sum(len(p) for p in per_op):] == [c for p in per_op for c in p]
    assert [c[0] for c in calls[:6]] == ['set_rays', 'snapshot_slots', 'set_goals', 'set_env_goals', 'set_episode', 'checkpoint']
    assert len(s.ckpts) == 1 + sum(o['kind'] == 'checkpoint' for o in programmes['n5']) and len(s.keep) > 0
