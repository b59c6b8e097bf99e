"""CPU tests (-m "not gpu") of the device-resident goals and episodes: the C boundary (header, binding), the independent numpy
restatement of one update (tests/numpy_episode.py) on hand-written cases, the goal arrays built from Goal objects, and the vector
env's argument checks (which run before any device is touched)."""
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import OBJECT_NAMES, BatchedREALRobotEnv
from real_robots_amd.envs.env import Goal
from tests import numpy_episode as ne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('rr_set_goals', 'rr_set_env_goals', 'rr_set_episode', 'rr_episode_update', 'rr_episode_buffer')


def _header():
    return open(os.path.join(ROOT, 'include', 'realrobot.h')).read()


def test_header_declares_the_calls_and_the_episode_enum_in_abi_7():
    h = _header()
    for name in CALLS:
        assert re.search(r'\bint\s+%s\s*\(\s*rr_env\s*\*\s*env\b' % name, h), name
    ep = dict((k, int(v)) for k, v in re.findall(r'\b(RR_EP_[A-Z_]+)\s*=\s*(\d+)', h))
    assert ep == {'RR_EP_SCORE': 0, 'RR_EP_REWARD': 1, 'RR_EP_DONE': 2, 'RR_EP_GOAL_INDEX': 3, 'RR_EP_EPISODE': 4, 'RR_EP_FINAL_OBS': 5,
                  'RR_EP_GOAL_POS': 6, 'RR_EP_GOAL_RGB': 7, 'RR_EP_COUNT': 8}
    assert (nat.EP_SCORE, nat.EP_REWARD, nat.EP_DONE, nat.EP_GOAL_INDEX, nat.EP_EPISODE, nat.EP_FINAL_OBS, nat.EP_GOAL_POS,
            nat.EP_GOAL_RGB) == tuple(range(8)) and len(nat.EP_NAMES) == 8
    # additive: the ABI version and the field enum are where they were
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert int(re.search(r'\bRR_F_COUNT\s*=\s*(\d+)', h).group(1)) == 16
    doc = h[h.index('int rr_evaluate_goals('):h.index('int rr_episode_buffer(')]
    for cite in ('env.py:151-166', 'env.py:181-200', 'env.py:345-352'):
        assert cite in doc, cite
    assert 'POINTER MAY CHANGE' in doc and 'checkpoints do not carry it' in doc and 're-bases' in doc


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    for name in CALLS:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None
    assert len(L.rr_set_goals.argtypes) == 6 and len(L.rr_set_env_goals.argtypes) == 3 and len(L.rr_set_episode.argtypes) == 3
    assert len(L.rr_episode_update.argtypes) == 2 and len(L.rr_episode_buffer.argtypes) == 4
    assert L.rr_abi_version() == 7


# ---------------------------------------------------------------------------------------------- numpy restatement, by hand
def test_numpy_score_by_hand():
    """An object 10 cm from its goal scores 0.25 (the constant's definition), one on its goal 1; only flagged objects count."""
    pos = np.array([[0.0, 0.0, 0.5], [0.1, 0.2, 0.5], [0.3, 0.3, 0.3]], np.float32)
    fin = np.array([[0.1, 0.0, 0.5], [0.1, 0.2, 0.5], [np.nan, np.nan, np.nan]], np.float32)
    assert abs(float(ne.score(pos, fin, [1, 0, 0])) - 0.25) < 1e-6
    assert abs(float(ne.score(pos, fin, [1, 1, 0])) - 1.25) < 1e-6
    assert abs(float(ne.score(pos, fin, [3, 3, 2])) - 1.25) < 1e-6          # bit 1 alone does not count
    assert ne.score(pos, fin, [0, 2, 0]) == 0 and ne.score(pos, fin, [0, 0, 0]).dtype == np.float32
    assert ne.score(pos, fin, [1, 1, 0]) == np.float32(np.float32(0.0) + ne.score(pos, fin, [1, 0, 0])) + np.float32(1.0)


def test_numpy_done_bits_and_next_index():
    t, e = np.array([0, 5, 6, 7, 2, 2, 2]), np.array([0, 0, 0, 0, 1, 4, 2], np.uint32)
    assert ne.done_bits(t, e, 6).tolist() == [0, 0, 1, 1, 2, 2, 0]          # flag 2 (a refused command) freezes nothing
    assert ne.done_bits(t, e, 0).tolist() == [0, 0, 0, 0, 2, 2, 0] == ne.done_bits(t, e, -3).tolist()
    assert ne.done_bits([9], [5], 6).tolist() == [3]
    idx = np.array([0, 1, 2, -1], np.int32)
    assert ne.next_index(idx, 1, 3).tolist() == [1, 2, 0, -1]
    assert ne.next_index(idx, 0, 3).tolist() == [0, 1, 2, -1]               # stride 0 keeps the goal
    assert ne.next_index(idx, 7, 3).tolist() == [1, 2, 0, -1]               # stride > G
    assert ne.next_index(idx, -1, 3).tolist() == [2, 0, 1, -1]
    assert ne.next_index([0, -1], 5, 1).tolist() == [0, -1]                 # G = 1


def _table():
    """Three goals over three objects: goal 0 names all, goal 1 names only object 1 (one of three) and gives a start pose to
    object 2 alone, goal 2 names objects 0 and 2 and has no start pose."""
    final = np.full((3, 3, 3), np.nan, np.float32)
    start = np.full((3, 3, 7), np.nan, np.float32)
    flags = np.array([[3, 3, 3], [0, 1, 2], [1, 0, 1]], np.uint8)
    final[0] = [[0.0, 0.0, 0.5], [0.1, 0.0, 0.5], [0.2, 0.0, 0.5]]
    start[0] = [[0.0, 0.1, 0.5, 0, 0, 0, 1], [0.1, 0.1, 0.5, 0, 0, 0, 1], [0.2, 0.1, 0.5, 0, 0, 0, 1]]
    final[1, 1] = [0.1, 0.3, 0.5]
    start[1, 2] = [-0.2, 0.2, 0.5, 0, 0, 0, 1]
    final[2, 0], final[2, 2] = [0.0, -0.1, 0.5], [0.2, -0.1, 0.5]
    return start, final, flags


def test_numpy_update_by_hand():
    start, final, flags = _table()
    home = np.tile(np.array([[0.0, 0.0, 0.5], [0.1, 0.0, 0.5], [0.2, 0.0, 0.5]], np.float32), (4, 1, 1))
    rec = ne.Record(4, start, final, flags, horizon=6, stride=1)
    assert rec.goal_pos().shape == (4, 3, 3) and np.isnan(rec.goal_pos()).all()
    pos = home.copy()
    rec.set_env_goals([0, 1, 2, -1], pos)
    gp = rec.goal_pos()
    assert not np.isnan(gp[0]).any() and (gp[0] == final[0]).all()
    assert np.isnan(gp[1, 0]).all() and (gp[1, 1] == final[1, 1]).all() and np.isnan(gp[1, 2]).all()      # one of three named
    assert np.isnan(gp[3]).all()
    assert rec.prev[0] == np.float32(3.0) and rec.prev[3] == 0           # env 0 sits on its goal: re-based to 3
    # a step that moves object 0 of every env 10 cm in y
    pos[:, 0, 1] += 0.1
    out = rec.update(pos, [1, 1, 1, 1], [0, 0, 0, 0], reset_done=True, home_pos=home)
    assert out["done"].tolist() == [0, 0, 0, 0] and not out["reset"].any() and rec.episode.tolist() == [0, 0, 0, 0]
    assert abs(float(out["score"][0]) - 2.25) < 1e-6 and abs(float(out["reward"][0]) + 0.75) < 1e-6
    assert out["score"][3] == 0 and out["reward"][3] == 0               # no goal
    assert out["reward"][1] == 0                                        # goal 1 does not name object 0
    assert (out["reward"] == out["score"] - np.array([3.0, rec_prev1(final, home), rec_prev2(final, home), 0.0], np.float32)).all()
    # no further motion: rewards are exactly zero, whatever the score
    out2 = rec.update(pos, [2, 2, 2, 2], [0, 0, 0, 0], reset_done=True, home_pos=home)
    assert (out2["reward"] == 0).all() and (out2["score"] == out["score"]).all()
    # envs 0 and 3 truncate, env 2 is frozen; without reset_done nothing but the bits
    idx0 = rec.index.copy()
    out3 = rec.update(pos, [6, 3, 3, 6], [0, 0, 1, 0], reset_done=False, home_pos=home)
    assert out3["done"].tolist() == [1, 0, 2, 1] and not out3["reset"].any() and (rec.index == idx0).all()
    out4 = rec.update(pos, [6, 3, 3, 6], [0, 0, 1, 0], reset_done=True, home_pos=home)
    assert out4["reset"].tolist() == [True, False, True, True]
    assert rec.index.tolist() == [1, 1, 0, -1] and rec.episode.tolist() == [1, 0, 1, 1]
    assert out4["placed"].tolist() == [[False, False, True], [False] * 3, [True] * 3, [False] * 3]
    # the previous score of a reset env is the score of its start state: env 0 (goal 1) starts with object 1 at home, 30 cm away
    assert rec.prev[0] == ne.score(home[0], final[1], flags[1]) and rec.prev[3] == 0
    assert rec.prev[2] == ne.score(start[0][:, :3], final[0], flags[0])
    assert rec.prev[1] == out4["score"][1]
    assert (out4["score"] == out3["score"]).all()                       # the call still describes the finished episode


def rec_prev1(final, home):
    return ne.score(home[1], final[1], [0, 1, 2])


def rec_prev2(final, home):
    return ne.score(home[2], final[2], [1, 0, 1])


def test_numpy_single_goal_and_zero_stride():
    start, final, flags = _table()
    pos = np.zeros((2, 3, 3), np.float32)
    one = ne.Record(2, start[:1], final[:1], flags[:1], horizon=1, stride=1)          # G = 1
    one.set_env_goals([0, -1], pos)
    one.update(pos, [1, 1], [0, 0], True, home_pos=pos)
    assert one.index.tolist() == [0, -1] and one.episode.tolist() == [1, 1]
    keep = ne.Record(2, start, final, flags, horizon=1, stride=0)                     # stride 0
    keep.set_env_goals([2, 1], pos)
    keep.update(pos, [1, 0], [0, 0], True, home_pos=pos)
    assert keep.index.tolist() == [2, 1] and keep.episode.tolist() == [1, 0]
    far = ne.Record(2, start, final, flags, horizon=1, stride=8)                      # stride > G
    far.set_env_goals([2, 1], pos)
    far.update(pos, [1, 1], [0, 0], True, home_pos=pos)
    assert far.index.tolist() == [1, 0]


# ---------------------------------------------------------------------------------------------- Goal objects -> arrays
def test_goal_arrays_from_goal_objects():
    """Three hand-made goals, restated here as evaluate_batched gathers g_init, g_final and g_mask."""
    q = [0.0, 0.0, 0.0, 1.0]
    img = [np.full((4, 8, 3), 10 * (k + 1), np.uint8) for k in range(3)]
    goals = [Goal(initial_state={'cube': [0.0, 0.1, 0.5] + q, 'tomato': [0.1, 0.1, 0.5] + q, 'mustard': [0.2, 0.1, 0.5] + q},
                  final_state={'cube': [0.0, 0.0, 0.5] + q, 'tomato': [0.1, 0.0, 0.5] + q, 'mustard': [0.2, 0.0, 0.5] + q},
                  retina=img[0], challenge='2D'),
             Goal(initial_state={'mustard': [-0.2, 0.2, 0.5] + q}, final_state={'tomato': [0.1, 0.3, 0.5] + q}, retina=img[1], challenge='2D'),
             Goal(initial_state={}, final_state={'cube': [0.0, -0.1, 0.5] + q, 'orange': [9.0, 9.0, 9.0] + q}, retina=img[2], challenge='3D')]
    for names in (OBJECT_NAMES, OBJECT_NAMES[:1]):
        n_objects, G = len(names), len(goals)
        g_final = np.full((G, n_objects, 3), np.nan, np.float32)
        g_mask = np.zeros((G, n_objects), np.uint8)
        g_init = np.full((G, n_objects, 7), np.nan, np.float32)
        for k, g in enumerate(goals):
            for n_, pose in g.final_state.items():
                if n_ in names:
                    g_final[k, names.index(n_)] = np.asarray(pose, np.float32)[:3]
                    g_mask[k, names.index(n_)] = 1
            for n_, pose in g.initial_state.items():
                if n_ in names:
                    g_init[k, names.index(n_)] = np.asarray(pose, np.float32)
        start, final, flags, rgb = BatchedREALRobotEnv.goal_arrays(goals, names)
        assert start.dtype == final.dtype == np.float32 and flags.dtype == np.uint8
        assert np.array_equal(start, g_init, equal_nan=True) and np.array_equal(final, g_final, equal_nan=True)
        assert ((flags & 1) == g_mask).all() and (((flags & 2) != 0) == ~np.isnan(g_init[..., 0])).all()
        assert rgb.shape == (3, 4, 8, 3) and all((rgb[k] == img[k]).all() for k in range(3))
    goals[1].retina = None
    assert BatchedREALRobotEnv.goal_arrays(goals, OBJECT_NAMES)[3] is None


# ---------------------------------------------------------------------------------------------- vector env argument checks
def test_vector_env_checks_goals_before_it_touches_a_device(tmp_path):
    from real_robots_amd.vector import REALRobotVectorEnv
    kw = dict(objects=3, eye_width=16, eye_height=8, device=10 ** 6)      # a device that does not exist: reaching it is an error of its own
    q = [0.0, 0.0, 0.0, 1.0]
    good = Goal(initial_state={}, final_state={'cube': [0.0, 0.0, 0.5] + q}, retina=np.zeros((8, 16, 3), np.uint8))
    with pytest.raises(ValueError, match="empty"):
        REALRobotVectorEnv(2, goals=[], **kw)
    with pytest.raises(ValueError, match="no goals dataset"):
        REALRobotVectorEnv(2, goals=str(tmp_path / 'nowhere.npy.npz'), **kw)
    with pytest.raises(ValueError, match="not a Goal"):
        REALRobotVectorEnv(2, goals=[good, {'final_state': {}}], **kw)
    with pytest.raises(ValueError, match="names none"):
        REALRobotVectorEnv(2, goals=[Goal(initial_state={}, final_state={'orange': [0.0, 0.0, 0.5] + q})], **kw)
    with pytest.raises(ValueError, match="retina has shape"):
        REALRobotVectorEnv(2, goals=[Goal(initial_state={}, final_state={'cube': [0.0, 0.0, 0.5] + q}, retina=np.zeros((8, 12, 3), np.uint8))], **kw)
    with pytest.raises(ValueError, match="path or a list"):
        REALRobotVectorEnv(2, goals=7, **kw)
    # a good list passes the checks and only then fails on the device
    with pytest.raises(nat.NativeError):
        REALRobotVectorEnv(2, goals=[good], **kw)


def test_vector_env_signature_keeps_its_defaults():
    """goals=None is the default and comes after every existing argument: existing callers and their spaces are untouched."""
    import inspect
    from real_robots_amd.envs.robot import Kuka
    from real_robots_amd.vector import REALRobotVectorEnv
    p = inspect.signature(REALRobotVectorEnv.__init__).parameters
    assert p['goals'].default is None and p['goal_stride'].default == 1
    assert list(p)[-2:] == ['goals', 'goal_stride'] and list(p)[-3] == 'contact_obs'
    # the single spaces come from Kuka alone, goals or not: "goal" was one of the reference's four standard keys all along
    sp = Kuka(True, 3, 16, 8, env=None).observation_space.spaces
    assert sp['goal'].shape == (8, 16, 3) and 'goal_positions' in sp
