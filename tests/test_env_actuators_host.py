"""Per-env actuators without a GPU: the two entry points are declared, bound and exported and refuse a NULL env (ABI still 7); the
Python layer checks shapes, signs and finiteness before the library is called; the vector env's actuator draws (with a stand-in for
the batched env) are reproducible per seed, stay in their ranges times the handle's values, are redrawn for the truncated envs only,
and leave the seeded dynamics / camera / appearance draws as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd import vector
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NJ = 11
DEFAULT_ROW = np.array([0.1, 1.0, 100000.0, 0.5], np.float32)


def test_header_binding_and_library_export_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    assert re.search(r'\bint rr_set_env_actuators\(rr_env \*env, const float \*act_host, const uint8_t \*env_mask_host\);', hdr)
    assert re.search(r'\bint rr_get_env_actuators\(rr_env \*env, float \*act_out_host\);', hdr)
    assert int(re.search(r'#define RR_ABI_VERSION (\d+)', hdr).group(1)) == 7 == nat.RR_ABI_VERSION
    for s in ('rr_set_env_actuators', 'rr_get_env_actuators'):
        assert s in nat.SYMBOLS
    assert nat.ACT_ROW == ('kp', 'kd', 'max_force', 'damping') and nat.N_JOINTS == NJ
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    rows = np.ones((2, NJ, 4), np.float32)
    assert L.rr_set_env_actuators(None, rows.ctypes.data, None) == -1
    assert L.rr_set_env_actuators(None, None, None) == -1
    assert L.rr_get_env_actuators(None, rows.ctypes.data) == -1


class _ActLib:
    """Stands in for the library: holds one batch's table, records what rr_set_env_actuators is given."""

    def __init__(self, n):
        self.raw = np.tile(DEFAULT_ROW, (n, NJ, 1))
        self.calls, self.n = [], n

    def rr_get_env_actuators(self, h, ptr):
        C.memmove(ptr, self.raw.ctypes.data, self.raw.nbytes)
        return 0

    def rr_set_env_actuators(self, h, ptr, mask):
        rows = None if ptr is None else np.ctypeslib.as_array((C.c_float * self.raw.size).from_address(ptr)).reshape(self.raw.shape).copy()
        m = None if mask is None else np.ctypeslib.as_array((C.c_uint8 * self.n).from_address(mask)).copy()
        self.calls.append((rows, m))
        return 0


def _fake_env(n=4):
    env = BatchedREALRobotEnv.__new__(BatchedREALRobotEnv)
    env.L, env.h, env.N, env.n_objects = _ActLib(n), None, n, 3
    return env


@pytest.mark.parametrize('kw', [
    dict(kp=np.ones((3, NJ))), dict(kp=np.ones((4, NJ + 1))), dict(kd=np.ones(4)), dict(max_force=np.ones((4, NJ, 1))),
    dict(damping=np.ones(9)), dict(kp=np.nan), dict(kd=np.inf), dict(max_force=-1.0), dict(damping=-0.5), dict(kp=1e39),
    dict(kp=0.2, kd=[1.0] * 10 + [-1.0]), dict(kp=0.2, damping=np.nan), dict(kp=0.2, env_mask=np.ones(5)),
    dict(env_mask=np.ones((4, 1))), dict(damping='soft')])
def test_bad_arguments_raise_before_the_library_is_called(kw):
    env = _fake_env()
    with pytest.raises(ValueError) as ei:
        env.set_env_actuators(**kw)
    assert env.L.calls == []
    bad = [k for k in ('kp', 'kd', 'max_force', 'damping') if k in kw]
    if 'env_mask' in kw:
        assert 'env_mask' in str(ei.value)
    else:
        assert bad[-1] in str(ei.value), "the message names the field"


def test_broadcast_arguments_reach_the_library_and_none_keeps_what_is_in_force():
    env = _fake_env()
    per_joint = np.linspace(0.3, 0.05, NJ)
    env.set_env_actuators(kp=per_joint, max_force=0.0, env_mask=[1, 0, 0, 1])
    rows, mask = env.L.calls[-1]
    assert mask.tolist() == [1, 0, 0, 1] and rows.dtype == np.float32
    assert np.array_equal(rows[..., 0], np.tile(per_joint.astype(np.float32), (4, 1))) and np.all(rows[..., 2] == 0.0)
    assert np.all(rows[..., 1] == DEFAULT_ROW[1]) and np.all(rows[..., 3] == DEFAULT_ROW[3])          # kd, damping kept
    per_env = np.arange(4.0)[:, None] + 1.0
    env.set_env_actuators(damping=per_env)
    rows, mask = env.L.calls[-1]
    assert mask is None and np.array_equal(rows[..., 3], np.tile(per_env.astype(np.float32), (1, NJ)))
    env.set_env_actuators(env_mask=[0, 1, 0, 0])              # nothing given: back to the handle's values for the masked envs
    rows, mask = env.L.calls[-1]
    assert rows is None and mask.tolist() == [0, 1, 0, 0]
    d = env.env_actuators()
    assert sorted(d) == ['damping', 'kd', 'kp', 'max_force'] and all(v.shape == (4, NJ) and v.dtype == np.float32 for v in d.values())


class _FakeBatch:
    """Stands in for BatchedREALRobotEnv behind the vector env: records actuator, appearance, camera and dynamics uploads."""

    def __init__(self, num_envs, objects=3, width=320, height=240, **kw):
        self.N, self.n_objects = num_envs, objects
        self.act_calls, self.app_calls, self.cam_calls, self.dyn_calls = [], [], [], []
        self._dyn = np.tile(np.array([1.5, 1e-3, 1e-3, 1e-3, 0.5, 0.1, 0.0, 0.0], np.float32), (num_envs, objects, 1))
        self._col = np.tile(np.asarray(load_model()['inst_color'], np.float32), (num_envs, 1, 1))
        self._act0 = np.tile(DEFAULT_ROW * np.linspace(1.0, 2.0, NJ, dtype=np.float32)[:, None], (num_envs, 1, 1))
        self._act = self._act0.copy()

    def default_env_actuators(self):
        return BatchedREALRobotEnv._actuators_dict(self._act0)

    def env_actuators(self):
        return BatchedREALRobotEnv._actuators_dict(self._act)

    def set_env_actuators(self, kp=None, kd=None, max_force=None, damping=None, env_mask=None):
        m = np.ones(self.N, bool) if env_mask is None else np.asarray(env_mask).astype(bool)
        for k, v in enumerate((kp, kd, max_force, damping)):
            if v is not None:
                self._act[m, :, k] = np.broadcast_to(np.asarray(v, np.float32), (self.N, NJ))[m]
        self.act_calls.append(m.copy())

    def default_env_appearance(self):
        light = np.array([-50.0, 30.0, 100.0]) / np.linalg.norm([-50.0, 30.0, 100.0])
        return {'colours': self._col.copy(), 'light_dirs': np.tile(light.astype(np.float32), (self.N, 1))}

    def set_env_appearance(self, colours=None, light_dirs=None, env_mask=None):
        self.app_calls.append((np.array(colours), np.array(light_dirs)))

    def set_env_cameras(self, views, projs, env_mask=None):
        self.cam_calls.append((np.array(views), np.array(projs)))

    def default_object_dynamics(self):
        return BatchedREALRobotEnv._dynamics_dict(self._dyn)

    def object_dynamics(self):
        return BatchedREALRobotEnv._dynamics_dict(self._dyn)

    def set_object_dynamics(self, env_mask=None, **kw):
        self.dyn_calls.append({k: np.array(v) for k, v in kw.items()})

    def reset(self, mask=None):
        pass

    def render(self):
        pass

    def step(self, cmd, render=False):
        pass

    def host(self, field):
        return np.zeros((self.N, 9), np.float32)


@pytest.fixture
def fake_batch(monkeypatch):
    monkeypatch.setattr(vector, 'BatchedREALRobotEnv', _FakeBatch)


RAND = {'kp': (0.8, 1.2), 'kd': (1.0, 1.2), 'max_force': (0.5, 1.0), 'damping': (0.5, 2.0)}


def _vec(n=6, **kw):
    return vector.REALRobotVectorEnv(n, eye_width=128, eye_height=96, render_every_step=False, **kw)


def test_actuator_draws_are_seeded_per_env_and_joint_and_within_range(fake_batch):
    a, b, c = _vec(actuator_randomization=RAND), _vec(actuator_randomization=RAND), _vec(actuator_randomization=RAND)
    _, ia = a.reset(seed=7)
    _, ib = b.reset(seed=7)
    _, ic = c.reset(seed=8)
    base = a._be.default_env_actuators()
    for k, (lo, hi) in RAND.items():
        va = ia['actuators'][k]
        assert va.shape == (6, NJ) and va.dtype == np.float32
        assert np.array_equal(va, ib['actuators'][k]) and not np.array_equal(va, ic['actuators'][k])
        assert np.array_equal(va, a._be.env_actuators()[k])
        ratio = va.astype(np.float64) / base[k]
        assert (ratio >= lo - 1e-6).all() and (ratio <= hi + 1e-6).all()
        assert len(np.unique(ratio)) == 6 * NJ, "every env and joint its own draw"
    assert a._be.act_calls[-1].all()


def test_the_generator_is_spawn_key_3_and_missing_fields_keep_the_handle_values(fake_batch):
    n, seed = 5, 12
    v = _vec(n, actuator_randomization={'kd': (1.0, 1.5), 'damping': (0.0, 3.0)})
    _, info = v.reset(seed=seed)
    base = v._be.default_env_actuators()
    rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(3,)))
    kd = rng.uniform(1.0, 1.5, size=(n, NJ))
    dm = rng.uniform(0.0, 3.0, size=(n, NJ))
    assert np.array_equal(info['actuators']['kd'], (base['kd'].astype(np.float64) * kd).astype(np.float32))
    assert np.array_equal(info['actuators']['damping'], (base['damping'].astype(np.float64) * dm).astype(np.float32))
    assert np.array_equal(info['actuators']['kp'], base['kp']) and np.array_equal(info['actuators']['max_force'], base['max_force'])


def test_autoreset_redraws_the_truncated_envs_only(fake_batch):
    v = vector.REALRobotVectorEnv(4, eye_width=64, eye_height=64, render_every_step=False, max_episode_steps=3,
                                  actuator_randomization=RAND)
    _, info0 = v.reset(seed=1)
    v._steps[:] = [0, 2, 0, 2]
    _, _, _, trunc, info = v.step(np.zeros((4, 9), np.float32))
    assert trunc.tolist() == [False, True, False, True]
    assert info['_actuators'].tolist() == [False, True, False, True]
    assert v._be.act_calls[-1].tolist() == [False, True, False, True]
    for k in RAND:
        assert np.all(info['actuators'][k] == info0['actuators'][k], axis=1).tolist() == [True, False, True, False]
    _, _, _, trunc, info = v.step(np.zeros((4, 9), np.float32))
    assert not trunc.any() and 'actuators' not in info


def test_actuator_randomization_leaves_the_other_draws_of_a_seed_unchanged(fake_batch):
    dyn = {'mass': (0.5, 2.0), 'friction': (0.5, 1.5)}
    cam = {'translation': 0.03, 'rotation': 3.0, 'fov': (75.0, 85.0)}
    app = {'colour': (0.6, 1.0), 'brightness': (0.8, 1.25), 'light': 35.0}
    a = _vec(dynamics_randomization=dyn, camera_randomization=cam, appearance_randomization=app)
    b = _vec(dynamics_randomization=dyn, camera_randomization=cam, appearance_randomization=app, actuator_randomization=RAND)

    def same(ia, ib):
        for k in ia['object_dynamics']:
            assert np.array_equal(ia['object_dynamics'][k], ib['object_dynamics'][k])
        for k in ('view', 'proj'):
            assert np.array_equal(ia['camera'][k], ib['camera'][k])
        for k in ('colours', 'light_dirs'):
            assert np.array_equal(ia['appearance'][k], ib['appearance'][k])
    _, ia = a.reset(seed=3)
    _, ib = b.reset(seed=3)
    same(ia, ib)
    assert 'actuators' not in ia and a._be.act_calls == [] and 'actuators' in ib
    for v in (a, b):                                      # ... and on the autoreset draws that follow
        v.max_episode_steps = 1
    _, _, _, _, ja = a.step(np.zeros((6, 9), np.float32))
    _, _, _, _, jb = b.step(np.zeros((6, 9), np.float32))
    same(ja, jb)


@pytest.mark.parametrize('bad', [{'stiffness': (0.5, 1.0)}, {'kp': (1.0, 0.5)}, {'kp': (-0.1, 1.0)}, {'kd': (0.5, np.inf)},
                                 {'kd': 0.5}, {'max_force': (np.nan, 1.0)}, {'damping': (1.0,)}])
def test_bad_actuator_randomization_raises(fake_batch, bad):
    with pytest.raises(ValueError):
        _vec(actuator_randomization=bad)
