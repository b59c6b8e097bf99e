"""Per-env object dynamics (rr_set_object_dynamics / rr_get_object_dynamics; changeDynamics / getDynamicsInfo).

The core check: a batch whose envs carry different object dynamics steps every env exactly -- bit for bit, contacts, touch and
images included -- as a handle built from a model blob patched to that env's values does.  Then the same against the float oracle
on that patched blob, a sliding distance against Coulomb's law, checkpoints, validation, the facade and the vector env.
"""
import struct

import numpy as np
import pytest

import oracle.oracle as oracle_mod
from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests.test_gpu_contacts_fuzz import oracle_sensitivity, state_bounds, SENS_FACTOR

pytestmark = pytest.mark.gpu

W = H = 64
N_MIX = 96
SETS = ('default', 'heavy_cube', 'low_friction', 'bouncy_rolling')


def _entries(blob):
    """name -> (dtype code, offset, nbytes) of the model blob's table (the layout real_robots_amd/model.py reads)."""
    magic, n, _ = struct.unpack_from('<8sII', blob, 0)
    assert magic == b'RRMODEL1'
    out = {}
    for i in range(n):
        name, dt, nd, s0, s1, s2, s3, off, nb = struct.unpack_from('<32sII4IQQ', blob, 16 + i * 72)
        out[name.split(b'\0')[0].decode()] = (dt, off, nb)
    return out


def _arr(blob, ent, name, shape):
    dt, off, nb = ent[name]
    return np.frombuffer(blob, dtype=np.float32 if dt == 0 else np.int32, count=nb // 4, offset=off)[:int(np.prod(shape))].reshape(shape)


def patched_blob(rows):
    """The default blob with the objects' dynamics replaced by `rows` (float32 [3, 8] in rr_set_object_dynamics' row layout):
    obj_mass, obj_inertia and the shape_mat / shape_roll rows of every collision shape an object owns."""
    base = nat.model_blob()
    ent = _entries(base)
    b = bytearray(base)
    ns = ent['shape_owner'][2] // 16
    owner = _arr(base, ent, 'shape_owner', (ns, 4))

    def put(name, idx, values):
        _, off, _ = ent[name]
        v = np.asarray(values, np.float32).ravel()
        b[off + 4 * idx: off + 4 * idx + 4 * v.size] = v.tobytes()
    for o in range(3):
        put('obj_mass', o, rows[o, 0])
        put('obj_inertia', 3 * o, rows[o, 1:4])
        for s in range(ns):
            if owner[s, 0] == 2 and owner[s, 1] == o:
                put('shape_mat', 2 * s, rows[o, 4:6])
                put('shape_roll', 2 * s, rows[o, 6:8])
    return bytes(b)


def default_rows():
    base = nat.model_blob()
    ent = _entries(base)
    ns = ent['shape_owner'][2] // 16
    owner = _arr(base, ent, 'shape_owner', (ns, 4))
    mat, roll = _arr(base, ent, 'shape_mat', (ns, 2)), _arr(base, ent, 'shape_roll', (ns, 2))
    rows = np.zeros((3, 8), np.float32)
    rows[:, 0] = _arr(base, ent, 'obj_mass', (3,))
    rows[:, 1:4] = _arr(base, ent, 'obj_inertia', (3, 3))
    for o in range(3):
        s = [s for s in range(ns) if owner[s, 0] == 2 and owner[s, 1] == o][0]
        rows[o, 4:6], rows[o, 6:8] = mat[s], roll[s]
    return rows


def param_sets():
    d = default_rows()
    heavy = d.copy()
    heavy[0, 0:4] *= 5.0                          # the cube five times heavier (uniform density: the inertia follows)
    low = d.copy()
    low[:, 4] = 0.1                               # low lateral friction on every object
    bouncy = d.copy()
    bouncy[:, 5], bouncy[:, 6], bouncy[:, 7] = 0.8, 0.05, 0.05
    return [d, heavy, low, bouncy]


def mixed_dyn(sets, n):
    return np.stack([sets[i % len(sets)] for i in range(n)])


def _drive(envs, steps, seed, on_step=None):
    """Same commands for every handle: macro pushes (the first half), then full-range joint commands that press the links onto the
    table; a render every 10th step."""
    rng = np.random.default_rng(seed)
    n = envs[0].N
    macro = np.stack([rng.uniform([-0.25, -0.4], [0.05, 0.4], size=(2, 2)) for _ in range(n)]).astype(np.float32)
    for e in envs:
        e.plan_macro(macro)
    for t in range(steps):
        render = t % 10 == 9
        if t < steps // 2:
            for e in envs:
                e.step_plan(render=render)
        else:
            cmd = (synthetic_actions(range(n), t, seed=seed) * 1.6).astype(np.float32)
            for e in envs:
                e.step(cmd, render=render)
        if on_step:
            on_step(t, render)


def _compare(mixed, uniform, envs, with_contacts):
    st_m, st_u = mixed.state, uniform.state
    assert np.array_equal(st_m[envs].view(np.uint32), st_u[envs].view(np.uint32)), "state differs"
    assert np.array_equal(mixed.host(nat.F_TOUCH)[envs], uniform.host(nat.F_TOUCH)[envs]), "touch differs"
    for f in (nat.F_RGB, nat.F_DEPTH, nat.F_MASK):
        assert np.array_equal(mixed.host(f)[envs], uniform.host(f)[envs]), "image field %d differs" % f
    if with_contacts:
        for i in envs:
            cm, cu = mixed.contacts(i), uniform.contacts(i)
            assert cm.shape == cu.shape and np.array_equal(cm.view(np.uint32), cu.view(np.uint32)), "contacts of env %d differ" % i


PATHS = {'default': {}, 'no_split': {'RR_NO_SPLIT': '1', 'RR_NO_LOOKAHEAD': '1'}, 'small_pool': {'RR_SOLVER_POOL': '300'}}


@pytest.mark.parametrize('path', list(PATHS))
def test_per_env_dynamics_equal_patched_models_bit_for_bit(monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    sets = param_sets()
    mixed = BatchedREALRobotEnv(N_MIX, objects=3, width=W, height=H)
    mixed.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(mixed_dyn(sets, N_MIX)))
    uniform = []
    for s in sets:
        with monkeypatch.context() as m:
            m.setattr(nat, 'model_blob', lambda b=patched_blob(s): b)
            uniform.append(BatchedREALRobotEnv(N_MIX, objects=3, width=W, height=H))
    assert np.array_equal(uniform[0].object_dynamics()['mass'], mixed.default_object_dynamics()['mass'])
    members = [np.arange(k, N_MIX, len(sets)) for k in range(len(sets))]
    cls_seen = np.zeros(N_MIX, np.int64)

    def check(t, render):
        cls_seen[:] = np.maximum(cls_seen, mixed.host(nat.F_ENV_CLASS))
        if render:
            for k in range(len(sets)):
                _compare(mixed, uniform[k], members[k], with_contacts=(t % 50 == 49))
    _drive([mixed] + uniform, 300, seed=7, on_step=check)
    for k in range(1, len(sets)):
        assert (cls_seen[members[k]] >= 1).any() and (cls_seen[members[k]] == 2).any(), \
            "set %s never reached the heavy / very heavy solve" % SETS[k]
    # the mixed batch is not the default batch: the sets really changed something
    assert not np.array_equal(mixed.state[members[2]], uniform[0].state[members[2]])
    for e in [mixed] + uniform:
        e.close()


def test_one_step_differentials_against_the_oracle_on_patched_blobs(monkeypatch):
    sets = param_sets()
    mixed = BatchedREALRobotEnv(N_MIX, objects=3, width=W, height=H)
    mixed.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(mixed_dyn(sets, N_MIX)))
    _drive([mixed], 160, seed=3)
    rng = np.random.default_rng(1)
    cmd = (synthetic_actions(range(N_MIX), 160, seed=3) * 1.6).astype(np.float32)
    st0 = mixed.state
    ncs = np.array([len(mixed.contacts(i)) for i in range(N_MIX)])
    picks = {k: int(max(range(k, N_MIX, 4), key=lambda i: ncs[i])) for k in range(1, 4)}
    caches = {i: mixed.contacts(i) for i in picks.values()}
    mixed.step(cmd)
    st1 = mixed.state
    for k, i in picks.items():
        assert ncs[i] > 0
        with monkeypatch.context() as m:
            m.setattr(oracle_mod, 'model_blob', lambda b=patched_blob(sets[k]): b)
            o = oracle_mod.Oracle(3, W, H, f32=True)
        o.state = st0[i].astype(np.float64)
        o.set_contact_cache(caches[i])
        o.step(cmd[i].astype(np.float64))
        cd, co = mixed.contacts(i), o.contacts()
        keep = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]          # everything but the normal force, mu included
        assert cd.shape == co.shape and np.array_equal(cd[:, keep], co[:, keep].astype(np.float32)), "contact list of set %s" % SETS[k]
        ref = o.state.copy()
        fmax = float(cd[:, 10].max()) if len(cd) else 0.0
        bj, bo, bv = state_bounds(fmax)
        dj = float(np.abs(st1[i][:22] - ref[:22]).max())
        dobj = np.abs(st1[i][22:61] - ref[22:61]).reshape(3, 13)
        do, dv = float(dobj[:, :7].max()), float(dobj[:, 7:].max())
        if dj > bj or do > bo or dv > bv:
            sj, so, sv = oracle_sensitivity(o, st0[i], caches[i], cmd[i], ref, 3, rng)
            assert dj <= max(bj, SENS_FACTOR * sj) and do <= max(bo, SENS_FACTOR * so) and dv <= max(bv, SENS_FACTOR * sv), \
                (SETS[k], dj, do, dv, sj, so, sv)
    mixed.close()


def test_sliding_distance_follows_coulomb_friction():
    """A cube kicked along the table stops after v^2 / (2 mu g), mu = mu_cube * mu_table (the product rule of the pair).  Error
    budget of the tolerance (15 % + 2 mm): linear damping 0.04 (1 + |v|) / s over the < 0.25 s of sliding (< 1.5 %), the
    explicit time step (5 ms against a stopping time of 80 ms or more: one step of sliding at most, < 6 %), and the friction
    pyramid of two tangent rows, which is exact for a slide along one of them and within a few % along any other."""
    g = 9.81
    mus = np.array([0.2, 0.35, 0.5], np.float32)
    env = BatchedREALRobotEnv(3, objects=1, width=W, height=H)
    mu_table = 1.0       # the table's lateral friction in the model (shape_mat of its boxes)
    env.set_object_dynamics(friction=mus[:, None])
    hold = np.zeros((3, 9), np.float32)
    hold[:] = env.host(nat.F_JOINTS)      # the arm holds its start pose, away from the cube
    for _ in range(150):                  # the cube lands and settles
        env.step(hold)
    st = env.state
    v0 = 0.4
    st[:, 22 + 7] = v0                    # x velocity of the cube (pos3 quat4 lin3 ang3)
    st[:, 22 + 8:22 + 13] = 0.0
    env.state = st
    x0 = st[:, 22].copy()
    for _ in range(200):
        env.step(hold)
    d = env.state[:, 22] - x0
    expect = v0 ** 2 / (2 * mus * mu_table * g)
    assert np.all(np.abs(d - expect) <= 0.15 * expect + 0.002), (d, expect)
    assert d[0] > d[1] > d[2]
    env.close()


def test_checkpoint_carries_dynamics_and_restores_bitwise(monkeypatch):
    sets = param_sets()
    n = 24
    a = BatchedREALRobotEnv(n, objects=3, width=W, height=H)
    a.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(mixed_dyn(sets, n)))
    _drive([a], 60, seed=5)
    ck = a.checkpoint()
    saved = a.object_dynamics()
    cmd = (synthetic_actions(range(n), 60, seed=11) * 1.6).astype(np.float32)
    for _ in range(20):
        a.step(cmd)
    ref_state, ref_c = a.state, [a.contacts(i) for i in range(n)]
    # save, change, restore: the saved values come back
    a.set_object_dynamics(mass=3.0, friction=0.3)
    a.restore(ck)
    for k, v in saved.items():
        assert np.array_equal(a.object_dynamics()[k], v)
    # restore into a handle that had other dynamics, then step: bitwise the uninterrupted run
    b = BatchedREALRobotEnv(n, objects=3, width=W, height=H)
    b.set_object_dynamics(mass=0.7, friction=1.2, restitution=0.5)
    b.step(cmd)
    b.restore(ck)
    for _ in range(20):
        b.step(cmd)
    assert np.array_equal(b.state.view(np.uint32), ref_state.view(np.uint32))
    for i in range(n):
        assert np.array_equal(b.contacts(i).view(np.uint32), ref_c[i].view(np.uint32))
    # reset and set_state leave the dynamics as they are
    b.reset()
    b.state = b.state
    b.set_object_poses(b.host(nat.F_OBJ_POSE))
    for k, v in saved.items():
        assert np.array_equal(b.object_dynamics()[k], v)
    a.close()
    b.close()


def test_validation_and_masks():
    n = 8
    env = BatchedREALRobotEnv(n, objects=3, width=W, height=H)
    before = env.object_dynamics()
    bad = [dict(mass=0.0), dict(mass=-1.0), dict(mass=np.nan), dict(inertia=np.inf), dict(inertia=[0.0, 1e-3, 1e-3]),
           dict(friction=-0.1), dict(restitution=np.nan), dict(rolling=-1e-3), dict(spinning=np.inf),
           dict(mass=np.ones(n)), dict(inertia=np.ones((n, 3))), dict(friction=np.ones((2, 2))),
           dict(mass=1.0, env_mask=np.ones(3, np.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            env.set_object_dynamics(**kw)
        for k, v in before.items():
            assert np.array_equal(env.object_dynamics()[k], v), kw
    # the C entry point itself: one bad row anywhere fails the whole call and changes nothing
    raw = env._dynamics_raw()
    raw[:, :, 0] = 2.0
    raw[5, 1, 4] = -0.5
    assert env.L.rr_set_object_dynamics(env.h, raw.ctypes.data, None) == -1
    raw[5, 1, 4] = 0.5
    raw[6, 2, 2] = 0.0
    assert env.L.rr_set_object_dynamics(env.h, raw.ctypes.data, None) == -1
    assert env.L.rr_get_object_dynamics(env.h, None) == -1
    for k, v in before.items():
        assert np.array_equal(env.object_dynamics()[k], v)
    # a masked set changes only the masked envs
    mask = np.zeros(n, np.uint8)
    mask[[1, 4]] = 1
    env.set_object_dynamics(mass=4.0, friction=0.25, env_mask=mask)
    after = env.object_dynamics()
    for i in range(n):
        if mask[i]:
            assert np.all(after['mass'][i] == 4.0) and np.all(after['friction'][i] == np.float32(0.25))
            assert np.allclose(after['inertia'][i], before['inertia'][i] * (4.0 / before['mass'][i])[:, None], rtol=1e-6)
        else:
            for k in after:
                assert np.array_equal(after[k][i], before[k][i])
    env.close()


def test_facade_change_dynamics_equals_batched_env0():
    from real_robots_amd.envs.env import REALRobotEnv
    from real_robots_amd.mathutil import quat_from_euler
    env = REALRobotEnv(objects=3, eye_width=W, eye_height=H)
    env.reset()
    env._p.changeDynamics(2, -1, lateralFriction=0.2, mass=2.5)
    env._p.changeDynamics(3, -1, restitution=0.4, rollingFriction=0.01, spinningFriction=0.02, localInertiaDiagonal=[1e-3, 1e-3, 5e-4])
    info = env._p.getDynamicsInfo(2, -1)
    assert len(info) == 12 and info[0] == pytest.approx(2.5) and info[1] == pytest.approx(0.2)
    assert info[2] == pytest.approx((0.00153 * 2.5 / 1.5,) * 3, rel=1e-5)
    info3 = env._p.getDynamicsInfo(3, -1)
    assert info3[5] == pytest.approx(0.4) and info3[6] == pytest.approx(0.01) and info3[7] == pytest.approx(0.02)
    for call in (lambda: env._p.changeDynamics(2, -1, linearDamping=0.1), lambda: env._p.changeDynamics(0, -1, mass=1.0),
                 lambda: env._p.changeDynamics(2, 0, mass=1.0), lambda: env._p.getDynamicsInfo(1, -1),
                 lambda: env._p.changeDynamics(2, -1, mass=1.0, contactStiffness=1.0)):
        with pytest.raises(NotImplementedError):
            call()
    be = BatchedREALRobotEnv(1, objects=3, width=W, height=H)
    fac = env._backend()
    be.set_object_dynamics(**fac.object_dynamics())
    be.state = fac.state                              # the facade's start (its reset places the objects itself)
    for i, name in enumerate(env.robot.used_objects[1:]):
        p = env.robot.object_poses[name]
        be.set_object_home(0, i, np.concatenate([p[:3], quat_from_euler(*p[3:])]))
    rng = np.random.default_rng(2)
    for t in range(120):
        a = rng.uniform(env.robot.min_joints, env.robot.max_joints).astype(np.float32)
        env.step({'joint_command': a, 'render': False})
        be.step(a[None])
    assert np.array_equal(fac.state.view(np.uint32), be.state.view(np.uint32))
    env.close()
    be.close()


def test_vector_env_dynamics_randomization():
    from real_robots_amd.vector import REALRobotVectorEnv
    n = 16
    rnd = {'mass': (0.5, 2.0), 'friction': (0.5, 1.5)}
    v1 = REALRobotVectorEnv(n, eye_width=W, eye_height=H, max_episode_steps=5, render_every_step=False, dynamics_randomization=rnd)
    v2 = REALRobotVectorEnv(n, eye_width=W, eye_height=H, max_episode_steps=5, render_every_step=False, dynamics_randomization=rnd)
    _, i1 = v1.reset(seed=123)
    _, i2 = v2.reset(seed=123)
    d1, d2 = i1['object_dynamics'], i2['object_dynamics']
    for k in d1:
        assert np.array_equal(d1[k], d2[k])
    dflt = v1._be.default_object_dynamics()
    for k, (lo, hi) in rnd.items():
        r = d1[k] / dflt[k]
        assert r.min() >= lo * (1 - 1e-6) and r.max() <= hi * (1 + 1e-6)
    r_in = d1['inertia'] / dflt['inertia']
    assert np.allclose(r_in, (d1['mass'] / dflt['mass'])[..., None], rtol=1e-5)     # uniform density
    assert np.array_equal(d1['restitution'], dflt['restitution'])
    assert np.array_equal(v1._be.object_dynamics()['mass'], d1['mass'])
    # autoreset redraws only the truncated envs: stagger the clocks so that half of the envs truncate first
    v1._steps[: n // 2] = 2
    act = np.zeros((n, 9), np.float32)
    for _ in range(2):
        _, _, _, trunc, inf = v1.step(act)
        assert not trunc.any() and 'object_dynamics' not in inf
    _, _, _, trunc, inf = v1.step(act)
    assert trunc[: n // 2].all() and not trunc[n // 2:].any()
    assert np.array_equal(inf['_object_dynamics'], trunc)
    now = v1._be.object_dynamics()
    assert np.array_equal(now['mass'][n // 2:], d1['mass'][n // 2:])
    assert not np.array_equal(now['mass'][: n // 2], d1['mass'][: n // 2])
    assert np.array_equal(inf['object_dynamics']['mass'], now['mass'])
    # without the argument nothing changes
    v3 = REALRobotVectorEnv(4, eye_width=W, eye_height=H, render_every_step=False)
    _, i3 = v3.reset(seed=1)
    assert i3 == {}
    assert np.array_equal(v3._be.object_dynamics()['mass'], v3._be.default_object_dynamics()['mass'])
    for v in (v1, v2, v3):
        v.close()
