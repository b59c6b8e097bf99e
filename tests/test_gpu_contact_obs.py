"""GPU tests (-m gpu) of the whole-batch contact observations (rr_contact_observations, include/realrobot.h): the three device
fields against what rr_get_contacts returns one env at a time -- records bit for bit -- and against the independent sequential
float32 restatement of the body rows (tests/numpy_contacts.py), bit for bit; the max column of the skin rows against
RR_F_TOUCH; and that the call has no effect on the simulation."""
import ctypes as C

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.model import load_model
from tests import numpy_contacts as nc

pytestmark = pytest.mark.gpu

NL = len(nat.LINK_NAMES)
TOUCH_ROWS = [nat.LINK_NAMES.index(n) for n in ('skin_00', 'skin_01', 'skin_10', 'skin_11')]      # the order of RR_F_TOUCH
U = np.uint32


def _bits(a):
    return np.ascontiguousarray(a).view(U)


def _check(env, where):
    """One call, every env: records == rr_get_contacts bit for bit and zero beyond, count == RR_F_CONTACT_COUNT, body rows ==
    the numpy restatement bit for bit, skin maxima == RR_F_TOUCH for the envs without an error flag.  Returns the host copies."""
    co = env.contact_observations(host=True)
    lists = [env.contacts(i) for i in range(env.N)]
    assert co['contacts'].shape == (env.N, 48, 12) and co['body_force'].shape == (env.N, 20, 2) and co['body_partners'].shape == (env.N, 20)
    assert (co['count'] == env.host(nat.F_CONTACT_COUNT)).all(), where
    for i, rows in enumerate(lists):
        k = len(rows)
        assert k == co['count'][i], (where, i, k, co['count'][i])
        assert (_bits(co['contacts'][i, :k]) == _bits(rows)).all(), (where, i, 'records')
        assert not _bits(co['contacts'][i, k:]).any(), (where, i, 'rows beyond the count')
    force, partners = nc.body_rows(lists, n_links=NL)
    assert (_bits(co['body_force']) == _bits(force)).all(), (where, 'body_force', co['body_force'], force)
    assert (co['body_partners'] == partners).all(), (where, 'body_partners', co['body_partners'], partners)
    ok = env.host(nat.F_ERRFLAGS) == 0
    touch = env.host(nat.F_TOUCH)
    assert (_bits(co['body_force'][ok][:, TOUCH_ROWS, 0]) == _bits(touch[ok])).all(), (where, 'touch', touch)
    return co


def _grasp_script():
    """The grasp of tests/test_gpu_contacts_fuzz.py, restated: above the cube with open fingers, down, close."""
    from oracle.kinematics import inverse_kinematics, quat_from_euler
    orient = quat_from_euler(0, 3.14, -1.57)
    q_hi = inverse_kinematics(np.zeros(11), [-0.1, 0.0, 0.55], orient)
    q_lo = inverse_kinematics(q_hi, [-0.1, 0.0, 0.47], orient)
    cmds = []
    for q, g, n in [(q_hi, [0.5, 0.0], 150), (q_lo, [0.5, 0.0], 120), (q_lo, [0.0, 0.0], 60)]:
        cmds += [np.concatenate([q[:7], g])] * n
    return np.array(cmds, np.float32)


def test_touch_rows_are_the_models_touch_links():
    assert list(np.array(load_model()['touch_links'])) == TOUCH_ROWS


def test_empty_after_reset_and_resting_objects():
    """N = 3 (less than one workgroup of envs: the env < N guard): all zero after reset; after 100 idle steps the object rests on
    the table -- its row carries bit 0 and a positive sum, the robot's rows stay zero."""
    env = BatchedREALRobotEnv(3, objects=1, width=64, height=64)
    env.reset()
    co = _check(env, 'reset')
    assert not co['count'].any() and not _bits(co['contacts']).any() and not _bits(co['body_force']).any() and not co['body_partners'].any()
    for _ in range(100):
        env.step(None)
    co = _check(env, 'rest')
    assert (co['body_partners'][:, NL] == 1).all() and (co['body_force'][:, NL, 1] > 0).all() and (co['count'] > 0).all()
    assert (co['body_force'][:, NL, 0] <= co['body_force'][:, NL, 1]).all()
    assert not _bits(co['body_force'][:, :NL]).any() and not co['body_partners'][:, :NL].any()
    assert not _bits(co['body_force'][:, NL + 1:]).any() and not co['body_partners'][:, NL + 1:].any()      # objects the handle does not have
    assert env.body_row_names() == list(nat.LINK_NAMES) + ['cube']
    env.close()


def test_grasp_records_rows_and_touch():
    env = BatchedREALRobotEnv(4, objects=1, width=64, height=64)
    for _ in range(100):
        env.step(None)
    skin_pairs = 0
    for t, c in enumerate(_grasp_script()):
        env.step(np.tile(c, (4, 1)))
        if t >= 262 and t % 2 == 0:
            co = _check(env, ('grasp', t))
            skin = (co['body_force'][:, TOUCH_ROWS, 0] > 0).any(-1)
            skin_pairs += int(skin.sum())
            # a skin that touches the cube: the cube's row has the robot's bit
            on_cube = ((co['body_partners'][:, TOUCH_ROWS] & 2) != 0).any(-1)
            assert ((co['body_partners'][on_cube, NL] & 16) != 0).all()
            assert (co['body_partners'][:, :NL] & 16 == 0).all()             # no robot body is ever body B
    assert skin_pairs >= 20, skin_pairs
    env.close()


def test_push_many_contacts():
    """N = 34 (no multiple of any block shape), three objects, macro pushes: every 20th step from 200 on, every env."""
    N = 34
    env = BatchedREALRobotEnv(N, objects=3, width=64, height=64)
    rng = np.random.default_rng(5)
    env.plan_macro(rng.uniform([-0.25, -0.5], [0.05, 0.5], size=(N, 2, 2)))
    many = 0
    for t in range(761):
        env.step_plan(render=False)
        if t >= 200 and t % 20 == 0:
            co = _check(env, ('push', t))
            many += int(((co['count'] > 16) & (env.host(nat.F_ENV_CLASS) >= 1)).sum())
    assert many >= 1, many
    env.close()


def _rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _hull(obj):
    m = load_model()
    own, nv = np.array(m['shape_owner']), np.array(m['shape_nv'])
    s = [s for s in range(len(own)) if own[s][0] == 2 and own[s][1] == obj][0]
    return np.array(m['shape_verts'][s][:nv[s]], np.float64)


def test_object_beside_object_feeds_two_rows():
    """Object 1 is put beside object 0 on the table, along -y, with a gap between the hulls' extents of 5 mm (env 0) and 10 mm
    (env 1) -- inside the 0.02 contact margin; env 2 is left alone.  After one step rows 17 and 18 of envs 0 and 1 carry each
    other's bit, those of env 2 do not."""
    env = BatchedREALRobotEnv(3, objects=3, width=64, height=64)
    for _ in range(100):
        env.step(None)
    poses = env.host(nat.F_OBJ_POSE)
    for i, gap in ((0, 0.005), (1, 0.010)):
        p0, q0, q1 = poses[i, 0, :3].astype(np.float64), poses[i, 0, 3:], poses[i, 1, 3:]
        e0 = (-(_hull(0) @ _rot(q0).T)[:, 1]).max()          # object 0's extent towards -y
        e1 = ((_hull(1) @ _rot(q1).T)[:, 1]).max()           # object 1's extent towards +y
        poses[i, 1, :3] = (p0[0], p0[1] - (e0 + gap + e1), poses[i, 1, 2])
    env.set_object_poses(poses)
    env.step(None)
    co = _check(env, 'beside')
    p = co['body_partners']
    assert ((p[:2, NL] & 0b100) != 0).all() and ((p[:2, NL + 1] & 0b010) != 0).all(), p[:, NL:]
    assert (p[:2, NL:NL + 2] & 1 == 1).all()                 # both still rest on the table
    assert p[2, NL] == 1 and p[2, NL + 1] == 1 and p[2, NL + 2] == 1, p[2]
    env.close()


def test_refused_command_gives_zero_rows():
    env = BatchedREALRobotEnv(3, objects=1, width=64, height=64)
    for _ in range(100):
        env.step(None)
    assert (_check(env, 'before')['body_partners'][:, NL] == 1).all()
    cmd = np.zeros((3, 9), np.float32)
    cmd[1, 3] = np.nan
    nat.check(env.L.rr_step(env.h, cmd.ctypes.data, 0, 0, None))      # (BatchedREALRobotEnv.step asserts finite commands: robot.py:189)
    assert list(env.host(nat.F_ERRFLAGS) & 2) == [0, 2, 0]
    co = _check(env, 'refused')
    assert co['count'][1] == 0 and not _bits(co['contacts'][1]).any() and not _bits(co['body_force'][1]).any() and not co['body_partners'][1].any()
    assert (co['body_partners'][[0, 2], NL] == 1).all() and (co['body_force'][[0, 2], NL, 1] > 0).all()
    env.close()


def test_no_side_effects_and_fields_keep_the_last_call():
    """Two handles run the grasp for 300 steps; one calls contact_observations() after every step, the other never: state, touch
    and a checkpoint are bit-identical.  The fields hold what the last CALL computed: a later step does not refresh them."""
    a = BatchedREALRobotEnv(4, objects=1, width=64, height=64)
    b = BatchedREALRobotEnv(4, objects=1, width=64, height=64)
    cmds = _grasp_script()
    for c in cmds[:300]:
        for e in (a, b):
            e.step(np.tile(c, (4, 1)))
        a.contact_observations()
    assert (_bits(a.host(nat.F_STATE)) == _bits(b.host(nat.F_STATE))).all()
    assert (_bits(a.host(nat.F_TOUCH)) == _bits(b.host(nat.F_TOUCH))).all()
    assert (a.checkpoint() == b.checkpoint()).all()
    then = a.contact_observations(host=True)
    assert then['count'].any() and _bits(then['body_force']).any()
    # the fingers go on closing: the later steps' lists differ, the fields do not follow them until the next call
    for c in cmds[300:]:
        a.step(np.tile(c, (4, 1)))
    for f, k in ((nat.F_CONTACTS, 'contacts'), (nat.F_BODY_FORCE, 'body_force'), (nat.F_BODY_PARTNERS, 'body_partners')):
        assert (_bits(a.host(f)) == _bits(then[k])).all(), k
    now = a.contact_observations(host=True)
    assert not (_bits(now['contacts']) == _bits(then['contacts'])).all()
    # the device views are the same storage over calls and steps
    p1, p2 = a.device_buffer(nat.F_BODY_FORCE).ptr, a.contact_observations()['body_force'].ptr
    assert p1 == p2 and p1
    a.close()
    b.close()


def test_fields_are_allocated_and_zero_before_the_first_call():
    env = BatchedREALRobotEnv(3, objects=2, width=64, height=64)
    for _ in range(60):
        env.step(None)
    p, n = C.c_void_p(), C.c_size_t()
    nat.check(env.L.rr_get_buffer(env.h, nat.F_BODY_PARTNERS, C.byref(p), C.byref(n)))
    assert p.value and n.value == 3 * 20 * 4
    assert not _bits(env.host(nat.F_CONTACTS)).any() and not _bits(env.host(nat.F_BODY_FORCE)).any() and not env.host(nat.F_BODY_PARTNERS).any()
    co = _check(env, 'first call')
    assert (co['body_partners'][:, NL:NL + 2] == 1).all() and not co['body_partners'][:, NL + 2].any()
    env.close()


def test_vector_env_contact_obs():
    from real_robots_amd.envs.robot import Kuka
    from real_robots_amd.vector import REALRobotVectorEnv
    kw = dict(objects=1, eye_width=64, eye_height=64, render_every_step=False, max_episode_steps=60)
    base = Kuka(False, 1, 64, 64, env=None).observation_space
    plain = REALRobotVectorEnv(3, **kw)
    obs, _ = plain.reset(seed=0)
    assert set(obs) == {'joint_positions', 'touch_sensors'}
    assert set(plain.single_observation_space.spaces) == set(base.spaces) == set(plain.observation_space.spaces)
    assert 'body_force' not in plain.observation_space.spaces
    plain.close()
    v = REALRobotVectorEnv(3, contact_obs=True, **kw)
    assert set(v.single_observation_space.spaces) == set(base.spaces) | {'body_force', 'body_partners'}
    assert v.single_observation_space['body_force'].shape == (20, 2) and v.observation_space['body_force'].shape == (3, 20, 2)
    assert v.single_observation_space['body_partners'].shape == (20,) and v.observation_space['body_partners'].shape == (3, 20)
    assert v.observation_space['body_force'].dtype == np.float32 and v.observation_space['body_partners'].dtype == np.uint32
    obs, _ = v.reset(seed=0)
    assert obs['body_force'].shape == (3, 20, 2) and obs['body_force'].dtype == np.float32 and not obs['body_force'].any()
    assert obs['body_partners'].shape == (3, 20) and obs['body_partners'].dtype == np.uint32 and not obs['body_partners'].any()
    for t in range(59):
        obs, _, _, trunc, _ = v.step(np.zeros((3, 9), np.float32))
    assert not trunc.any() and (obs['body_partners'][:, NL] == 1).all() and (obs['body_force'][:, NL, 1] > 0).all()
    f, p = nc.body_rows([v._be.contacts(i) for i in range(3)], n_links=NL)
    assert (_bits(obs['body_force']) == _bits(f)).all() and (obs['body_partners'] == p).all()
    assert v.observation_space['body_force'].contains(obs['body_force'])
    # the same-step autoreset: the entries describe the reset state, like the others
    obs, _, _, trunc, infos = v.step(np.zeros((3, 9), np.float32))
    assert trunc.all() and not obs['body_force'].any() and not obs['body_partners'].any()
    v.close()
    d = REALRobotVectorEnv(3, contact_obs=True, device_obs=True, **kw)
    obs, _ = d.reset(seed=0)
    assert obs['body_force'].shape == (3, 20, 2) and obs['body_force'].typestr == np.dtype(np.float32).str and obs['body_force'].ptr
    assert obs['body_partners'].shape == (3, 20) and obs['body_partners'].typestr == np.dtype(np.uint32).str
    d.close()
