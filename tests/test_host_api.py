"""CPU tests (-m "not gpu") of the host layer and the C-ABI boundary (no compute calls: there is no GPU here)."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import real_robots_amd as rr
from real_robots_amd import _native as nat
from real_robots_amd import spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, 'include', 'realrobot.h')).read()
    declared = sorted(set(re.findall(r'\b(rr_[a-z_]+)\s*\(', header)))
    assert declared == sorted(nat.SYMBOLS)
    L = nat.load_library()
    for name in declared:
        assert getattr(L, name) is not None
    assert L.rr_abi_version() == nat.RR_ABI_VERSION


def test_header_is_plain_c_and_a_c_caller_links(tmp_path):
    """include/realrobot.h must be consumable from C99 (the boundary has no C++/torch types) and a C program must link
    against the shared library; the program only calls the two entry points that need no GPU."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'caller.c'
    src.write_text(
        '#include <stdio.h>\n#include "realrobot.h"\n'
        'int main(void) {\n'
        '    rr_config cfg = {0};\n    rr_env *env = NULL;\n'
        '    cfg.abi_version = RR_ABI_VERSION; cfg.num_envs = 0;      /* invalid on purpose */\n'
        '    int rc = rr_create(&cfg, NULL, 0, NULL, &env);\n'
        '    printf("%d %d %s\\n", rr_abi_version(), rc, rr_last_error());\n'
        '    return (rc == RR_EINVAL && env == NULL && sizeof(rr_config) == 80) ? 0 : 1;\n}\n')
    exe = tmp_path / 'caller'
    libdir = os.path.dirname(nat.LIB_PATH)
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe),
                    '-L', libdir, '-l:' + os.path.basename(nat.LIB_PATH), '-Wl,-rpath,' + libdir], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split()[0] == str(nat.RR_ABI_VERSION)


def test_create_rejects_bad_arguments_and_fails_loudly_without_gpu():
    L = nat.load_library()
    blob = nat.model_blob()
    h = C.c_void_p()
    cfg = nat.Config()
    cfg.abi_version, cfg.num_envs, cfg.n_objects, cfg.width, cfg.height = nat.RR_ABI_VERSION, 4, 3, 128, 128
    assert L.rr_create(None, blob, len(blob), None, C.byref(h)) == -1
    bad = nat.Config.from_buffer_copy(cfg)
    bad.n_objects = 5
    assert L.rr_create(C.byref(bad), blob, len(blob), None, C.byref(h)) == -1
    assert b'n_objects' in L.rr_last_error()
    bad = nat.Config.from_buffer_copy(cfg)
    bad.abi_version = 99
    assert L.rr_create(C.byref(bad), blob, len(blob), None, C.byref(h)) == -1
    bad = nat.Config.from_buffer_copy(cfg)
    bad.solver_flags = 4
    assert L.rr_create(C.byref(bad), blob, len(blob), None, C.byref(h)) == -1 and b'solver_flags' in L.rr_last_error()
    bad = nat.Config.from_buffer_copy(cfg)
    bad.motor_kp = float('nan')
    assert L.rr_create(C.byref(bad), blob, len(blob), None, C.byref(h)) == -1 and b'non-finite' in L.rr_last_error()
    assert L.rr_create(C.byref(cfg), b'garbage' * 10, 70, None, C.byref(h)) == -3     # RR_EMODEL
    import torch
    if not torch.cuda.is_available():
        rc = L.rr_create(C.byref(cfg), blob, len(blob), None, C.byref(h))
        assert rc == -2 and b'no CPU fallback' in L.rr_last_error()                 # RR_EDEVICE
        env = rr.make('REALRobot2020-R2J3-v0')
        with pytest.raises(RuntimeError):
            env.reset()


def test_create_image_size_limit_matches_the_tile_rule(monkeypatch):
    """rr_create checks the image size before it looks for a device: a size the tile rule accepts gets past the checks
    (RR_EDEVICE without a GPU, a handle with one), a rejected one returns RR_EINVAL.  Tiles of 4096 pixels, 64 wide above a
    width of 128, at most 255 of them: 1024 x 960 is 16 x 15 = 240 tiles, 1024 x 961 and 1024 x 1020 are 16 x 16 = 256;
    1020 x 64 is 16 tiles, and 255 strips 4 wide under RR_TILE_W=4 -- exactly the last index before the sentinel.  The
    example sizes of the header's rr_config comment are the ones this rule accepts and rejects."""
    L = nat.load_library()
    blob = nat.model_blob()

    def create(W, H):
        cfg = nat.Config()
        cfg.abi_version, cfg.num_envs, cfg.n_objects, cfg.width, cfg.height = nat.RR_ABI_VERSION, 1, 1, W, H
        h = C.c_void_p()
        rc = L.rr_create(C.byref(cfg), blob, len(blob), None, C.byref(h))
        if rc == 0:
            L.rr_destroy(h)
        assert rc in (0, -1, -2), rc
        return rc != -1, L.rr_last_error()

    monkeypatch.delenv('RR_TILE_W', raising=False)
    assert create(1024, 960)[0]
    ok, err = create(1024, 961)
    assert not ok and b'255 raster tiles' in err
    assert not create(1024, 1020)[0]
    assert create(1020, 64)[0]
    monkeypatch.setenv('RR_TILE_W', '4')
    assert create(1020, 64)[0]                    # 255 tiles
    assert not create(1024, 64)[0]                # 256 tiles
    monkeypatch.delenv('RR_TILE_W')
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'realrobot.h')).read()
    fits, fails = re.search(r'\((\d+) x (\d+) fits, (\d+) x (\d+) does not\)', hdr).groups()[:2], \
        re.search(r'\((\d+) x (\d+) fits, (\d+) x (\d+) does not\)', hdr).groups()[2:]
    assert create(*map(int, fits))[0] and not create(*map(int, fails))[0]
    src = open(os.path.join(os.path.dirname(__file__), '..', 'real_robots_amd', 'csrc', 'rr_host.inc')).read()
    assert re.search(r'e\.g\. (\d+) x (\d+) fits, (\d+) x (\d+) does not', src).groups() == fits + fails


def _blob_entries(blob):
    """name -> (byte position of the entry in the table, offset, nbytes): `RRMODEL1`, a u32 count at byte 8, the table at byte 16,
    72 bytes an entry {name[32], dtype, ndim, shape[4], u64 offset, u64 nbytes} (Blob / BlobEntry in rr_host.inc)."""
    import struct
    assert blob[:8] == b'RRMODEL1'
    out = {}
    for i in range(struct.unpack_from('<I', blob, 8)[0]):
        at = 16 + 72 * i
        off, nbytes = struct.unpack_from('<QQ', blob, at + 56)
        out[blob[at:at + 32].split(b'\0')[0].decode()] = (at, off, nbytes)
    return out


def _rename(blob, ent, name):
    blob[ent[name][0]] ^= 0x20               # first letter to upper case: no entry of that name any more


def _halve_nbytes(blob, ent, name):
    import struct
    struct.pack_into('<Q', blob, ent[name][0] + 64, ent[name][2] // 2)


def _set_word(blob, ent, name, index, value):
    import struct
    struct.pack_into('<i', blob, ent[name][1] + 4 * index, value)


@pytest.mark.parametrize('mutate, urdf, word', [
    (lambda b, e: _rename(b, e, 'body_jpos'), 0, b'body_jpos'),
    (lambda b, e: _halve_nbytes(b, e, 'shape_verts'), 0, b'shape_verts'),
    (lambda b, e: _set_word(b, e, 'dims', 0, 10), 0, b'dims'),
    (lambda b, e: _set_word(b, e, 'shape_ne', 0, 49), 0, b'shape_ne'),
    (lambda b, e: _set_word(b, e, 'body_parent', 3, 0), 0, b'kinematic tree'),
    (lambda b, e: _rename(b, e, 'body_inertia_urdf'), 1, b'body_inertia_urdf'),
    (lambda b, e: _rename(b, e, 'body_inertia_urdf'), 0, None),
], ids=['body_jpos-renamed', 'shape_verts-short', 'dims', 'shape_ne', 'body_parent', 'urdf-inertia-missing', 'urdf-inertia-unused'])
def test_create_reports_a_malformed_model_before_it_looks_for_a_device(mutate, urdf, word):
    """The model is parsed on the host before rr_create touches the device: a malformed blob returns RR_EMODEL with the
    blob entry in the message and a null handle on any machine.  The last case is a valid model for its config (the
    entry it lacks is not read): past the model checks, RR_EDEVICE without a GPU, a handle with one."""
    L = nat.load_library()
    blob = bytearray(nat.model_blob())
    mutate(blob, _blob_entries(blob))
    cfg = nat.Config()
    cfg.abi_version, cfg.num_envs, cfg.n_objects, cfg.width, cfg.height = nat.RR_ABI_VERSION, 1, 1, 64, 64
    cfg.use_urdf_inertia = urdf
    h = C.c_void_p(0xdead)
    rc = L.rr_create(C.byref(cfg), bytes(blob), len(blob), None, C.byref(h))
    if word is not None:
        assert rc == -3 and word in L.rr_last_error(), (rc, L.rr_last_error())      # RR_EMODEL
        assert not h.value
        return
    import torch
    if torch.cuda.is_available():
        assert rc == 0 and h.value, (rc, L.rr_last_error())
        assert L.rr_destroy(h) == 0
    else:
        assert rc == -2 and b'no CPU fallback' in L.rr_last_error() and not h.value, (rc, L.rr_last_error())


def test_settings_reader_and_integration_table_name_the_same_variables():
    """Every RR_* variable the library reads is read in one place, once, and INTEGRATION.md's table documents exactly those
    (plus the ones the Python side reads)."""
    src = open(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_host.inc')).read()
    read = re.findall(r'getenv\("(RR_[A-Z0-9_]+)"\)', src)
    assert len(read) == len(set(read)) > 0, sorted(read)
    for inc in os.listdir(os.path.join(ROOT, 'real_robots_amd', 'csrc')):
        if inc.endswith(('.inc', '.hip')) and inc != 'rr_host.inc':
            assert 'getenv' not in open(os.path.join(ROOT, 'real_robots_amd', 'csrc', inc)).read(), inc
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    table = doc[doc.index('## Environment variables'):]
    documented = set()
    for row in table.splitlines():
        if row.startswith('| `RR_'):
            documented |= set(re.findall(r'`(RR_[A-Z0-9_]+)', row.split('|')[1]))
    assert set(read) == documented - {'RR_LIB', 'RR_MODEL', 'RR_NO_TORCH_PRELOAD'}


def test_solver_dict_reaches_the_config_struct():
    """ABI 6: the constants the reference leaves to pybullet's defaults travel in rr_config (same 80 bytes as ABI 5's reserved
    words); 0 = default, an explicit zero is passed as the header's "literal zero" (negative)."""
    assert C.sizeof(nat.Config) == 80
    cfg = nat.Config()
    nat.apply_solver(cfg, None)
    assert cfg.motor_kp == 0 and cfg.solver_flags == 0
    nat.apply_solver(cfg, {'motor_kp': 0.5, 'warmstart': 0.0, 'rate_limit': False, 'erp': 0.3})
    assert abs(cfg.motor_kp - 0.5) < 1e-7 and cfg.warmstart < 0 and cfg.solver_flags == nat.SOLVER_NO_RATE_LIMIT and abs(cfg.erp - 0.3) < 1e-7
    nat.apply_solver(cfg, {'rate_limit': True})
    assert cfg.solver_flags == 0
    for bad in ({'kp': 1}, {'motor_kd': -0.1}, {'lin_damping': float('inf')}, {'erp': 0}):
        with pytest.raises(ValueError):
            nat.apply_solver(nat.Config(), bad)
    env = rr.make('REALRobot2020-R2J1-v0', solver={'motor_kp': 0.5})
    assert env._solver == {'motor_kp': 0.5}


def test_null_env_calls_return_einval():
    L = nat.load_library()
    assert L.rr_step(None, None, 0, 0, None) == -1
    assert L.rr_reset(None, None) == -1
    assert L.rr_render(None) == -1
    assert L.rr_sync(None) == -1
    assert L.rr_destroy(None) == 0


def test_registry_has_the_18_reference_ids():
    ids = rr.registered_ids()
    assert len(ids) == 18
    for rnd in ('R1', 'R2'):
        for a in 'JCM':
            for n in (1, 2, 3):
                assert 'REALRobot2020-%s%s%d-v0' % (rnd, a, n) in ids
    with pytest.raises(KeyError):
        rr.make('REALRobot-v0')


def test_env_spaces_and_constructor_contract():
    env = rr.make('REALRobot2020-R1M2-v0')
    assert env.robot.used_objects == ['table', 'cube', 'tomato']
    assert set(env.action_space.spaces) == {'macro_action', 'render'}
    assert env.macro_space.shape == (2, 2)
    assert set(env.observation_space.spaces) == {'joint_positions', 'touch_sensors', 'retina', 'depth', 'goal', 'mask',
                                                 'goal_mask', 'object_positions', 'goal_positions'}
    assert env.observation_space.spaces['retina'].shape == (240, 320, 3)
    env2 = rr.make('REALRobot2020-R2J3-v0')
    assert set(env2.observation_space.spaces) == {'joint_positions', 'touch_sensors', 'retina', 'depth', 'goal'}
    a = env2.action_space.sample()
    assert a['joint_command'].shape == (9,) and env2.joints_space.contains(a['joint_command'])
    lim = env2.robot.max_joints
    assert np.allclose(lim[[0, 1, 2, 6, 7]], [0.666 * np.pi, 0.666 * np.pi, 0.944 * np.pi, 0.972 * np.pi, np.pi / 2])
    assert (env2.intrinsic_timesteps, env2.extrinsic_timesteps, env2.extrinsic_trials) == (int(15e6), int(10e3), 50)
    assert env2.goal_idx == -1 and (env2.goal.retina == 0).all()
    # minor API of the reference env: eye cameras, the debug camera factory, the earlier rounds' score formula, `_p`
    from real_robots_amd.envs import EyeCamera
    assert isinstance(env2.eyes['eye'], EyeCamera) and env2.eyes['eye'].eyePosition == [0.01, 0, 1.2]
    env2.set_eye('side', eye_pos=[0.5, 0.5, 0.8], target_pos=[0, 0, 0.3])
    assert set(env2.eyes) == {'eye', 'side'}
    env2.setCamera()
    assert abs(env2.extrinsicFormula(np.zeros(3), np.array([0.05, 0, 0]), np.array([0, 0, 0, 1.0]), np.array([0, 0, 0, 1.0])) - 0.25) < 1e-12
    assert np.allclose(env2._p.getEulerFromQuaternion(env2._p.getQuaternionFromEuler([0.1, -0.2, 0.3])), [0.1, -0.2, 0.3])
    with pytest.raises(ValueError):
        rr.REALRobotEnv(action_type='teleport')
    with pytest.raises(AssertionError):
        env2.set_goals_dataset_path('/nonexistent/goals.npz')


def test_evaluate_argument_checks():
    class P(rr.BasePolicy):
        def step(self, o, r, d):
            return {'joint_command': np.zeros(9), 'render': False}
    for kw in (dict(environment='R3'), dict(environment='R2', action_type='macro_action'), dict(action_type='fly'),
               dict(n_objects=4)):
        with pytest.raises(Exception):
            rr.evaluate(P, goals_dataset_path=__file__, **kw)
    with pytest.raises(Exception):
        rr.evaluate(object, environment='R2', action_type='joints', goals_dataset_path=__file__)
    with pytest.raises(NotImplementedError):
        rr.BasePolicy(None, None).step(None, 0, False)


def test_goal_dataset_format_roundtrip(tmp_path):
    """np.savez_compressed(path, list_of_goals) / np.load(allow_pickle) of Goal objects (env.py:143-145)."""
    from real_robots_amd.envs import Goal
    g = Goal(initial_state={'cube': np.arange(7.0)}, final_state={'cube': np.ones(7)}, retina=np.zeros((4, 4, 3), np.uint8),
             challenge='2D', mask=np.zeros((4, 4), np.int32))
    path = str(tmp_path / 'goals.npy.npz')
    np.savez_compressed(path, np.array([g, g], dtype=object))
    env = rr.make('REALRobot2020-R1J1-v0')
    env.set_goals_dataset_path(path)
    env.load_goals()
    assert len(env.goals) == 2 and env.goals[0].challenge == '2D'
    assert pickle.loads(pickle.dumps(g)).final_state['cube'].shape == (7,)


def test_saved_goals_pickle_under_the_reference_module_path(tmp_path):
    """A dataset written here must load where only the reference package exists: the Goal class pickles as
    real_robots.envs.env.Goal (env.py:15-24; generate_goals.py:435-436), not under real_robots_amd."""
    from real_robots_amd.envs.env import Goal
    from real_robots_amd.generate_goals import save_goals
    g = Goal(initial_state={'cube': np.arange(7.0)}, final_state={'cube': np.ones(7)}, retina=np.zeros((2, 2, 3), np.uint8),
             challenge='2D', mask=np.zeros((2, 2), np.int32))
    path = str(tmp_path / 'goals.npy')
    save_goals(path, [g])
    raw = pickle.dumps(g, protocol=2)
    assert b'real_robots.envs.env' in raw and b'real_robots_amd' not in raw
    arr = np.load(path + '.npz', allow_pickle=True)
    assert list(arr.items())[0][1][0].challenge == '2D'
    import real_robots.envs.env as ref_path
    assert ref_path.Goal is Goal


def test_spaces_standins():
    b = spaces.Box(low=np.zeros(3), high=np.ones(3), dtype=float)
    assert b.contains(b.sample()) and not b.contains(np.array([2.0, 0, 0]))
    d = spaces.Dict({'a': b, 'r': spaces.MultiBinary(1)})
    s = d.sample()
    assert set(s) == {'a', 'r'} and d.contains(s)


def test_model_blob_and_ik():
    from oracle.kinematics import EE_LINK, inverse_kinematics, link_pose, quat_from_euler
    from real_robots_amd.model import load_model
    m = load_model()
    assert tuple(m['dims'][:4]) == (11, 17, 22, 22)
    assert abs(float(m['body_mass'].sum()) - 27.5) < 1e-4          # SURVEY A.2 total mass
    q = inverse_kinematics(np.zeros(11), [0.0, 0.2, 0.5], quat_from_euler(0, 3.14, -1.57))
    assert np.linalg.norm(link_pose(q, EE_LINK)[1] - [0.0, 0.2, 0.5]) < 2e-3


def test_shard_ranges_partition_and_actions_are_shard_invariant():
    from real_robots_amd.distributed import shard_range, shard_of, synthetic_actions
    for total, world in ((4096, 8), (10, 3), (7, 8)):
        covered = []
        for r in range(world):
            a, b = shard_range(total, r, world)
            covered += list(range(a, b))
        assert covered == list(range(total))
    assert shard_of(5, 10, 3) == (1, 1)
    full = synthetic_actions(range(16), step=7)
    a, b = shard_range(16, 1, 2)
    assert (synthetic_actions(range(a, b), step=7) == full[a:b]).all()
    assert (synthetic_actions(range(16), step=8) == full).sum() > 0      # held
    assert not (synthetic_actions(range(16), step=60) == full).all()     # resampled


def test_pybullet_harness_imports_without_pybullet_and_mirrors_the_protocol_constants():
    """oracle/pybullet_ref.py is the route to `cpu_baseline.kind = "reference"` and to golden vectors from a real
    PyBullet; here (no pybullet) it must import, report unavailable, refuse loudly -- and its protocol constants must be
    the ones the compiled model carries."""
    from oracle import pybullet_ref as pr
    from real_robots_amd.model import load_model
    m = load_model()
    lo, hi = pr.joint_limits()
    assert np.allclose(lo, m['act_min'], atol=1e-6) and np.allclose(hi, m['act_max'], atol=1e-6)
    assert np.allclose(pr.MAX_DIFF, m['act_maxdiff'], atol=1e-7)
    assert np.allclose(pr.ROBOT_POSITION, m['robot_pos'], atol=1e-7)
    for k, name in enumerate(pr.OBJECTS):
        assert np.allclose(pr.OBJECT_POSES[name][:3], m['obj_pose0'][k][:3], atol=1e-6)
    assert len(pr.perimeter_pairs()) == 36 and pr.seeded_actions(3, 5).shape == (5, 9)
    if not pr.available():
        with pytest.raises(pr.PyBulletUnavailable):
            pr.PyBulletRef()
        with pytest.raises(pr.PyBulletUnavailable):
            pr.cpu_baseline(seconds=0.1)
    else:                                  # a box with pybullet: the harness must at least reset and step
        ref = pr.PyBulletRef(1, 64, 64)
        ref.step(np.zeros(9))
        assert ref.state61().shape == (61,)
        ref.close()


def test_dlpack_capsule_lifecycle_without_a_gpu():
    """DeviceBuffer.__dlpack__ builds a DLManagedTensor by hand (ctypes): kDLROCM device, compact row-major shape, and the
    bookkeeping entry that keeps the struct alive goes away when an unconsumed capsule is dropped."""
    import gc

    class Owner:
        device = 3
    b = nat.DeviceBuffer(0x1000, (4, 9), '<f4', Owner())
    assert b.__dlpack_device__() == (nat.KDL_ROCM, 3)
    n0 = len(nat._dl_alive)
    cap = b.__dlpack__()
    assert len(nat._dl_alive) == n0 + 1
    m = next(iter(nat._dl_alive.values()))[0]
    assert m.dl_tensor.ndim == 2 and [m.dl_tensor.shape[i] for i in range(2)] == [4, 9]
    assert (m.dl_tensor.dtype.code, m.dl_tensor.dtype.bits) == (2, 32) and m.dl_tensor.data == 0x1000
    del cap, m
    gc.collect()
    assert len(nat._dl_alive) == n0


def test_bench_bookkeeping_and_committed_profiles():
    """bench.py's accounting without a GPU: the algorithmic bytes of SURVEY 8(d) (state + command + low-dim observation,
    128x128 RGB + depth), the rule that a committed PMC profile is only attached to a run of the configuration it was
    collected on, and the committed `*_latest.json` files themselves (per-step bytes below the algorithmic image bytes: the
    images persist in HBM and a frame rewrites only what changed)."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.algo_bytes(3, 128, 128)
    assert a['_state'] == (22 + 39 + 11) * 8 + 36 + (9 + 4 + 21) * 4 == 748
    assert a['_image'] == 128 * 128 * 7 + 22 * 12 * 4 == 115744
    cfg = {"envs": 4096, "objects": 3, "width": 128, "height": 128, "render": True, "command_scale": 1.0, "solver_iters": 50}
    # a profile is quoted only for the configuration AND the kernel source it was collected on (recorded hash of realrobot.hip)
    recorded = json.load(open(os.path.join(ROOT, 'profiles', 'traffic_latest.json'))).get('source_sha256')
    real_hash = bench.kernel_source_hash
    bench.kernel_source_hash = lambda: recorded
    prof, why = bench.load_profile('traffic_latest.json', cfg)
    assert prof is not None and why is None and prof['config'] == cfg
    other, why = bench.load_profile('traffic_latest.json', dict(cfg, envs=1024))
    assert other is None and 'collected on' in why
    bench.kernel_source_hash = lambda: 'another build'
    stale, why = bench.load_profile('traffic_latest.json', cfg)
    assert stale is None and 'stale profile' in why
    bench.kernel_source_hash = real_hash
    assert len(real_hash()) == 64
    assert bench.load_profile('no_such_file.json', cfg)[0] is None
    bench.kernel_source_hash = lambda: recorded
    # the committed figures: every kernel of the step is there, the render stage stays below a full image write
    for k in ('k_prep_a16', 'k_prep_b16', 'k_prep_ab16', 'k_prep', 'k_collide', 'k_solve', 'k_render_setup', 'k_raster', 'k_shade', 'render_stage'):
        assert prof[k] > 0, k
    assert prof['render_stage'] < a['_image'] * 4096 and prof['k_solve'] < 100e6
    sq, _ = bench.load_profile('sq_latest.json', cfg)
    bench.kernel_source_hash = real_hash
    assert sq['valu_wave_instr_per_launch']['k_raster'] > 1e8
    assert os.path.exists(os.path.join(ROOT, 'profiles', prof['source'])) and os.path.exists(os.path.join(ROOT, 'profiles', sq['source']))
    assert bench.SIDE_STREAM_KERNELS == ('k_solve_heavy', 'render_heavy') and set(bench.SIDE_STREAM_KERNELS) <= set(nat_names())


def nat_names():
    from real_robots_amd import _native as nat
    assert len(nat.KERNEL_NAMES) == nat.NUM_KERNELS == 9
    return nat.KERNEL_NAMES


def test_product_package_never_imports_the_oracle():
    """oracle/ is test infrastructure: no module of the product package may import it (statically), and importing the whole
    product -- facade, evaluate, goal generator, vector adapter, CLI -- must not pull it in (dynamically).  The IK / plan
    checker lives in oracle/kinematics.py; the product plans on the device."""
    import ast
    import glob
    import subprocess
    import sys
    pkg = os.path.join(ROOT, 'real_robots_amd')
    for path in glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True):
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            mods = []
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom) and node.level == 0:
                mods = [node.module or '']
            assert not any(m == 'oracle' or m.startswith('oracle.') for m in mods), path
    assert not os.path.exists(os.path.join(pkg, 'kinematics.py'))
    code = ("import sys; import real_robots_amd, real_robots_amd.evaluate, real_robots_amd.generate_goals, real_robots_amd.vector, "
            "real_robots_amd.cli, real_robots_amd.envs.env, real_robots; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'")
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


def test_goal_generator_distance_predicate():
    """generate_goals.py:296-313: some pair of objects no farther apart than max_objects_dist."""
    from real_robots_amd.generate_goals import two_near_objects
    p = np.array([[0.0, 0.0, 0.3], [0.25, 0.0, 0.3], [0.0, 0.5, 0.3]])
    assert two_near_objects(p, 0.25) and not two_near_objects(p, 0.2) and not two_near_objects(p[:1], 10.0)
