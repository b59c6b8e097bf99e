"""BatchedREALRobotEnv: N independent REALRobot envs stepped in lock-step on one MI355X.

Host-side mirror of the reference's step protocol for a batch (REALRobotEnv.step_joints, env.py:326-356;
Kuka.apply_action/calc_state/get_touch_sensors, robot.py:152-211), implemented by librealrobot_hip.so.
Observations stay on the device; `obs_host()` copies what the caller asks for.
"""
import ctypes as C

import numpy as np

from . import _native as nat

OBJECT_NAMES = ['cube', 'tomato', 'mustard']       # robot.py:49-50 (after "table")


def _env_mask(env_mask, N):
    """env_mask of a per-env setter -> (uint8 [N] or None, its address or None); a wrong shape raises ValueError."""
    if env_mask is None:
        return None, None
    m = np.ascontiguousarray(env_mask).astype(np.uint8)
    if m.shape != (N,):
        raise ValueError("env_mask must have shape (%d,)" % N)
    return m, m.ctypes.data


def _on_device(a):
    """a CUDA torch tensor or an object with `__cuda_array_interface__`"""
    if hasattr(a, 'is_cuda') and hasattr(a, 'data_ptr'):
        return bool(a.is_cuda)
    return getattr(a, '__cuda_array_interface__', None) is not None


def _float32_arg(v, name, shape, nonneg=False):
    """v broadcast to float32 `shape`; a shape that does not broadcast, a value that is not finite in float32 or (nonneg)
    a negative one raises ValueError naming the field."""
    try:
        with np.errstate(over='ignore'):
            a = np.broadcast_to(np.asarray(v, dtype=np.float64).astype(np.float32), shape)
    except (ValueError, TypeError):
        raise ValueError("%s: cannot broadcast an array of shape %s to %s" % (name, np.shape(v), shape))
    if not np.isfinite(a).all() or (nonneg and (a < 0).any()):
        raise ValueError("%s must be finite (in float32)%s" % (name, " and >= 0" if nonneg else ""))
    return np.ascontiguousarray(a)


class BatchedREALRobotEnv:
    def __init__(self, num_envs, objects=3, width=320, height=240, device=0, solver_iters=50, envs_per_block=0,
                 stream=None, use_urdf_inertia=False, dt=0.0, erp=0.0, margin=0.0, want_mask=True, solver=None):
        """solver: dict overriding the constants the reference leaves to pybullet's defaults (keys of `_native.SOLVER_DEFAULTS`:
        motor_kp 0.1, motor_kd 1.0, motor_max_force 100000, warmstart 0.85, lin_damping / ang_damping 0.04, erp 0.2, rate_limit
        True -- robot.py:196-201, env.py:202-204, 314-321)."""
        self.L = nat.load_library()
        cfg = nat.Config()
        cfg.abi_version = nat.RR_ABI_VERSION
        cfg.num_envs, cfg.n_objects, cfg.width, cfg.height = int(num_envs), int(objects), int(width), int(height)
        cfg.device, cfg.solver_iters, cfg.envs_per_block = int(device), int(solver_iters), int(envs_per_block)
        cfg.dt, cfg.erp, cfg.margin, cfg.use_urdf_inertia = dt, erp, margin, int(bool(use_urdf_inertia))
        cfg.flags = 0 if want_mask else nat.FLAG_NO_MASK
        nat.apply_solver(cfg, solver)
        self.solver = dict(nat.SOLVER_DEFAULTS, **({'erp': erp} if erp > 0 else {}), **(solver or {}))
        blob = nat.model_blob()
        h = C.c_void_p()
        self.h = None
        nat.check(self.L.rr_create(C.byref(cfg), blob, len(blob), C.c_void_p(stream or 0), C.byref(h)))
        self.h = h
        self.N, self.n_objects, self.W, self.H, self.device = int(num_envs), int(objects), int(width), int(height), int(device)
        self.object_names = OBJECT_NAMES[:self.n_objects]
        self._shapes = {
            nat.F_JOINTS: ((self.N, 9), np.float32), nat.F_TOUCH: ((self.N, 4), np.float32),
            nat.F_OBJ_POSE: ((self.N, self.n_objects, 7), np.float32),
            nat.F_RGB: ((self.N, self.H, self.W, 3), np.uint8), nat.F_DEPTH: ((self.N, self.H, self.W), np.float32),
            nat.F_MASK: ((self.N, self.H, self.W), np.int32), nat.F_TIMESTEP: ((self.N,), np.int32),
            nat.F_ERRFLAGS: ((self.N,), np.uint32), nat.F_STATE: ((self.N, 61), np.float32),
            nat.F_FRAG_COUNT: ((self.N, 1), np.uint32), nat.F_CONTACT_COUNT: ((self.N,), np.int32),
            nat.F_ENV_CLASS: ((self.N,), np.int32), nat.F_PREP: ((self.N, nat.PREP_FLOATS), np.float32),
            nat.F_CONTACTS: ((self.N, nat.MAX_CONTACTS, 12), np.float32),
            nat.F_BODY_FORCE: ((self.N, nat.CONTACT_ROWS, 2), np.float32), nat.F_BODY_PARTNERS: ((self.N, nat.CONTACT_ROWS), np.uint32)}
        p_, n_ = C.c_void_p(), C.c_size_t()                  # the tile count is the library's choice: ask for it
        nat.check(self.L.rr_get_buffer(self.h, nat.F_FRAG_COUNT, C.byref(p_), C.byref(n_)))
        self._shapes[nat.F_FRAG_COUNT] = ((self.N, max(1, n_.value // (4 * self.N))), np.uint32)
        self._dyn_default = self._dynamics_raw()           # a fresh handle holds the model's object dynamics
        self._app_default = self.env_appearance()          # ... and the model's appearance
        self._act_default = self._actuators_raw()          # ... and the handle's motor constants with the model's joint damping

    def map_images(self, mask=True):
        """Pinned host copies of the images that every rendered step refreshes (rr_map_images; a handful of envs only): numpy views
        (rgb [N, H, W, 3] u8, depth [N, H, W] f32, mask [N, H, W] i32 or None) -- valid after `sync()`."""
        key = '_img_mirror_m' if mask else '_img_mirror'
        if getattr(self, key, None) is None:
            pr, pd, pm = C.c_void_p(), C.c_void_p(), C.c_void_p()
            nat.check(self.L.rr_map_images(self.h, C.byref(pr), C.byref(pd), C.byref(pm) if mask else None))
            npx = self.N * self.H * self.W
            rgb = np.frombuffer((C.c_uint8 * (npx * 3)).from_address(pr.value), dtype=np.uint8).reshape(self.N, self.H, self.W, 3)
            dep = np.frombuffer((C.c_float * npx).from_address(pd.value), dtype=np.float32).reshape(self.N, self.H, self.W)
            msk = np.frombuffer((C.c_int32 * npx).from_address(pm.value), dtype=np.int32).reshape(self.N, self.H, self.W) if mask else None
            setattr(self, key, (rgb, dep, msk))
        # (whoever asks for the views with the mask gets a mask block that is being refreshed: a block deselected by
        # select_image_mirror is selected again here -- and brought up to date at once by the library -- so that no holder of these
        # views reads a stale mask without an error)
        sel = getattr(self, '_img_sel', 7)
        if mask and not sel & 4:
            self.select_image_mirror(rgb=bool(sel & 1), depth=bool(sel & 2), mask=True)
        return getattr(self, key)

    def select_image_mirror(self, rgb=True, depth=True, mask=True):
        """Which mapped image blocks a rendered step refreshes (rr_select_image_mirror); a block selected again is brought up to
        date at once (valid after `sync_observations()`).  The selection is tracked here: `map_images(mask=True)` selects a
        deselected mask block again."""
        sel = (1 if rgb else 0) | (2 if depth else 0) | (4 if mask else 0)
        if sel != getattr(self, '_img_sel', 7):
            nat.check(self.L.rr_select_image_mirror(self.h, sel))
            self._img_sel = sel

    def close(self):
        self._mirror = self._img_mirror = self._img_mirror_m = None      # (views into memory the library frees)
        if getattr(self, 'h', None):
            self.L.rr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ stepping
    def reset(self, env_mask=None):
        """rr_reset of the masked envs (None: all).  A mask in device memory (a CUDA torch tensor, `__cuda_array_interface__`) is
        read in place on the library's stream, without a host round trip (`write_state(reset=True)`)."""
        if env_mask is None:
            nat.check(self.L.rr_reset(self.h, None))
        elif _on_device(env_mask):
            self.write_state(None, env_mask, reset=True)
        else:
            m = np.ascontiguousarray(env_mask, dtype=np.uint8)
            assert m.shape == (self.N,)
            nat.check(self.L.rr_reset(self.h, m.ctypes.data))

    def step(self, joint_cmd=None, render=False, device_ptr=None):
        """joint_cmd: None (zeros, env.py:333-334), float array [N, 9] on the host, or `device_ptr` (int address of
        an f32 [N, 9] device buffer). render: False / True / uint8 array [N] of per-env camera flags."""
        flags = None
        if isinstance(render, np.ndarray) and render.size > 1:
            flags = np.ascontiguousarray(render, dtype=np.uint8)
            assert flags.shape == (self.N,)
            mode = 2
        else:
            mode = 1 if np.any(render) else 0
        if device_ptr is not None:
            nat.check(self.L.rr_step(self.h, C.c_void_p(device_ptr), 1, mode, flags.ctypes.data if flags is not None else None))
            return
        if joint_cmd is None:
            nat.check(self.L.rr_step(self.h, None, 0, mode, flags.ctypes.data if flags is not None else None))
            return
        a = np.ascontiguousarray(joint_cmd, dtype=np.float32)
        assert a.shape == (self.N, 9), "joint_command must have shape [N, 9]"      # robot.py:190
        assert np.isfinite(a).all(), "joint_command must be finite"               # robot.py:189
        nat.check(self.L.rr_step(self.h, a.ctypes.data, 0, mode, flags.ctypes.data if flags is not None else None))

    def render(self):
        nat.check(self.L.rr_render(self.h))

    def sync(self):
        nat.check(self.L.rr_sync(self.h))

    def sync_observations(self):
        """Waits for the mapped observation blocks of the last step only (rr_sync_observations)."""
        nat.check(self.L.rr_sync_observations(self.h))

    def map_observations(self):
        """Host mirror of the low-dimensional observations (rr_map_observations): numpy views over pinned host memory that every
        step refreshes -- valid after `sync()`.  Returns dict(joints [N, 9], touch [N, 4], obj_pose [N, n_obj, 7], timestep [N],
        errflags [N])."""
        if getattr(self, '_mirror', None) is None:
            p, n = C.c_void_p(), C.c_size_t()
            nat.check(self.L.rr_map_observations(self.h, C.byref(p), C.byref(n)))
            N, k = self.N, self.n_objects
            buf = (C.c_float * (n.value // 4)).from_address(p.value)
            f = np.frombuffer(buf, dtype=np.float32)
            o = 0
            out = {}
            for name, shape in (('joints', (N, 9)), ('touch', (N, 4)), ('obj_pose', (N, k, 7))):
                sz = int(np.prod(shape))
                out[name] = f[o:o + sz].reshape(shape)
                o += sz
            out['timestep'] = f[o:o + N].view(np.int32)
            out['errflags'] = f[o + N:o + 2 * N].view(np.uint32)
            self._mirror = out
        return self._mirror

    # ------------------------------------------------------------------ data access
    def host(self, field):
        shape, dt = self._shapes[field]
        out = np.empty(shape, dt)
        nat.check(self.L.rr_copy_to_host(self.h, field, out.ctypes.data, out.nbytes))
        return out

    def device_buffer(self, field):
        shape, dt = self._shapes[field]
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(self.L.rr_get_buffer(self.h, field, C.byref(p), C.byref(n)))
        return nat.DeviceBuffer(p.value, shape, np.dtype(dt).str, self)

    @property
    def state(self):
        return self.host(nat.F_STATE)

    @state.setter
    def state(self, s):
        s = np.ascontiguousarray(s, dtype=np.float32)
        assert s.shape == (self.N, 61)
        nat.check(self.L.rr_set_state(self.h, s.ctypes.data))

    # ------------------------------------------------------------------ state writes and reads on the device
    def _state_arg(self, a, name, kinds, shape):
        """An argument of write_state -> (address, 1 on the device / 0 on the host, object that keeps the memory alive).  A CUDA
        torch tensor or a `__cuda_array_interface__` object is device memory, anything else a host array; either must have one of
        the dtypes `kinds` (numpy names) and exactly `shape`, and be contiguous: a ValueError naming the argument otherwise."""
        what = "%s must be a contiguous %s array of shape %s" % (name, ' or '.join(kinds), shape)
        if hasattr(a, 'is_cuda') and hasattr(a, 'data_ptr'):        # a torch tensor
            if a.is_cuda:
                if str(a.dtype).replace('torch.', '') not in kinds or tuple(a.shape) != shape or not a.is_contiguous():
                    raise ValueError("%s, not %s %s%s" % (what, a.dtype, tuple(a.shape), '' if a.is_contiguous() else ' (not contiguous)'))
                return int(a.data_ptr()), 1, a
            a = a.numpy()
        cai = getattr(a, '__cuda_array_interface__', None)
        if cai is not None:
            dt = np.dtype(cai['typestr'])
            dense = tuple(int(np.prod(shape[i + 1:])) * dt.itemsize for i in range(len(shape)))
            if dt.name not in kinds or tuple(cai['shape']) != shape or cai.get('strides') not in (None, dense):
                raise ValueError("%s, not %s %s strides %s" % (what, cai['typestr'], tuple(cai['shape']), cai.get('strides')))
            return int(cai['data'][0]), 1, a
        a = np.asarray(a)
        if a.dtype.name not in kinds or a.shape != shape or not a.flags.c_contiguous:
            raise ValueError("%s, not %s %s%s" % (what, a.dtype, a.shape, '' if a.flags.c_contiguous else ' (not contiguous)'))
        return a.ctypes.data, 0, a

    def write_state(self, state=None, env_mask=None, *, joint_pos=False, joint_vel=False, obj_pose=False, obj_vel=False, reset=False,
                    fresh=False):
        """Masked write into the state by column groups (rr_write_state): resets, teleports, postures and velocity kicks decided
        on the device.  state: float32 [N, 61], the rows of `state` / `read_state()` -- q[11] qd[11], per object pos3 quat4 lin3
        ang3; env_mask: uint8 or bool [N] (None: all envs).  Both are CUDA torch tensors / `__cuda_array_interface__` objects, read
        in place on the library's stream without waiting (produce them on that stream or synchronise first, and keep them unchanged
        until later work on that stream), or both host arrays (staged, synchronous).  Per masked env, in this order: `reset` (as
        `reset()`), then the selected groups -- joint_pos (columns 0..10), joint_vel (11..21), obj_pose (pos3 quat4 of this handle's
        objects; without obj_vel the object's twist is zeroed, a teleport), obj_vel (lin3 ang3; alone: a velocity kick) --, then
        `fresh`: error flags 0, touch 0, contact history dropped, what `state = ...` does behind its write.  Without reset / fresh
        the contact history, clock, error flags, touch sensors and motor targets are kept (a frozen env stays frozen).  Columns
        that are not selected, rows of unmasked envs and columns of objects the handle does not have are not used (NaN is fine
        there); selected values are not validated -- the next step's guard flags a non-finite state.  Wrong dtype, shape,
        contiguity, arguments on different sides, column flags without a state or no flag at all raise ValueError before the library
        is called.  The episode record is not touched: re-base the score with `set_env_goals`, as after `reset()`."""
        parts = ((nat.W_JOINT_POS if joint_pos else 0) | (nat.W_JOINT_VEL if joint_vel else 0) | (nat.W_OBJ_POSE if obj_pose else 0) |
                 (nat.W_OBJ_VEL if obj_vel else 0) | (nat.W_RESET if reset else 0) | (nat.W_FRESH if fresh else 0))
        if parts == 0:
            raise ValueError("write_state: none of joint_pos, joint_vel, obj_pose, obj_vel, reset, fresh is set")
        if state is None and parts & nat.W_COLUMNS:
            raise ValueError("write_state: state is None, but joint_pos / joint_vel / obj_pose / obj_vel need one")
        if state is not None and not parts & nat.W_COLUMNS:
            raise ValueError("write_state: a state without any of joint_pos, joint_vel, obj_pose, obj_vel")
        sp, s_dev, s_keep = (None, None, None) if state is None else self._state_arg(state, 'state', ('float32',), (self.N, 61))
        mp, m_dev, m_keep = (None, None, None) if env_mask is None else self._state_arg(env_mask, 'env_mask', ('uint8', 'bool'), (self.N,))
        if s_dev is not None and m_dev is not None and s_dev != m_dev:
            raise ValueError("write_state: state and env_mask must live on the same side (state on the %s, env_mask on the %s)"
                             % (('host', 'device')[s_dev], ('host', 'device')[m_dev]))
        on_dev = s_dev if s_dev is not None else (m_dev or 0)
        nat.check(self.L.rr_write_state(self.h, sp, mp, parts, on_dev))
        del s_keep, m_keep

    def read_state(self):
        """One launch on the library's stream gathers the present state into the device buffer of the `state` field
        (rr_read_state) and returns it: float32 [N, 61], zero copy (DLPack / `__cuda_array_interface__`), valid for readers ordered
        behind the call.  Steps do not refresh it, and `state = ...`, `set_object_poses`, `evaluate_goals` and a host
        `write_state` use the same buffer for staging: copy what has to last."""
        nat.check(self.L.rr_read_state(self.h))
        return self.device_buffer(nat.F_STATE)

    def checkpoint(self):
        """Opaque snapshot (numpy uint8 array) of everything a later `restore` needs to continue bit for bit: state with motor
        targets, contact history of the warm start, episode clocks, error flags, touch sensors, object home poses, object
        dynamics and actuators."""
        n = C.c_size_t()
        nat.check(self.L.rr_checkpoint_bytes(self.h, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        nat.check(self.L.rr_checkpoint_save(self.h, buf.ctypes.data, buf.nbytes))
        return buf

    def restore(self, ckpt):
        buf = np.ascontiguousarray(ckpt, dtype=np.uint8)
        nat.check(self.L.rr_checkpoint_restore(self.h, buf.ctypes.data, buf.nbytes))

    # ------------------------------------------------------------------ env forks and snapshot slots on the device
    def _source_index(self, src_index):
        """src_index of copy_envs -> (address or None, index_on_device, object that keeps the memory alive).  A host integer array
        [N] is checked here for shape and range (-1 or an env); a device array (`__cuda_array_interface__`, a CUDA torch tensor) for
        int32, contiguous and shape [N] -- its values are the kernel's to check.  Anything else raises ValueError."""
        N = self.N
        if src_index is None:
            return None, 0, None
        if hasattr(src_index, 'is_cuda') and hasattr(src_index, 'data_ptr'):        # a torch tensor
            if src_index.is_cuda:
                if str(src_index.dtype) != 'torch.int32' or tuple(src_index.shape) != (N,) or not src_index.is_contiguous():
                    raise ValueError("a device src_index must be a contiguous int32 tensor of shape (%d,), not %s %s"
                                     % (N, src_index.dtype, tuple(src_index.shape)))
                return int(src_index.data_ptr()), 1, src_index
            src_index = src_index.numpy()
        cai = getattr(src_index, '__cuda_array_interface__', None)
        if cai is not None:
            if np.dtype(cai['typestr']) != np.dtype(np.int32) or tuple(cai['shape']) != (N,) or cai.get('strides') not in (None, (4,)):
                raise ValueError("a device src_index must be a contiguous int32 array of shape (%d,), not %s %s"
                                 % (N, cai['typestr'], tuple(cai['shape'])))
            return int(cai['data'][0]), 1, src_index
        a = np.asarray(src_index)
        if a.dtype.kind not in 'iu':
            raise ValueError("src_index must be an integer array, not %s" % a.dtype)
        if a.shape != (N,):
            raise ValueError("src_index must have shape (%d,), not %s" % (N, a.shape))
        bad = np.flatnonzero((a < -1) | (a >= N))
        if bad.size:
            raise ValueError("src_index: env %d: %d is not -1 or in [0, %d)" % (bad[0], a[bad[0]], N))
        a = np.ascontiguousarray(a, dtype=np.int32)
        return a.ctypes.data, 0, a

    def snapshot_slots(self, n):
        """n snapshot slots (0 .. 64) on the device (rr_snapshot_slots), every one filled with the present records of the running
        envs; replaces all earlier slots, 0 frees them."""
        nat.check(self.L.rr_snapshot_slots(self.h, int(n)))

    def copy_envs(self, src_index=None, src_slot=None, dst_slot=None):
        """The record of env i in dst_slot becomes the record of env src_index[i] in src_slot (rr_copy_envs); a slot of None is the
        running envs.  src_index: None (identity), an integer array [N] on the host (-1: keep env i), or an int32 device array [N]
        (`__cuda_array_interface__` / CUDA torch tensor, read in place on the library's stream; an entry out of range keeps that
        env).  A record is the state with the motor targets, the contact history of the warm start, clock, error flags and touch
        sensors: the copy continues its source's run bit for bit.  Settings (object dynamics, actuators, home poses, cameras,
        appearance), the episode record and the images stay with the destination env.  Same slot with an index copies as if all
        sources were read first (swaps and cycles are fine).  Does not wait for the device."""
        ptr, on_dev, keep = self._source_index(src_index)
        nat.check(self.L.rr_copy_envs(self.h, nat.SLOT_LIVE if src_slot is None else int(src_slot),
                                      nat.SLOT_LIVE if dst_slot is None else int(dst_slot), ptr, on_dev))
        del keep

    def fork(self, src_index):
        """Running env i becomes an exact copy of running env src_index[i] (-1: stays as it is), on the device."""
        self.copy_envs(src_index)

    def save_snapshot(self, slot, src_index=None):
        """pybullet's in-memory saveState for the batch: the running envs' records into `slot` (with src_index: env
        src_index[i] into place i)."""
        self.copy_envs(src_index, None, slot)

    def load_snapshot(self, slot, src_index=None):
        """pybullet's restoreState: the records of `slot` into the running envs (with src_index: saved env src_index[i] into
        running env i -- one saved env into many)."""
        self.copy_envs(src_index, slot, None)

    def set_object_pose(self, env, obj, pose7):
        p = np.ascontiguousarray(pose7, dtype=np.float32)
        assert p.shape == (7,)
        nat.check(self.L.rr_set_object_pose(self.h, int(env), int(obj), p.ctypes.data))

    def set_object_poses(self, poses, env_mask=None):
        """Teleports the objects of the masked envs (None: all): poses [N, n_objects, 7] (xyz + xyzw quaternion),
        velocities zeroed -- one upload for the whole batch."""
        p = np.ascontiguousarray(poses, dtype=np.float32)
        assert p.shape == (self.N, self.n_objects, 7)
        m = None
        if env_mask is not None:
            m = np.ascontiguousarray(env_mask, dtype=np.uint8)
            assert m.shape == (self.N,)
        nat.check(self.L.rr_set_object_poses(self.h, p.ctypes.data, m.ctypes.data if m is not None else None))

    # ------------------------------------------------------------------ object dynamics (changeDynamics / getDynamicsInfo)
    def _dynamics_raw(self):
        out = np.empty((self.N, self.n_objects, 8), np.float32)
        nat.check(self.L.rr_get_object_dynamics(self.h, out.ctypes.data))
        return out

    @staticmethod
    def _dynamics_dict(raw):
        return {'mass': raw[..., 0].copy(), 'inertia': raw[..., 1:4].copy(), 'friction': raw[..., 4].copy(),
                'restitution': raw[..., 5].copy(), 'rolling': raw[..., 6].copy(), 'spinning': raw[..., 7].copy()}

    def object_dynamics(self):
        """Every env's object dynamics: dict of float32 arrays mass [N, n_objects], inertia [N, n_objects, 3] (principal moments,
        object frame), friction (lateral), restitution, rolling, spinning [N, n_objects]."""
        return self._dynamics_dict(self._dynamics_raw())

    def default_object_dynamics(self):
        """The model's values (what a fresh handle has), same layout as `object_dynamics()`."""
        return self._dynamics_dict(self._dyn_default)

    def set_object_dynamics(self, mass=None, inertia=None, friction=None, restitution=None, rolling=None, spinning=None,
                            env_mask=None):
        """pybullet's changeDynamics for the objects of a batch (rr_set_object_dynamics).  Every argument broadcasts to
        [N, n_objects] (`inertia`: [N, n_objects, 3], the principal moments in the object frame); None keeps the current value.
        env_mask (uint8 / bool [N], None: all envs) selects the envs that change.  Mass and inertia must be finite and > 0,
        friction, restitution, rolling and spinning friction finite and >= 0; anything else raises ValueError before the library
        is called, and nothing changes.
        `mass` without `inertia` scales the current inertia by the ratio of the masses (uniform density): a choice of this
        project -- what pybullet does with the inertia on a mass-only changeDynamics cannot be checked here.
        The values outlive reset(), `state = ...` and teleports, and checkpoints carry them."""
        N, k = self.N, self.n_objects
        cur = self._dynamics_raw()
        new = cur.astype(np.float64)

        def arg(v, name, shape, positive):
            try:
                a = np.broadcast_to(np.asarray(v, dtype=np.float64), shape)
            except (ValueError, TypeError):
                raise ValueError("%s: cannot broadcast an array of shape %s to %s" % (name, np.shape(v), shape))
            if not np.isfinite(a).all() or ((a <= 0).any() if positive else (a < 0).any()):
                raise ValueError("%s must be finite and %s" % (name, "> 0" if positive else ">= 0"))
            return a
        if mass is not None:
            new[..., 0] = arg(mass, 'mass', (N, k), True)
            if inertia is None:
                new[..., 1:4] = cur[..., 1:4] * (new[..., 0] / cur[..., 0])[..., None]
        if inertia is not None:
            new[..., 1:4] = arg(inertia, 'inertia', (N, k, 3), True)
        for col, (name, v) in enumerate((('friction', friction), ('restitution', restitution), ('rolling', rolling),
                                         ('spinning', spinning)), start=4):
            if v is not None:
                new[..., col] = arg(v, name, (N, k), False)
        new = new.astype(np.float32)
        if not np.isfinite(new).all() or (new[..., :4] <= 0).any():     # (an inertia scaled out of float32's range)
            raise ValueError("mass and inertia must be finite and > 0 in float32")
        m, mp = _env_mask(env_mask, N)
        nat.check(self.L.rr_set_object_dynamics(self.h, new.ctypes.data, mp))

    # ------------------------------------------------------------------ actuators (setJointMotorControl2 gains / force, jointDamping)
    def _actuators_raw(self):
        out = np.empty((self.N, nat.N_JOINTS, 4), np.float32)
        nat.check(self.L.rr_get_env_actuators(self.h, out.ctypes.data))
        return out

    @staticmethod
    def _actuators_dict(raw):
        return {name: raw[..., k].copy() for k, name in enumerate(nat.ACT_ROW)}

    def env_actuators(self):
        """Every env's actuators in force: dict of float32 arrays kp, kd, max_force, damping [N, 11], the joints in the order of
        q[11] of the state (seven arm joints, then the four finger joints)."""
        return self._actuators_dict(self._actuators_raw())

    def default_env_actuators(self):
        """The handle's values (what a fresh handle has: `solver=` in every row, the model's joint damping), same layout."""
        return self._actuators_dict(self._act_default)

    def set_env_actuators(self, kp=None, kd=None, max_force=None, damping=None, env_mask=None):
        """Per-env, per-joint motor constants and joint damping (rr_set_env_actuators; pybullet's setJointMotorControl2(
        positionGain=, velocityGain=, force=) and changeDynamics(jointDamping=)).  Every argument broadcasts to [N, 11] (joints in the
        order of q[11]); None keeps what is in force.  env_mask (uint8 / bool [N], None: all envs) selects the envs that change.
        All values must be finite and >= 0 (in float32); 0 is a literal zero -- gain off, motor off, no damping.  Anything else
        raises ValueError naming the field before the library is called, and nothing changes.  All four None: the masked envs
        return to the handle's values (`default_env_actuators()`).
        The values outlive reset(), `state = ...` and teleports, and checkpoints carry them.  The ranges are the caller's
        responsibility: kd < 1, or large kp without the rate limit, can diverge under full-range commands (the error flags tell)."""
        N, nj = self.N, nat.N_JOINTS
        m, mp = _env_mask(env_mask, N)
        cols = [(k, _float32_arg(v, name, (N, nj), nonneg=True))
                for k, (name, v) in enumerate(zip(nat.ACT_ROW, (kp, kd, max_force, damping))) if v is not None]
        if not cols:
            nat.check(self.L.rr_set_env_actuators(self.h, None, mp))
            return
        new = self._actuators_raw()
        for k, a in cols:
            new[..., k] = a
        nat.check(self.L.rr_set_env_actuators(self.h, new.ctypes.data, mp))

    def set_object_home(self, env, obj, pose7):
        """Pose object `obj` of env `env` (None: every env) returns to on reset / when it leaves the table
        (Kuka.object_poses, robot.py:19-24)."""
        p = np.ascontiguousarray(pose7, dtype=np.float32)
        assert p.shape == (7,)
        nat.check(self.L.rr_set_object_home(self.h, -1 if env is None else int(env), int(obj), p.ctypes.data))

    def evaluate_goals(self, goal_pos, goal_mask=None):
        """REALRobotEnv.evaluateGoal (env.py:181-200) for the whole batch, on the device: goal_pos [N, n_objects, 3], goal_mask
        [N, n_objects] (None: every object counts) -> scores float32 [N]."""
        g = np.ascontiguousarray(goal_pos, dtype=np.float32)
        assert g.shape == (self.N, self.n_objects, 3)
        m = None
        if goal_mask is not None:
            m = np.ascontiguousarray(goal_mask, dtype=np.uint8)
            assert m.shape == (self.N, self.n_objects)
        out = np.empty(self.N, np.float32)
        nat.check(self.L.rr_evaluate_goals(self.h, g.ctypes.data, m.ctypes.data if m is not None else None, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ goals and episodes on the device
    def set_goals(self, start_poses, final_pos, flags, goal_rgb=None):
        """The goal table of the handle (rr_set_goals): start_poses [G, n_objects, 7] (xyz + xyzw quaternion), final_pos
        [G, n_objects, 3], flags uint8 [G, n_objects] (bit 0 `_native.GOAL_SCORED`: the object counts in the score; bit 1
        `_native.GOAL_HAS_START`: it has a start pose, else it starts from its home pose), goal_rgb uint8 [G, H, W, 3] or None.
        Values whose bit is clear are not read (NaN is fine there); a value that is read must be finite.  G == 0 drops the table.
        A new table leaves every env without a goal until `set_env_goals`."""
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        if f.ndim != 2 or f.shape[1] != self.n_objects:
            raise ValueError("flags must have shape (G, %d), not %s" % (self.n_objects, f.shape))
        G = f.shape[0]
        s = np.ascontiguousarray(start_poses, dtype=np.float32)
        p = np.ascontiguousarray(final_pos, dtype=np.float32)
        if s.shape != (G, self.n_objects, 7) or p.shape != (G, self.n_objects, 3):
            raise ValueError("start_poses / final_pos must have shapes (%d, %d, 7) / (%d, %d, 3), not %s / %s"
                             % (G, self.n_objects, G, self.n_objects, s.shape, p.shape))
        if (~np.isfinite(p) & ((f & nat.GOAL_SCORED) != 0)[..., None]).any() or \
                (~np.isfinite(s) & ((f & nat.GOAL_HAS_START) != 0)[..., None]).any():
            raise ValueError("set_goals: a goal position / start pose that its flag selects is not finite")
        r = None
        if goal_rgb is not None:
            r = np.ascontiguousarray(goal_rgb, dtype=np.uint8)
            if r.shape != (G, self.H, self.W, 3):
                raise ValueError("goal_rgb must have shape (%d, %d, %d, 3), not %s" % (G, self.H, self.W, r.shape))
        nat.check(self.L.rr_set_goals(self.h, G, s.ctypes.data if G else None, p.ctypes.data if G else None, f.ctypes.data if G else None,
                                      r.ctypes.data if (r is not None and G) else None))
        self.n_goals, self.goal_images = G, bool(G and r is not None)

    @staticmethod
    def goal_arrays(goals, names):
        """(start_poses [G, k, 7], final_pos [G, k, 3], flags [G, k], goal_rgb [G, H, W, 3] or None) of a list of `Goal` objects
        for the objects `names`: what evaluate_batched gathers as g_init, g_final and g_mask -- NaN where a goal does not name an
        object, flag bit 0 for the objects of final_state, bit 1 for those of initial_state.  goal_rgb: the goals' retinas when
        every goal has one."""
        names = list(names)
        G, k = len(goals), len(names)
        g_final = np.full((G, k, 3), np.nan, np.float32)
        g_init = np.full((G, k, 7), np.nan, np.float32)
        flags = np.zeros((G, k), np.uint8)
        for j, g in enumerate(goals):
            for n_, pose in (g.final_state or {}).items():
                if n_ in names:
                    g_final[j, names.index(n_)] = np.asarray(pose, np.float32)[:3]
                    flags[j, names.index(n_)] |= nat.GOAL_SCORED
            for n_, pose in (g.initial_state or {}).items():
                if n_ in names:
                    g_init[j, names.index(n_)] = np.asarray(pose, np.float32)
                    flags[j, names.index(n_)] |= nat.GOAL_HAS_START
        rgb = None
        if G and all(getattr(g, 'retina', None) is not None for g in goals):
            rgb = np.stack([np.asarray(g.retina, np.uint8) for g in goals])
        return g_init, g_final, flags, rgb

    def set_goals_from(self, goals, names=None):
        """`set_goals` from `Goal` objects (envs.env.Goal: initial_state / final_state dicts name -> pose, retina); names: the
        objects of the handle (default: `object_names`).  Returns the arrays of `goal_arrays`."""
        arr = self.goal_arrays(goals, self.object_names if names is None else names)
        self.set_goals(*arr)
        return arr

    def set_env_goals(self, index, env_mask=None):
        """Goal index of the masked envs (rr_set_env_goals): int [N] (or one int for all), -1: no goal.  Refreshes their goal
        observations and re-bases their previous score to the score of the current state; moves nothing."""
        try:
            idx = np.ascontiguousarray(np.broadcast_to(np.asarray(index, dtype=np.int32), (self.N,)))
        except ValueError:
            raise ValueError("index must have shape (%d,)" % self.N)
        m, mp = _env_mask(env_mask, self.N)
        nat.check(self.L.rr_set_env_goals(self.h, idx.ctypes.data, mp))

    def set_episode(self, horizon, goal_stride=1):
        """horizon > 0: an env is truncated once its timestep reaches it (<= 0: never); goal_stride: an auto-reset takes an env
        from goal i to (i + goal_stride) mod G (rr_set_episode)."""
        nat.check(self.L.rr_set_episode(self.h, int(horizon), int(goal_stride)))

    def episode_update(self, reset_done=False):
        """One launch on the library's stream (rr_episode_update): score, reward = score - previous score and done bits (1
        truncated, 2 frozen) of every env; with reset_done the envs with done != 0 are reset into their next goal on the device
        (their last observation goes to the `final_obs` buffer).  Does not wait and does not render."""
        nat.check(self.L.rr_episode_update(self.h, 1 if reset_done else 0))

    def _episode_shape(self, which):
        N, k = self.N, self.n_objects
        return {nat.EP_SCORE: ((N,), np.float32), nat.EP_REWARD: ((N,), np.float32), nat.EP_DONE: ((N,), np.uint32),
                nat.EP_GOAL_INDEX: ((N,), np.int32), nat.EP_EPISODE: ((N,), np.int32),
                nat.EP_FINAL_OBS: ((N, 13 + 7 * k + 1), np.float32), nat.EP_GOAL_POS: ((N, k, 3), np.float32),
                nat.EP_GOAL_RGB: ((N, self.H, self.W, 3), np.uint8)}[which]

    def episode_buffer(self, name, host=False):
        """A buffer of the episode record (rr_episode_buffer), by name (`_native.EP_NAMES`: score, reward, done, goal_index,
        episode, final_obs [N, 9 + 4 + 7 n_objects + 1], goal_pos [N, n_objects, 3], goal_rgb [N, H, W, 3]) or EP_* constant: a
        device view (DLPack / __cuda_array_interface__, zero copy; ordering as for the other device buffers), or with host=True a
        numpy copy after a wait.  goal_rgb exists only while the goal table has images -- ask again after `set_goals`."""
        which = nat.EP_NAMES.index(name) if isinstance(name, str) and name in nat.EP_NAMES else name
        if not isinstance(which, (int, np.integer)) or not 0 <= which < len(nat.EP_NAMES):
            raise ValueError("unknown episode buffer %r (known: %s)" % (name, ', '.join(nat.EP_NAMES)))
        shape, dt = self._episode_shape(int(which))
        if host:
            out = np.empty(shape, dt)
            nat.check(self.L.rr_episode_copy_to_host(self.h, int(which), out.ctypes.data, out.nbytes))
            return out
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(self.L.rr_episode_buffer(self.h, int(which), C.byref(p), C.byref(n)))
        return nat.DeviceBuffer(p.value, shape, np.dtype(dt).str, self)

    def link_poses(self):
        out = np.empty((self.N, len(nat.LINK_NAMES), 7), np.float32)
        nat.check(self.L.rr_link_poses(self.h, out.ctypes.data))
        return out

    def contacts(self, env):
        out = np.empty((48, 12), np.float32)
        n = C.c_int32()
        nat.check(self.L.rr_get_contacts(self.h, int(env), out.ctypes.data, 48, C.byref(n)))
        return out[:n.value]

    def contact_observations(self, host=False):
        """Kuka.get_contacts (robot.py:131-150) for the whole batch (rr_contact_observations): one launch on the library's stream
        turns the contact list of the last solved step into
          contacts [N, 48, 12] f32 -- the rows of `contacts(env)` for every env, all zero from the env's count on;
          count [N] i32 -- the number of rows (the RR_F_CONTACT_COUNT field: the only one of the four that later steps refresh);
          body_force [N, 20, 2] f32 -- {max, sum} of the normal force on every body of `body_row_names()`;
          body_partners [N, 20] u32 -- what that body touches: bit 0 a static body, bit 1 + j object j, bit 4 the robot.
        Returns them as device buffers (zero copy, valid after later work on the library's stream or `sync()`; they hold what the
        last call computed), or with host=True as numpy arrays after a sync."""
        nat.check(self.L.rr_contact_observations(self.h))
        get = self.host if host else self.device_buffer
        return {'contacts': get(nat.F_CONTACTS), 'count': get(nat.F_CONTACT_COUNT), 'body_force': get(nat.F_BODY_FORCE),
                'body_partners': get(nat.F_BODY_PARTNERS)}

    # ------------------------------------------------------------------ kinematic observations
    @staticmethod
    def _kinematic_points_arg(links, local_pos=None):
        """(links, local_pos) of `set_kinematic_points` -> (int32 [P], float32 [P, 3]); every argument error is a ValueError raised
        here, before the native call."""
        if isinstance(links, (str, int, np.integer)):
            links = [links]
        idx = []
        for l in links:
            if isinstance(l, str):
                if l not in nat.LINK_NAMES:
                    raise ValueError("unknown link %r (known: %s)" % (l, ', '.join(nat.LINK_NAMES)))
                l = nat.LINK_NAMES.index(l)
            elif not isinstance(l, (int, np.integer)) or isinstance(l, (bool, np.bool_)):
                raise ValueError("a link is a name of LINK_NAMES or an index, not %r" % (l,))
            if not 0 <= int(l) < len(nat.LINK_NAMES):
                raise ValueError("link index %d is not in [0, %d)" % (int(l), len(nat.LINK_NAMES)))
            idx.append(int(l))
        if not 1 <= len(idx) <= nat.KIN_MAX_POINTS:
            raise ValueError("%d points: between 1 and %d are allowed" % (len(idx), nat.KIN_MAX_POINTS))
        if local_pos is None:
            loc = np.zeros((len(idx), 3), np.float32)
        else:
            with np.errstate(over='ignore'):
                loc = np.ascontiguousarray(np.asarray(local_pos, dtype=np.float64).astype(np.float32))
            if loc.shape != (len(idx), 3):
                raise ValueError("local_pos must have shape (%d, 3), not %s" % (len(idx), loc.shape))
            if not np.isfinite(loc).all():
                raise ValueError("local_pos must be finite (in float32)")
        return np.array(idx, np.int32), loc

    def set_kinematic_points(self, links, local_pos=None):
        """The points of `kinematic_observations` (rr_set_kinematic_points): up to 8 pairs of a robot link -- a name of
        `_native.LINK_NAMES` or its index -- and a position [P, 3] in that link's COM frame (pybullet's localPosition; None: the
        frame's origin).  A fresh env has one point, the gripper base (`_native.EE_LINK`) at its origin.  A setting of the env,
        like the cameras: resets, `state`, forks and `restore` keep it."""
        idx, loc = self._kinematic_points_arg(links, local_pos)
        nat.check(self.L.rr_set_kinematic_points(self.h, len(idx), idx.ctypes.data, loc.ctypes.data))

    def kinematic_points(self):
        """(links int32 [P], local_pos float32 [P, 3]) in force (rr_get_kinematic_points)."""
        n = C.c_int32()
        idx, loc = np.zeros(nat.KIN_MAX_POINTS, np.int32), np.zeros((nat.KIN_MAX_POINTS, 3), np.float32)
        nat.check(self.L.rr_get_kinematic_points(self.h, C.byref(n), idx.ctypes.data, loc.ctypes.data))
        return idx[:n.value].copy(), loc[:n.value].copy()

    def _query_buffer(self, fam, name, host):
        """Buffer `name` (of fam.fields, or its index) of a query family (`_native.QUERY_FAMILIES`): the device view, or a host copy.
        The shape is the family's row shape with its one free dim solved from the library's byte count."""
        which = fam.fields.index(name) if isinstance(name, str) and name in fam.fields else name
        if isinstance(which, (bool, np.bool_)) or not isinstance(which, (int, np.integer)) or not 0 <= which < len(fam.fields):
            raise ValueError("unknown %s buffer %r (known: %s)" % (fam.label, name, ', '.join(fam.fields)))
        which = int(which)
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(getattr(self.L, fam.buffer)(self.h, which, C.byref(p), C.byref(n)))
        dt, row, free = fam.buffers[which]
        dims = dict(N=self.N, O=self.n_objects)
        if 'Q' in row and free != 'Q':
            dims['Q'] = len(self.distance_pairs()[0])
        if 'P' in row and free != 'P':
            dims['P'] = len(self.kinematic_points()[0])
        shape = fam.shape(which, dims, n.value)
        if host:
            out = np.empty(shape, dt)
            nat.check(getattr(self.L, fam.copy_to_host)(self.h, which, out.ctypes.data, out.nbytes))
            return out
        return nat.DeviceBuffer(p.value, shape, np.dtype(dt).str, self)

    def kinematic_buffer(self, name, host=False):
        """One buffer of the kinematic observations as its LAST `kinematic_observations` call left it (all zero before the first),
        by name (`_native.KIN_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait."""
        return self._query_buffer(nat.QUERY_FAMILIES['kinematic'], name, host)

    def kinematic_observations(self, host=False):
        """getJointState / getLinkState(computeLinkVelocity=1) / getBaseVelocity / calculateJacobian for the whole batch
        (rr_kinematic_observations): one launch on the library's stream turns the present state into (float32)
          joint_vel [N, 11] -- qd in the order of q[11] of the state;
          link_pose [N, 17, 7] -- the rows of `link_poses()`; link_vel [N, 17, 6] -- world linear velocity of that frame's origin, angular;
          obj_vel [N, n_objects, 6] -- linear, angular;
          point_pos [N, P, 3], point_vel [N, P, 6], jacobian [N, P, 6, 11] -- for the P points of `set_kinematic_points`: rows linear
          xyz then angular xyz, columns the eleven joints (`jacobian @ _native.Q_FROM_CMD`: over the nine command entries).
        Returns them as device buffers (zero copy, DLPack; valid after later work on the library's stream or `sync()`; they hold what
        the last call computed -- steps do not refresh them), or with host=True as numpy arrays after a sync."""
        nat.check(self.L.rr_kinematic_observations(self.h))
        return {name: self.kinematic_buffer(i, host=host) for i, name in enumerate(nat.KIN_FIELDS)}

    # ------------------------------------------------------------------ ray casts against the collision hulls
    @staticmethod
    def _rays_arg(links, segments=None):
        """(links, segments) of `set_rays` -> (int32 [R], float32 [R, 6]); every argument error is a ValueError raised here, before
        the native call.  A link is a name of LINK_NAMES, its index, or 'world' / -1 for the world frame."""
        if isinstance(links, (str, int, np.integer)):
            links = [links]
        idx = []
        for l in links:
            if isinstance(l, str):
                if l != 'world' and l not in nat.LINK_NAMES:
                    raise ValueError("unknown link %r (known: world, %s)" % (l, ', '.join(nat.LINK_NAMES)))
                l = -1 if l == 'world' else nat.LINK_NAMES.index(l)
            elif not isinstance(l, (int, np.integer)) or isinstance(l, (bool, np.bool_)):
                raise ValueError("a link is 'world', a name of LINK_NAMES or an index, not %r" % (l,))
            if not -1 <= int(l) < len(nat.LINK_NAMES):
                raise ValueError("link index %d is neither -1 (the world) nor in [0, %d)" % (int(l), len(nat.LINK_NAMES)))
            idx.append(int(l))
        if len(idx) > nat.RAY_MAX:
            raise ValueError("%d rays: at most %d are allowed" % (len(idx), nat.RAY_MAX))
        if segments is None:
            seg = np.zeros((len(idx), 6), np.float32)
        else:
            try:
                with np.errstate(over='ignore'):
                    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.float64).astype(np.float32))
            except (ValueError, TypeError):
                raise ValueError("segments must be an array of shape (%d, 6)" % len(idx))
            if seg.shape != (len(idx), 6):
                raise ValueError("segments must have shape (%d, 6), not %s" % (len(idx), seg.shape))
            if not np.isfinite(seg).all():
                raise ValueError("segments must be finite (in float32)")
        return np.array(idx, np.int32), seg

    def set_rays(self, links, segments=None):
        """The ray table of `ray_cast` (rr_set_rays): up to 64 rays, each a frame -- 'world' / -1, or a robot link by name of
        `_native.LINK_NAMES` or index: that link's COM frame, pybullet's parentLinkIndex -- and a default segment [R, 6] {from xyz,
        to xyz} in that frame (None: zeros, for tables whose casts always bring their own segments).  A fresh env has no rays.  A
        setting of the env, like the kinematic points: resets, `state`, forks and `restore` keep it."""
        idx, seg = self._rays_arg(links, segments)
        nat.check(self.L.rr_set_rays(self.h, len(idx), idx.ctypes.data, seg.ctypes.data))

    def rays(self):
        """(links int32 [R], segments float32 [R, 6]) in force (rr_get_rays)."""
        n = C.c_int32()
        idx, seg = np.zeros(nat.RAY_MAX, np.int32), np.zeros((nat.RAY_MAX, 6), np.float32)
        nat.check(self.L.rr_get_rays(self.h, C.byref(n), idx.ctypes.data, seg.ctypes.data))
        return idx[:n.value].copy(), seg[:n.value].copy()

    def ray_buffer(self, name, host=False):
        """One buffer of the ray casts as the LAST `ray_cast` call left it (all zero before the first), by name
        (`_native.RAY_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait."""
        return self._query_buffer(nat.QUERY_FAMILIES['ray'], name, host)

    def ray_cast(self, rays=None, host=False):
        """pybullet's rayTestBatch for the whole batch (rr_ray_cast): one launch on the library's stream casts the R rays of
        `set_rays` of every env against the collision hulls -- table, shelf, robot links, this env's objects -- at the present
        state and returns
          hit [N, R, 8] float32 -- {fraction, distance (m), x, y, z (world), nx, ny, nz (world, outward)} of the first hull hit; a
              miss: fraction 1, the segment's length, its end point, a zero normal;
          id [N, R, 4] int32 -- {uid as in the mask image, body as in the contact records, URDF link or -1, collision shape}; all -1
              on a miss.
        rays: None (the table's segments for every env) or float32 [N, R, 6] per-env segments in the frames of the table's links -- a
        numpy array (checked finite, staged, synchronous) or a CUDA torch tensor / `__cuda_array_interface__` object, read in place
        on the library's stream without waiting (produce it on that stream or synchronise first; values are not validated: a
        non-finite segment is a miss).  A ray that starts inside a hull does not hit that hull (a sensor may sit inside its own
        link).  Returns device buffers (zero copy, DLPack; valid after later work on the library's stream or `sync()`; they hold what
        the last call computed -- steps do not refresh them), or with host=True numpy arrays after a sync."""
        R = len(self.rays()[0])
        if R == 0:
            raise ValueError("ray_cast: the ray table is empty (set_rays)")
        rp, on_dev, keep = (None, 0, None) if rays is None else self._state_arg(rays, 'rays', ('float32',), (self.N, R, 6))
        nat.check(self.L.rr_ray_cast(self.h, rp, on_dev))
        del keep
        return {name: self.ray_buffer(i, host=host) for i, name in enumerate(nat.RAY_FIELDS)}

    @staticmethod
    def ray_column(buf, col):
        """Column `col` of a buffer of `ray_cast` as [N, R]: a numpy view, or a strided device view (zero copy) of a device buffer."""
        if isinstance(buf, np.ndarray):
            return buf[:, :, col]
        item = np.dtype(buf.typestr).itemsize
        N, R, cols = buf.shape
        return nat.DeviceBuffer(buf.ptr + col * item, (N, R), buf.typestr, buf._owner, strides=(R * cols * item, cols * item))

    # ------------------------------------------------------------------ closest points between collision hulls
    @staticmethod
    def collision_shapes():
        """One row per collision shape of the model, in the order of the shape indices (column 3 of the ray casts' `id`): a list of
        dicts {index, uid (as in the mask image), body (as in the contact records: -1 static, 0..15 robot body, 16 + i object i),
        link (URDF link or -1), name}.  The name is the link's name of `_native.LINK_NAMES`, or 'table' / 'shelf' / 'robot_base' for
        the statics, or 'cube' / 'tomato' / 'mustard'."""
        from .model import load_model
        scenery = iter(('table', 'shelf'))
        rows = []
        for s, (kind, idx, link, uid) in enumerate(np.array(load_model()['shape_owner']).tolist()):
            if kind == 0:
                name = 'robot_base' if link >= 0 else next(scenery)
            else:
                name = nat.LINK_NAMES[link] if kind == 1 else OBJECT_NAMES[idx]
            rows.append(dict(index=s, uid=uid, body=-1 if kind == 0 else idx if kind == 1 else 16 + idx, link=link, name=name))
        return rows

    @staticmethod
    def _distance_arg(pairs, max_distance=None, n_objects=3):
        """(pairs, max_distance) of `set_distance_pairs` -> (n_pairs, int32 [Q], int32 [Q], float); every argument error is a
        ValueError raised here, before the native call.  pairs: 'collision' (n_pairs = -1: the step's own collision pairs), or a
        sequence of (a, b), each a shape by name of `collision_shapes()` or by index."""
        md = 0.0 if max_distance is None else max_distance
        if isinstance(md, (bool, np.bool_, str)) or not isinstance(md, (int, float, np.integer, np.floating)) or np.isnan(md):
            raise ValueError("max_distance is None or a number of metres (<= 0 or inf: no cull), not %r" % (max_distance,))
        md = float(np.float32(md))
        empty = np.zeros(0, np.int32)
        if isinstance(pairs, str):
            if pairs != 'collision':
                raise ValueError("pairs is 'collision' or a sequence of (shape a, shape b), not %r" % (pairs,))
            return -1, empty, empty, md
        shapes = BatchedREALRobotEnv.collision_shapes()
        names = {r['name']: r['index'] for r in shapes}
        out = []
        try:
            pairs = list(pairs)
        except TypeError:
            raise ValueError("pairs is 'collision' or a sequence of (shape a, shape b), not %r" % (pairs,))
        if len(pairs) > nat.DIST_MAX:
            raise ValueError("%d pairs: at most %d are allowed" % (len(pairs), nat.DIST_MAX))
        for j, pr in enumerate(pairs):
            if isinstance(pr, (str, bytes)) or not hasattr(pr, '__len__') or len(pr) != 2:
                raise ValueError("pair %d: a pair is (shape a, shape b), not %r" % (j, pr))
            ab = []
            for x in pr:
                if isinstance(x, str):
                    if x not in names:
                        raise ValueError("pair %d: unknown shape %r (known: %s)" % (j, x, ', '.join(names)))
                    x = names[x]
                elif not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
                    raise ValueError("pair %d: a shape is a name of collision_shapes() or an index, not %r" % (j, x))
                if not 0 <= int(x) < len(shapes):
                    raise ValueError("pair %d: shape index %d is not in [0, %d)" % (j, int(x), len(shapes)))
                if shapes[int(x)]['body'] >= 16 + int(n_objects):
                    raise ValueError("pair %d: shape %d (%s) belongs to an object this env (%d objects) does not have"
                                     % (j, int(x), shapes[int(x)]['name'], int(n_objects)))
                ab.append(int(x))
            if ab[0] == ab[1]:
                raise ValueError("pair %d: a == b (shape %d)" % (j, ab[0]))
            out.append(ab)
        arr = np.array(out, np.int32).reshape(-1, 2)
        return len(out), np.ascontiguousarray(arr[:, 0]), np.ascontiguousarray(arr[:, 1]), md

    def set_distance_pairs(self, pairs, max_distance=None):
        """The pair table of `closest_points` (rr_set_distance_pairs): up to 96 pairs (a, b) of collision shapes, each by name
        (`collision_shapes()`: a link's name, 'table', 'shelf', 'robot_base', 'cube', 'tomato', 'mustard') or by index; or
        'collision' for the step's own collision pairs in list order.  max_distance (m): pairs whose bounding spheres are further
        apart are culled (status 2); None, <= 0 or inf: no cull.  A fresh env has no pairs.  A setting of the env, like the rays:
        resets, `state`, forks and `restore` keep it."""
        n, a, b, md = self._distance_arg(pairs, max_distance, self.n_objects)
        nat.check(self.L.rr_set_distance_pairs(self.h, n, a.ctypes.data if n > 0 else None, b.ctypes.data if n > 0 else None, md))

    def distance_pairs(self):
        """(pairs int32 [Q, 2], max_distance) in force (rr_get_distance_pairs)."""
        n, md = C.c_int32(), C.c_float()
        a, b = np.zeros(nat.DIST_MAX, np.int32), np.zeros(nat.DIST_MAX, np.int32)
        nat.check(self.L.rr_get_distance_pairs(self.h, C.byref(n), a.ctypes.data, b.ctypes.data, C.byref(md)))
        return np.stack([a[:n.value], b[:n.value]], 1), md.value

    def distance_buffer(self, name, host=False):
        """One buffer of the closest points as the LAST `closest_points` call left it (all zero before the first), by name
        (`_native.DIST_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait."""
        return self._query_buffer(nat.QUERY_FAMILIES['distance'], name, host)

    @staticmethod
    def distance_columns(pts, ids):
        """The named columns of the two buffers of `closest_points`: numpy views, or strided device views (zero copy)."""
        if isinstance(pts, np.ndarray):
            cut = lambda lo: pts[:, :, lo:lo + 3]
        else:
            N, Q, cols = pts.shape
            cut = lambda lo: nat.DeviceBuffer(pts.ptr + 4 * lo, (N, Q, 3), pts.typestr, pts._owner, strides=(Q * cols * 4, cols * 4, 4))
        col = BatchedREALRobotEnv.ray_column
        return dict(distance=col(pts, 0), lower=col(pts, 1), point_a=cut(2), point_b=cut(5), normal=cut(8), status=col(ids, 0),
                    iterations=col(ids, 1), body_a=col(ids, 2), body_b=col(ids, 3))

    def closest_points(self, host=False):
        """pybullet's getClosestPoints for the whole batch (rr_closest_points): one launch on the library's stream computes the Q
        pairs of `set_distance_pairs` of every env at the present state and returns, as [N, Q] (the points and the normal [N, Q, 3])
        columns of the two buffers,
          distance float32 -- Euclidean distance (m) of the convex hulls of the two shapes' vertex sets; 0 when they overlap or touch
              (no penetration depth: inside the 2 cm margin the contact records carry it);
          lower float32 -- a proved lower bound of the distance (distance - lower bounds the error from above);
          point_a, point_b float32 -- world points of A and B that realise the distance; normal -- the unit vector from b to a;
          status int32 -- 0 separated, 1 overlapping or touching, 2 culled by max_distance (distance is the bounding spheres' gap),
              3 iteration cap reached (distance is an upper bound); iterations int32; body_a, body_b int32 -- as in the contact
              records.
        Device views (zero copy, strided, DLPack; valid after later work on the library's stream or `sync()`; they hold what the last
        call computed -- steps do not refresh them), or with host=True numpy views of host copies after a sync."""
        if len(self.distance_pairs()[0]) == 0:
            raise ValueError("closest_points: the pair table is empty (set_distance_pairs)")
        nat.check(self.L.rr_closest_points(self.h))
        return self.distance_columns(self.distance_buffer(0, host=host), self.distance_buffer(1, host=host))

    # ------------------------------------------------------------------ clearance at candidate postures
    @staticmethod
    def _posture_arg(postures, N):
        """The `postures` argument of `posture_clearance` for a handle of N envs -> K.  It is float32 [N, K, 11], C-contiguous, K in
        [1, 32]: a numpy array, a CUDA torch tensor or a `__cuda_array_interface__` object; every violation is a ValueError raised
        here, before the native call."""
        what = "postures must be a C-contiguous float32 array of shape (%d, K, 11), 1 <= K <= %d" % (N, nat.PC_MAX_POSTURES)
        a = postures
        if hasattr(a, 'is_cuda') and hasattr(a, 'data_ptr'):        # a torch tensor
            dt, shape, dense = str(a.dtype).replace('torch.', ''), tuple(a.shape), bool(a.is_contiguous())
        elif getattr(a, '__cuda_array_interface__', None) is not None:
            cai = a.__cuda_array_interface__
            dt, shape = np.dtype(cai['typestr']).name, tuple(cai['shape'])
            dense = cai.get('strides') in (None, tuple(int(np.prod(shape[i + 1:])) * 4 for i in range(len(shape))))
        else:
            try:
                a = np.asarray(a)
            except (ValueError, TypeError):
                raise ValueError("%s, not %r" % (what, type(postures).__name__))
            dt, shape, dense = a.dtype.name, a.shape, bool(a.flags.c_contiguous)
        if dt != 'float32' or len(shape) != 3 or shape[0] != N or shape[2] != nat.N_JOINTS or not 1 <= shape[1] <= nat.PC_MAX_POSTURES or not dense:
            raise ValueError("%s, not %s %s%s" % (what, dt, tuple(shape), '' if dense else ' (not contiguous)'))
        return int(shape[1])

    def posture_buffer(self, name, host=False):
        """One buffer of `posture_clearance` as the LAST call left it (all zero, and K = 0, before the first), by name
        (`_native.PC_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: nearest
        [N, K, 12] float32, id [N, K, 4] int32, distance [N, K, Q] float32, status [N, K, Q] int32."""
        return self._query_buffer(nat.QUERY_FAMILIES['posture'], name, host)

    @staticmethod
    def status_bytes(status, offset=0):
        """Bytes `offset` and `offset + 1` of every int32 of the status words [N, K, Q] as uint8 [N, K, Q] -- numpy views, or
        strided device views (zero copy).  offset 0: (pair_status, pair_iterations) of `posture_clearance` and `signed_distance`;
        offset 1: (pair_iterations, pair_expansions) of `signed_distance`."""
        if isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)) or not 0 <= offset <= 2:
            raise ValueError("offset is 0, 1 or 2 (a status word has four bytes), not %r" % (offset,))
        if isinstance(status, np.ndarray):
            b = status.view(np.uint8).reshape(status.shape + (4,))
            return b[..., offset], b[..., offset + 1]
        N, K, Q = status.shape
        view = lambda byte: nat.DeviceBuffer(status.ptr + byte, (N, K, Q), np.dtype(np.uint8).str, status._owner, strides=(K * Q * 4, Q * 4, 4))
        return view(offset), view(offset + 1)

    def posture_clearance(self, postures, host=False):
        """The clearance of K candidate joint postures per env (rr_posture_clearance): one launch on the library's stream evaluates
        posture (e, k) as if env e's joints q[11] were postures[e, k] -- the objects stay where they are now, unless attached to a link
        (`attach_objects`) -- against the pairs
        of `set_distance_pairs`, and reduces to the NEAREST pair on the device.  The simulation is not touched: no state write, the
        next step stays prepared.  postures: float32 [N, K, 11], 1 <= K <= 32, C-contiguous, the eleven independent joints (a
        nine-entry command maps through `_native.Q_FROM_CMD`) -- a numpy array (staged, synchronous) or a CUDA torch tensor /
        `__cuda_array_interface__` object, read in place on the library's stream without waiting (produce it on that stream or
        synchronise first); values are not validated.  Returns
          distance, lower float32 [N, K]; point_a, point_b, normal float32 [N, K, 3] -- the `closest_points` record of the nearest
              pair: the first minimum of the posture's pair_distance row (the lowest pair index among equal values);
          status int32 [N, K] -- that record's status (0 separated, 1 overlapping, 2 culled: the spheres' gap, 3 cap: an upper bound);
          pair int32 [N, K] -- its index in the pair table; body_a, body_b int32 [N, K] -- as in the contact records;
          pair_distance float32 [N, K, Q] -- every pair's distance, as `closest_points` would report it at that posture;
          pair_status, pair_iterations uint8 [N, K, Q] -- bytes 0 and 1 of the status words.
        Device views (zero copy, strided, DLPack; valid after later work on the library's stream or `sync()`; they hold what the last
        call computed), or with host=True numpy views of host copies after a sync."""
        K = self._posture_arg(postures, self.N)
        if len(self.distance_pairs()[0]) == 0:
            raise ValueError("posture_clearance: the pair table is empty (set_distance_pairs)")
        ptr, on_dev, keep = self._state_arg(postures, 'postures', ('float32',), (self.N, K, nat.N_JOINTS))
        nat.check(self.L.rr_posture_clearance(self.h, ptr, K, on_dev))
        del keep
        near, ids, dist, st = (self.posture_buffer(i, host=host) for i in range(len(nat.PC_FIELDS)))
        if isinstance(near, np.ndarray):
            cut = lambda lo: near[:, :, lo:lo + 3]
        else:
            cut = lambda lo: nat.DeviceBuffer(near.ptr + 4 * lo, (self.N, K, 3), near.typestr, near._owner, strides=(K * 48, 48, 4))
        col = self.ray_column
        ps, pi = self.status_bytes(st)
        return dict(distance=col(near, 0), lower=col(near, 1), point_a=cut(2), point_b=cut(5), normal=cut(8), status=col(ids, 0),
                    pair=col(ids, 1), body_a=col(ids, 2), body_b=col(ids, 3), pair_distance=dist, pair_status=ps, pair_iterations=pi)

    # ------------------------------------------------------------------ signed distance and penetration depth
    def signed_buffer(self, name, host=False):
        """One buffer of `signed_distance` as the LAST call left it (all zero, and K' = 0, before the first), by name
        (`_native.SD_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: deepest
        [N, K', 12] float32, id [N, K', 4] int32, signed [N, K', Q] float32, status [N, K', Q] int32, points [N, Q, 12] float32
        (K' = 1 after a present-state query; `points` is written by present-state queries only)."""
        return self._query_buffer(nat.QUERY_FAMILIES['signed'], name, host)

    def signed_distance(self, postures=None, host=False):
        """The SIGNED distance of the pairs of `set_distance_pairs` for every env (rr_signed_distance): where two hulls are apart,
        what `closest_points` reports; where they overlap, minus the penetration depth -- the length of the shortest translation
        of shape a that separates the two convex hulls --, its direction, two witness points and a proved bound.  One launch on the
        library's stream; the simulation is not touched.  postures None: the present state, one row per env; else float32
        [N, K, 11] exactly as for `posture_clearance` (a numpy array is staged, a CUDA tensor is read in place).  Returns, with a
        leading [N, K] (postures) or [N] (present state),
          distance float32 -- the signed distance of the DEEPEST pair: the first minimum of the row's pair_distance; bound float32 --
              for an overlapping pair minus a proved lower bound of the depth (-bound <= true depth <= -distance), else the lower
              bound of the distance;
          point_a, point_b, normal float32 [..., 3] -- a point of each hull and the unit vector from b towards a, a - b = distance *
              normal for both signs: moving shape a by -distance * normal separates an overlapping pair;
          status int32 -- 0 separated, 1 overlapping (the expansion converged), 2 culled (the spheres' gap), 3 GJK cap, 4 touching
              (distance = bound = 0, normal 0), 5 expansion cap (distance and bound are still valid bounds); pair, body_a, body_b
              int32 -- the pair's index in the table and the bodies as in the contact records;
          pair_distance float32 [..., Q]; pair_status, pair_iterations, pair_expansions uint8 [..., Q] -- bytes 0, 1 and 2 of the
              status words: status, GJK iterations, expansion trips;
        and for the present state also every pair's record as [N, Q] columns: pair_bound, pair_point_a, pair_point_b, pair_normal
        ([N, Q, 3]).  Device views (zero copy, strided, DLPack; valid after later work on the library's stream or `sync()`; they
        hold what the last call computed), or with host=True numpy views of host copies after a sync."""
        present = postures is None
        K = 1 if present else self._posture_arg(postures, self.N)
        if len(self.distance_pairs()[0]) == 0:
            raise ValueError("signed_distance: the pair table is empty (set_distance_pairs)")
        if present:
            nat.check(self.L.rr_signed_distance(self.h, None, 0, 0))
        else:
            ptr, on_dev, keep = self._state_arg(postures, 'postures', ('float32',), (self.N, K, nat.N_JOINTS))
            nat.check(self.L.rr_signed_distance(self.h, ptr, K, on_dev))
            del keep
        return self._signed_columns(present, K, host)

    def _signed_columns(self, present, K, host):
        """The dict of `signed_distance` over the RR_SD_* buffers as the last query (K' = K rows per env) left them."""
        deep, ids, dist, st = (self.signed_buffer(i, host=host) for i in range(4))
        if isinstance(deep, np.ndarray):
            cut = lambda lo: deep[:, :, lo:lo + 3]
        else:
            cut = lambda lo: nat.DeviceBuffer(deep.ptr + 4 * lo, (self.N, K, 3), deep.typestr, deep._owner, strides=(K * 48, 48, 4))
        col = self.ray_column
        ps, pi = self.status_bytes(st)
        pe = self.status_bytes(st, 1)[1]
        out = dict(distance=col(deep, 0), bound=col(deep, 1), point_a=cut(2), point_b=cut(5), normal=cut(8), status=col(ids, 0),
                   pair=col(ids, 1), body_a=col(ids, 2), body_b=col(ids, 3), pair_distance=dist, pair_status=ps, pair_iterations=pi,
                   pair_expansions=pe)
        if not present:
            return out

        def drop(v):        # the K' = 1 axis of a present-state query
            if isinstance(v, np.ndarray):
                return v[:, 0]
            strides = v.strides if v.strides is not None else tuple(int(np.prod(v.shape[i + 1:])) * np.dtype(v.typestr).itemsize for i in range(len(v.shape)))
            return nat.DeviceBuffer(v.ptr, v.shape[:1] + v.shape[2:], v.typestr, v._owner, strides=strides[:1] + strides[2:])
        out = {k: drop(v) for k, v in out.items()}
        pts = self.signed_buffer('points', host=host)
        if isinstance(pts, np.ndarray):
            cutq = lambda lo: pts[:, :, lo:lo + 3]
        else:
            Q = pts.shape[1]
            cutq = lambda lo: nat.DeviceBuffer(pts.ptr + 4 * lo, (self.N, Q, 3), pts.typestr, pts._owner, strides=(Q * 48, 48, 4))
        out.update(pair_bound=col(pts, 1), pair_point_a=cutq(2), pair_point_b=cutq(5), pair_normal=cutq(8))
        return out

    # ------------------------------------------------------------------ joint gradients of the signed distance
    def signed_gradient_buffer(self, name, host=False):
        """One buffer of `signed_distance_gradient` as the LAST call left it (all zero, and K' = 0, before the first), by name
        (`_native.SG_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: gradient
        [N, K', 12] float32 {d s*/dq_0..10, +0.0}, cost [N, K', 12] float32 {dC/dq_0..10, C}, pair_gradient [N, Q, 12] float32
        {d s_j/dq_0..10, +0.0} (K' = 1 after a present-state query; `pair_gradient` is written by present-state queries only)."""
        return self._query_buffer(nat.QUERY_FAMILIES['signed_gradient'], name, host)

    @staticmethod
    def _gradient_views(buf, present):
        """(the eleven joint columns [..., 11], column 11 [...]) of a [N, R, 12] buffer of rows -- numpy views or strided device views
        (zero copy); present: without the K' = 1 axis."""
        if isinstance(buf, np.ndarray):
            g, last = buf[:, :, :11], buf[:, :, 11]
            return (g[:, 0], last[:, 0]) if present else (g, last)
        N, R = buf.shape[:2]
        if present:
            return (nat.DeviceBuffer(buf.ptr, (N, 11), buf.typestr, buf._owner, strides=(R * 48, 4)),
                    nat.DeviceBuffer(buf.ptr + 44, (N,), buf.typestr, buf._owner, strides=(R * 48,)))
        return (nat.DeviceBuffer(buf.ptr, (N, R, 11), buf.typestr, buf._owner, strides=(R * 48, 48, 4)),
                nat.DeviceBuffer(buf.ptr + 44, (N, R), buf.typestr, buf._owner, strides=(R * 48, 48)))

    def signed_distance_gradient(self, postures=None, margin=0.0, host=False):
        """`signed_distance` plus its derivatives over the eleven joints (rr_signed_gradient), for trajectory optimisers: one
        launch on the library's stream at the present state (postures None) or at K candidate postures per env, the objects where
        they are now (an object attached to a link, `attach_objects`, moves with it and takes its joint columns); the simulation is
        not touched.  The arguments are `signed_distance`'s; margin (m, finite, >= 0; with a cull in
        force at most the table's max_distance) is the distance below which a pair costs.  Returns `signed_distance`'s dict (the
        same bytes in the same buffers) and, with a leading [N, K] (postures) or [N] (present state),
          gradient float32 [..., 11] -- d(distance)/dq of the DEEPEST pair: n . (a_k x (a - p_k)) over the joints that move shape a's
              body minus the same on b over those that move b's; +0.0 for a joint that moves neither and for a touching pair
              (status 4); at a kink of the distance (face against face) the gradient of the active feature pair;
          cost float32 [...] -- C = 1/2 sum_j max(margin - pair_distance_j, 0)^2 over all pairs, summed on the device in a fixed order;
          cost_gradient float32 [..., 11] -- dC/dq = -sum_j max(margin - pair_distance_j, 0) d(pair_distance_j)/dq;
        and for the present state pair_gradient float32 [N, Q, 11], every pair's gradient.  The columns are the joints of the
        state's q[11]: `gradient @ _native.Q_FROM_CMD` is the gradient over the nine command entries (the coupled finger joints
        follow their drivers), and likewise for cost_gradient and pair_gradient.  Device views (zero copy, strided, DLPack; valid
        after later work on the library's stream or `sync()`; they hold what the last call computed), or with host=True numpy views
        of host copies after a sync."""
        present = postures is None
        K = 1 if present else self._posture_arg(postures, self.N)
        if len(self.distance_pairs()[0]) == 0:
            raise ValueError("signed_distance_gradient: the pair table is empty (set_distance_pairs)")
        if present:
            nat.check(self.L.rr_signed_gradient(self.h, None, 0, 0, float(margin)))
        else:
            ptr, on_dev, keep = self._state_arg(postures, 'postures', ('float32',), (self.N, K, nat.N_JOINTS))
            nat.check(self.L.rr_signed_gradient(self.h, ptr, K, on_dev, float(margin)))
            del keep
        out = self._signed_columns(present, K, host)
        grad, cost = (self.signed_gradient_buffer(i, host=host) for i in range(2))
        out['gradient'] = self._gradient_views(grad, present)[0]
        out['cost_gradient'], out['cost'] = self._gradient_views(cost, present)
        if present:
            out['pair_gradient'] = self._gradient_views(self.signed_gradient_buffer('pair_gradient', host=host), False)[0]
        return out

    # ------------------------------------------------------------------ swept clearance along joint-space segments
    @staticmethod
    def _segment_arg(segments, N):
        """The `segments` argument of `swept_clearance` for a handle of N envs -> K.  It is float32 [N, K, 2, 11], C-contiguous, K in
        [1, 32]: a numpy array, a CUDA torch tensor or a `__cuda_array_interface__` object; every violation is a ValueError raised
        here, before the native call."""
        what = "segments must be a C-contiguous float32 array of shape (%d, K, 2, 11), 1 <= K <= %d" % (N, nat.PC_MAX_POSTURES)
        a = segments
        if hasattr(a, 'is_cuda') and hasattr(a, 'data_ptr'):        # a torch tensor
            dt, shape, dense = str(a.dtype).replace('torch.', ''), tuple(a.shape), bool(a.is_contiguous())
        elif getattr(a, '__cuda_array_interface__', None) is not None:
            cai = a.__cuda_array_interface__
            dt, shape = np.dtype(cai['typestr']).name, tuple(cai['shape'])
            dense = cai.get('strides') in (None, tuple(int(np.prod(shape[i + 1:])) * 4 for i in range(len(shape))))
        else:
            try:
                a = np.asarray(a)
            except (ValueError, TypeError):
                raise ValueError("%s, not %r" % (what, type(segments).__name__))
            dt, shape, dense = a.dtype.name, a.shape, bool(a.flags.c_contiguous)
        if dt != 'float32' or len(shape) != 4 or shape[0] != N or shape[2] != 2 or shape[3] != nat.N_JOINTS or not 1 <= shape[1] <= nat.PC_MAX_POSTURES or not dense:
            raise ValueError("%s, not %s %s%s" % (what, dt, tuple(shape), '' if dense else ' (not contiguous)'))
        return int(shape[1])

    def sweep_buffer(self, name, host=False):
        """One buffer of `swept_clearance` as the LAST call left it (all zero, and K = 0, before the first), by name
        (`_native.SW_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: stop
        [N, K, 12] float32, hit [N, K, 12] float32, id [N, K, 4] int32, free [N, K, Q] float32."""
        return self._query_buffer(nat.QUERY_FAMILIES['sweep'], name, host)

    def sweep_reach(self):
        """The reach table of `swept_clearance` (rr_sweep_reach), float32 [11, n_shapes]: how far a point of collision shape s can be
        from joint k's origin at any posture, rounded up; 0 where joint k does not move shape s."""
        out = np.zeros((nat.N_JOINTS, len(self.collision_shapes())), np.float32)
        nat.check(self.L.rr_sweep_reach(self.h, out.ctypes.data))
        return out

    def swept_clearance(self, segments, safety=0.0, tolerance=1e-3, host=False):
        """Is the joint-space motion q(t) = q0 + t (q1 - q0), t in [0, 1], free of the pairs of `set_distance_pairs` by `safety`, and if
        not, where does it first touch and what (rr_swept_clearance)?  One launch on the library's stream decides K segments per env
        by conservative advancement -- a proof, not a sampling: it steps t by (proved lower bound of the distance - safety) / (a bound
        of the distance's rate from the reach table) and re-evaluates only the pairs whose proved horizon has run out.  The objects
        stay where they are now; the simulation is not touched.  segments: float32 [N, K, 2, 11], 1 <= K <= 32, C-contiguous, start
        and end posture over the eleven independent joints -- a numpy array (staged, synchronous) or a CUDA torch tensor /
        `__cuda_array_interface__` object, read in place on the library's stream; safety (m, finite, >= 0); tolerance (m, finite,
        >= 1e-6): a pair whose lower bound is within safety + tolerance hits.  Returns, as [N, K] columns,
          fraction float32 -- 1.0 for a free segment, else the t of the stop: every pair's distance exceeds safety for t < fraction;
          q_stop float32 [N, K, 11] -- the posture evaluated last;
          status int32 -- 0 free, 1 hit, 3 step cap (a proved free prefix: continue from q_stop); pair int32 -- the reported pair
              (the lowest index among the hits; at status 3 the pair with the smallest horizon; -1 at status 0);
          steps, evaluations int32 -- postures evaluated (at most 64) and pair searches;
          distance, lower, point_a, point_b ([N, K, 3]), normal ([N, K, 3]) float32 -- the `closest_points` record of the reported
              pair at q_stop (all +0.0 at status 0);
          pair_free_until float32 [N, K, Q] -- for every pair the t up to which it is proved further than safety (at most 1).
        Device views (zero copy, strided, DLPack; valid after later work on the library's stream or `sync()`; they hold what the last
        call computed), or with host=True numpy views of host copies after a sync.  It refuses while objects are attached
        (`attach_objects`): `carried_sweep` is the same query with the carried objects moving."""
        K = self._segment_arg(segments, self.N)
        if len(self.distance_pairs()[0]) == 0:
            raise ValueError("swept_clearance: the pair table is empty (set_distance_pairs)")
        ptr, on_dev, keep = self._state_arg(segments, 'segments', ('float32',), (self.N, K, 2, nat.N_JOINTS))
        nat.check(self.L.rr_swept_clearance(self.h, ptr, K, on_dev, float(safety), float(tolerance)))
        del keep
        return self._sweep_columns(K, host)

    def _sweep_columns(self, K, host):
        """The columns of `swept_clearance` and `carried_sweep` cut from the four sweep buffers as the last call left them."""
        stop, hit, ids, free = (self.sweep_buffer(i, host=host) for i in range(len(nat.SW_FIELDS)))
        if isinstance(hit, np.ndarray):
            cut = lambda buf, lo, n: buf[:, :, lo:lo + n]
        else:
            cut = lambda buf, lo, n: nat.DeviceBuffer(buf.ptr + 4 * lo, (self.N, K, n), buf.typestr, buf._owner, strides=(K * 48, 48, 4))
        col = self.ray_column
        return dict(fraction=col(stop, 0), q_stop=cut(stop, 1, 11), status=col(ids, 0), pair=col(ids, 1), steps=col(ids, 2), evaluations=col(ids, 3),
                    distance=col(hit, 0), lower=col(hit, 1), point_a=cut(hit, 2, 3), point_b=cut(hit, 5, 3), normal=cut(hit, 8, 3), pair_free_until=free)

    def carried_sweep(self, segments, safety=0.0, tolerance=1e-3, host=False):
        """`swept_clearance` with the carried objects moving (rr_carried_sweep): the edge check of the transport half of a plan.  An
        object attached to a link (`attach_objects`) is re-staged with that link at every posture the advancement evaluates, and a
        pair's motion bound takes the carrying body's joints and a per-env reach for a carried shape; free objects stay where they
        are now.  Arguments, refusals and the returned dict of columns are `swept_clearance`'s; the buffers are `sweep_buffer`'s.
        While nothing is attached the call IS `swept_clearance` (the same kernel, the same bytes), so a planner can always call
        this one; an env without attachments on an attached handle gets `swept_clearance`'s bytes too.  The record of a stopped row
        is `posture_clearance(q_stop)`'s on the same handle, bit for bit."""
        K = self._segment_arg(segments, self.N)
        if len(self.distance_pairs()[0]) == 0:
            raise ValueError("carried_sweep: the pair table is empty (set_distance_pairs)")
        ptr, on_dev, keep = self._state_arg(segments, 'segments', ('float32',), (self.N, K, 2, nat.N_JOINTS))
        nat.check(self.L.rr_carried_sweep(self.h, ptr, K, on_dev, float(safety), float(tolerance)))
        del keep
        return self._sweep_columns(K, host)

    # ------------------------------------------------------------------ carried objects: objects attached to links
    @staticmethod
    def _link_id(l):
        """A link of `_native.LINK_NAMES` by name or index -> its index; -1 (free) passes through."""
        if isinstance(l, str):
            if l not in nat.LINK_NAMES:
                raise ValueError("unknown link %r (known: %s)" % (l, ', '.join(nat.LINK_NAMES)))
            return nat.LINK_NAMES.index(l)
        if not isinstance(l, (int, np.integer)) or isinstance(l, (bool, np.bool_)):
            raise ValueError("a link is a name of LINK_NAMES or an index, not %r" % (l,))
        if not -1 <= int(l) < len(nat.LINK_NAMES):
            raise ValueError("link index %d is neither -1 (free) nor in [0, %d)" % (int(l), len(nat.LINK_NAMES)))
        return int(l)

    @classmethod
    def _attach_args(cls, N, n_objects, links, rel_pose=None):
        """(links, rel_pose) of `attach_objects` -> (int32 [N, n_objects], float32 [N, n_objects, 7] or None); every argument error
        that needs no handle is a ValueError raised here, before the native call."""
        shape = (int(N), int(n_objects))
        if isinstance(links, dict):
            arr = np.full(shape, -1, np.int32)
            for key, l in links.items():
                if isinstance(key, str):
                    if key not in OBJECT_NAMES[:shape[1]]:
                        raise ValueError("unknown object %r (this env has: %s)" % (key, ', '.join(OBJECT_NAMES[:shape[1]])))
                    key = OBJECT_NAMES.index(key)
                elif not isinstance(key, (int, np.integer)) or isinstance(key, (bool, np.bool_)) or not 0 <= int(key) < shape[1]:
                    raise ValueError("an object is a name or an index in [0, %d), not %r" % (shape[1], key))
                arr[:, int(key)] = cls._link_id(l)
        else:
            a = np.asarray(links)
            if a.dtype.kind not in 'iu':
                raise ValueError("links is an integer array broadcastable to %s or a dict {object: link}, not dtype %s" % (shape, a.dtype))
            try:
                arr = np.ascontiguousarray(np.broadcast_to(a, shape)).astype(np.int32)
            except ValueError:
                raise ValueError("links: cannot broadcast an array of shape %s to %s" % (a.shape, shape))
            if ((arr < -1) | (arr >= len(nat.LINK_NAMES))).any():
                raise ValueError("links: an entry is neither -1 (free) nor in [0, %d)" % len(nat.LINK_NAMES))
        rel = None
        if rel_pose is not None:
            rel = _float32_arg(rel_pose, 'rel_pose', shape + (7,))
        return np.ascontiguousarray(arr), rel

    def attach_objects(self, links, rel_pose=None, env_mask=None):
        """Declares objects rigid with robot links for the posture queries (rr_set_attachments): what planners call attached or
        carried bodies.  While any attachment is set, `posture_clearance`, `signed_distance` and `signed_distance_gradient` place an
        attached object where its link's forward kinematics puts it at each candidate posture -- link_pose(posture) o rel_pose --
        instead of where the state says, and the gradient gives its shapes the joint columns of that link; free objects, envs
        without attachments and every pair without a carried shape keep their bits.  A query-side setting: no step reads it, and
        it is not a constraint of the simulation.  `swept_clearance` refuses while it is on (`carried_sweep` is the edge check that moves
        the carried objects); `closest_points` is unaffected.
        links: int [N, n_objects] (broadcastable; a link index of `_native.LINK_NAMES`, -1: free) or a dict {object name or index:
        link name or index} applied to every env, objects not named free.  rel_pose: float32 [N, n_objects, 7] (broadcastable), xyz +
        xyzw, the object's pose in the link's COM frame (`link_poses()`' frame: link_pose^-1 o object pose); None: CAPTURED on the
        device from the present state -- attach what the gripper holds right now.  The rows of the masked envs (env_mask, None: all)
        are replaced whole.  Persistent: resets, `write_state`, steps, forks and `set_distance_pairs` keep it; checkpoints and
        snapshots do not carry it."""
        arr, rel = self._attach_args(self.N, self.n_objects, links, rel_pose)
        m, mp = _env_mask(env_mask, self.N)
        nat.check(self.L.rr_set_attachments(self.h, arr.ctypes.data, None if rel is None else rel.ctypes.data, mp))

    def detach_objects(self, env_mask=None):
        """Frees every object of the masked envs (rr_set_attachments with no links).  Without a mask the feature goes off: the queries
        launch the kernels of a handle that never attached, and `swept_clearance` works again."""
        m, mp = _env_mask(env_mask, self.N)
        nat.check(self.L.rr_set_attachments(self.h, None, None, mp))

    def attachments(self):
        """(links int32 [N, n_objects], rel_pose float32 [N, n_objects, 7]) in force (rr_get_attachments): -1 and the identity pose for
        a free object.  A pose given to `attach_objects` comes back to float32 rounding (the sign of its quaternion is free); a
        captured one is what the device composes."""
        links = np.zeros((self.N, self.n_objects), np.int32)
        rel = np.zeros((self.N, self.n_objects, 7), np.float32)
        nat.check(self.L.rr_get_attachments(self.h, links.ctypes.data, rel.ctypes.data))
        return links, rel

    @classmethod
    def carry_pairs(cls, objects, exclude_links=(), n_objects=3):
        """A pair list for `set_distance_pairs` around carried objects (pure host code).  Each named object (name or index) is paired
        with every static shape, every other object and every robot shape except those of `exclude_links` (names or indices of
        `_native.LINK_NAMES`: the links that hold the object touch it by design and would own every row's minimum); behind them the
        robot's own pairs of the step's collision table, in its order: every robot shape against table and shelf and against the
        objects that are not named.  Returns int32 [Q, 2] shape indices, the carried object first in its pairs."""
        shapes = cls.collision_shapes()
        if isinstance(objects, (str, int, np.integer)):
            objects = [objects]
        named = []
        for o in objects:
            if isinstance(o, str):
                if o not in OBJECT_NAMES[:n_objects]:
                    raise ValueError("unknown object %r (this env has: %s)" % (o, ', '.join(OBJECT_NAMES[:n_objects])))
                o = OBJECT_NAMES.index(o)
            elif not isinstance(o, (int, np.integer)) or isinstance(o, (bool, np.bool_)) or not 0 <= int(o) < n_objects:
                raise ValueError("an object is a name or an index in [0, %d), not %r" % (n_objects, o))
            if int(o) not in named:
                named.append(int(o))
        if isinstance(exclude_links, (str, int, np.integer)):
            exclude_links = [exclude_links]
        excluded = set()
        for l in exclude_links:
            l = cls._link_id(l)
            if l < 0:
                raise ValueError("exclude_links names links, not -1")
            excluded.add(l)
        statics = [r['index'] for r in shapes if r['body'] < 0]
        scenery = [r['index'] for r in shapes if r['body'] < 0 and r['link'] < 0]
        robot = [r['index'] for r in shapes if 0 <= r['body'] < 16]
        obj_shape = {r['body'] - 16: r['index'] for r in shapes if 16 <= r['body'] < 16 + n_objects}
        pairs, seen = [], set()

        def put(a, b):
            if (a, b) not in seen and (b, a) not in seen:
                seen.add((a, b))
                pairs.append((a, b))
        for o in named:
            s = obj_shape[o]
            for t in statics:
                put(s, t)
            for p in sorted(obj_shape):
                if p != o:
                    put(s, obj_shape[p])
            for r in robot:
                if shapes[r]['link'] not in excluded:
                    put(s, r)
        others = [obj_shape[p] for p in sorted(obj_shape) if p not in named]
        for r in robot:
            for t in scenery:
                put(r, t)
        for r in robot:
            for s in others:
                put(r, s)
        if len(pairs) > nat.DIST_MAX:
            raise ValueError("%d pairs: at most %d are allowed" % (len(pairs), nat.DIST_MAX))
        return np.array(pairs, np.int32).reshape(-1, 2)

    # ------------------------------------------------------------------ kinematics at candidate postures
    def posture_kinematics_buffer(self, name, host=False):
        """One buffer of `posture_kinematics` as the LAST call left it (all zero, and K = 0, before the first), by name
        (`_native.PK_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: link_pose
        [N, K, 17, 7], point_pos [N, K, P, 3], jacobian [N, K, P, 6, 11] float32, for the P points of `set_kinematic_points`."""
        return self._query_buffer(nat.QUERY_FAMILIES['posture_kinematics'], name, host)

    def posture_kinematics(self, postures, host=False):
        """Where the links and the kinematic points would be at K candidate joint postures per env, and the points' Jacobians there
        (rr_posture_kinematics): one launch on the library's stream evaluates posture (e, k) as if env e's joints q[11] were
        postures[e, k] and writes (float32)
          link_pose [N, K, 17, 7] -- the rows of `kinematic_observations()['link_pose']` (COM frame, xyz + xyzw);
          point_pos [N, K, P, 3], jacobian [N, K, P, 6, 11] -- for the P points of `set_kinematic_points`: rows linear xyz then angular
          xyz, columns the eleven joints (`jacobian @ _native.Q_FROM_CMD`: over the nine command entries).
        A row depends on its posture, the model and the points alone -- not on the env's state; a candidate equal to the present joints
        gets the bits of `kinematic_observations`.  There are no velocity fields: a candidate has no joint velocity.  The simulation
        is not touched: no state write, the next step stays prepared.  postures: float32 [N, K, 11], 1 <= K <= 32, C-contiguous, the
        eleven independent joints -- a numpy array (staged, synchronous) or a CUDA torch tensor / `__cuda_array_interface__` object,
        read in place on the library's stream without waiting (produce it on that stream or synchronise first); values are neither
        validated nor clamped to the joint limits.  Returns device buffers (zero copy, DLPack; valid after later work on the library's
        stream or `sync()`; they hold what the last call computed), or with host=True numpy arrays after a sync."""
        K = self._posture_arg(postures, self.N)
        ptr, on_dev, keep = self._state_arg(postures, 'postures', ('float32',), (self.N, K, nat.N_JOINTS))
        nat.check(self.L.rr_posture_kinematics(self.h, ptr, K, on_dev))
        del keep
        return {name: self.posture_kinematics_buffer(i, host=host) for i, name in enumerate(nat.PK_FIELDS)}

    # ------------------------------------------------------------------ inverse kinematics at candidate targets
    def posture_ik_buffer(self, name, host=False):
        """One buffer of `posture_ik` as the LAST call left it (all zero, and K = 0, before the first), by name (`_native.PIK_FIELDS`)
        or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: posture [N, K, 11] float32, result
        [N, K, 4] float32 {residual, position error, orientation error angle, 0}, info [N, K, 2] int32 {status, iterations}."""
        return self._query_buffer(nat.QUERY_FAMILIES['posture_ik'], name, host)

    def posture_ik(self, targets, seeds=None, point=0, max_iterations=32, tolerance=1e-3, damping=0.1, max_step=0.5,
                   position_only=False, clamp=True, host=False):
        """Joint postures that put the tool at K target poses per env (rr_posture_ik): one launch on the library's stream solves
        target (e, k) by damped least squares over the seven arm joints -- `ik()`'s residual and update -- from seed (e, k).
          targets float32 [N, K, 7], 1 <= K <= 32: world xyz and xyzw quaternion (normalised by the call) of the tool frame, point
              `point` of `set_kinematic_points`: the point's position, its link's COM frame orientation -- what `posture_kinematics`
              reports as `point_pos` and the quaternion of `link_pose[link]`; point 0 of a fresh handle is the gripper base;
          seeds float32 [N, K, 11] or None: the env's present joints (read, never written).  The finger joints 7..10 are copied to the
              output; an arm joint that does not move the point's link keeps its seed value.
        Both are numpy arrays (staged, synchronous) or both CUDA torch tensors / `__cuda_array_interface__` objects, read in place on the
        library's stream without waiting; a mixed pair is a ValueError.  max_iterations in [1, 256]; a row stops when its residual
        |(position error, sin(angle) axis)| (position_only: |position error|, a 3 x 3 system, the quaternion ignored) is below
        `tolerance`; `damping` is lambda of J^T (J J^T + lambda^2 I)^-1 e, `max_step` caps |dq|inf of an update.  clamp=True keeps the arm
        joints within the model's limits (the seed is clamped first); clamp=False wraps them to (-pi, pi] as `ik()` does.  Returns
          posture float32 [N, K, 11] -- goes straight into `posture_clearance`, `signed_distance_gradient`, `posture_kinematics`;
          residual, position_error (m), orientation_error (rad, the true angle) float32 [N, K];
          status int32 [N, K] (0 converged, 1 iteration cap: the last iterate, 2 residual not finite: row unspecified), iterations
          int32 [N, K] (updates applied).
        Device views (zero copy, strided, DLPack; valid after later work on the library's stream or `sync()`; they hold what the last
        call computed), or with host=True numpy views of host copies after a sync.  The simulation is not touched.  A wave of 64 rows
        runs as long as its slowest row."""
        what = "targets must be a C-contiguous float32 array of shape (%d, K, 7), 1 <= K <= %d" % (self.N, nat.PC_MAX_POSTURES)
        cai = getattr(targets, '__cuda_array_interface__', None)
        try:
            shape = tuple(cai['shape'] if cai is not None else targets.shape if hasattr(targets, 'shape') else np.shape(targets))
        except (ValueError, TypeError):
            raise ValueError("%s, not %r" % (what, type(targets).__name__))
        if len(shape) != 3 or shape[0] != self.N or shape[2] != 7 or not 1 <= shape[1] <= nat.PC_MAX_POSTURES:
            raise ValueError("%s, not %s" % (what, shape))
        K = int(shape[1])
        tp, t_dev, t_keep = self._state_arg(targets, 'targets', ('float32',), (self.N, K, 7))
        sp, s_dev, s_keep = (None, None, None) if seeds is None else self._state_arg(seeds, 'seeds', ('float32',), (self.N, K, nat.N_JOINTS))
        if s_dev is not None and s_dev != t_dev:
            raise ValueError("posture_ik: targets and seeds must live on the same side (targets on the %s, seeds on the %s)"
                             % (('host', 'device')[t_dev], ('host', 'device')[s_dev]))
        opt = nat.IkOptions(int(point), int(max_iterations), float(tolerance), float(damping), float(max_step),
                            (nat.PIK_POSITION_ONLY if position_only else 0) | (nat.PIK_CLAMP_LIMITS if clamp else 0))
        nat.check(self.L.rr_posture_ik(self.h, tp, sp, K, t_dev, C.byref(opt)))
        del t_keep, s_keep
        posture, result, info = (self.posture_ik_buffer(i, host=host) for i in range(len(nat.PIK_FIELDS)))
        col = self.ray_column
        return dict(posture=posture, residual=col(result, 0), position_error=col(result, 1), orientation_error=col(result, 2),
                    status=col(info, 0), iterations=col(info, 1))

    # ------------------------------------------------------------------ joint-space dynamics at candidate postures
    def posture_dynamics_buffer(self, name, host=False):
        """One buffer of `posture_dynamics` as the LAST call left it (all zero, and K = 0, before the first), by name
        (`_native.PD_FIELDS`) or index: a device view (zero copy), or with host=True a numpy copy after a wait.  Shapes: mass_matrix
        and mass_inverse [N, K, 11, 11], gravity, bias and torque [N, K, 11] float32."""
        return self._query_buffer(nat.QUERY_FAMILIES['posture_dynamics'], name, host)

    @classmethod
    def _dynamics_args(cls, N, postures, velocities, accelerations):
        """The tensors of `posture_dynamics` for a handle of N envs -> (K, (address or None) x 3, on_device, keep-alive objects).
        Every violation -- shape, dtype, contiguity, velocities without postures, tensors on different sides -- is a ValueError raised
        here, before the native call; nothing of a handle is needed."""
        if postures is None:
            if velocities is not None:
                raise ValueError("posture_dynamics: velocities without postures (the present-state form takes the state's joint velocities)")
            K = 1
        else:
            K = cls._posture_arg(postures, N)
        ptrs, sides, keep = [], [], []
        for a, name in ((postures, 'postures'), (velocities, 'velocities'), (accelerations, 'accelerations')):
            if a is None:
                ptrs.append(None)
                continue
            ptr, dev, k = cls._state_arg(None, a, name, ('float32',), (N, K, nat.N_JOINTS))
            ptrs.append(ptr)
            sides.append((name, dev))
            keep.append(k)
        if len(set(dev for _, dev in sides)) > 1:
            raise ValueError("posture_dynamics: the tensors must live on the same side (%s)"
                             % ', '.join("%s on the %s" % (name, ('host', 'device')[dev]) for name, dev in sides))
        return K, ptrs, (sides[0][1] if sides else 1), keep

    def posture_dynamics(self, postures=None, velocities=None, accelerations=None, inverse=False, host=False):
        """What it costs to hold or move the arm at K candidate rows per env (rr_posture_dynamics; pybullet's calculateMassMatrix and
        calculateInverseDynamics for the whole batch): one launch on the library's stream evaluates row (e, k) -- a posture q, a joint
        velocity qd, a joint acceleration qdd over the eleven independent joints -- and writes (float32)
          mass_matrix [N, K, 11, 11] -- M(q), symmetric bit for bit, exactly +0.0 between the two finger branches;
          gravity [N, K, 11] -- G(q), the torques that hold the posture still;
          bias [N, K, 11] -- G(q) + C(q, qd), the inverse dynamics at zero acceleration;
          torque [N, K, 11] -- M qdd + bias, the inverse dynamics;
          mass_inverse [N, K, 11, 11] -- M^-1, computed and returned only with inverse=True.
        postures, velocities, accelerations: float32 [N, K, 11], 1 <= K <= 32, C-contiguous -- all numpy arrays (staged, synchronous)
        or all CUDA torch tensors / `__cuda_array_interface__` objects, read in place on the library's stream without waiting
        (produce them on that stream or synchronise first); a mixed set is a ValueError.  velocities=None: qd = 0 and `bias` has the
        bytes of `gravity`; accelerations=None: qdd = 0 and `torque` has the bytes of `bias`.  postures=None is the present-state
        form: K = 1, q and qd are the env's own (read, never written), velocities must be None, accelerations may be [N, 1, 11].
        Values are neither validated nor clamped to the joint limits.  The masses and inertias are the handle's (use_urdf_inertia
        counts), gravity is the step's; joint damping and the motors are in no output.  A row depends on its three input rows and the
        model alone.  The simulation is not touched: no state write, the next step stays prepared.  Returns device buffers (zero
        copy, DLPack; valid after later work on the library's stream or `sync()`; they hold what the last call computed), or with
        host=True numpy arrays after a sync."""
        K, (qp, vp, ap), on_dev, keep = self._dynamics_args(self.N, postures, velocities, accelerations)
        nat.check(self.L.rr_posture_dynamics(self.h, qp, vp, ap, K, on_dev, nat.PD_INVERSE if inverse else 0))
        del keep
        return {name: self.posture_dynamics_buffer(i, host=host) for i, name in enumerate(nat.PD_FIELDS) if inverse or name != 'mass_inverse'}

    # ------------------------------------------------------------------ joint torque inputs of the step
    @classmethod
    def _torque_args(cls, N, torques, env_mask):
        """The arguments of `set_joint_torques` for a handle of N envs -> (address or None, torques on the device, address or None,
        mask on the device, keep-alive objects).  Every violation -- shape, dtype, contiguity, a non-finite host value in a masked
        row, torques and mask on different sides -- is a ValueError raised here, before the native call; nothing of a handle is needed."""
        tp = mp = None
        t_dev = m_dev = 0
        keep = []
        if env_mask is not None:
            if _on_device(env_mask):
                mp, m_dev, k = cls._state_arg(None, env_mask, 'env_mask', ('uint8', 'bool'), (N,))
            else:
                k, mp = _env_mask(env_mask, N)
            keep.append(k)
        if torques is not None:
            if _on_device(torques):
                # the [N, 1, 11] view of posture_dynamics()'s present-state form is the same memory as [N, 11]
                shape = tuple(torques.shape) if hasattr(torques, 'shape') else tuple(torques.__cuda_array_interface__['shape'])
                full = (N, 1, nat.N_JOINTS) if shape == (N, 1, nat.N_JOINTS) else (N, nat.N_JOINTS)
                tp, t_dev, k = cls._state_arg(None, torques, 'torques', ('float32',), full)
            else:
                if hasattr(torques, 'is_cuda') and hasattr(torques, 'numpy'):      # a CPU torch tensor
                    torques = torques.numpy()
                try:
                    with np.errstate(over='ignore'):
                        a = np.ascontiguousarray(np.broadcast_to(np.asarray(torques, dtype=np.float64).astype(np.float32), (N, nat.N_JOINTS)))
                except (ValueError, TypeError):
                    raise ValueError("torques: cannot broadcast an array of shape %s to %s" % (np.shape(torques), (N, nat.N_JOINTS)))
                rows = a if env_mask is None or m_dev else a[keep[0] != 0]      # (a host mask: only its rows have to be finite)
                if not np.isfinite(rows).all():
                    raise ValueError("torques must be finite (in float32) in the rows of env_mask")
                tp, t_dev, k = a.ctypes.data, 0, a
            keep.append(k)
            if env_mask is not None and t_dev != m_dev:
                raise ValueError("set_joint_torques: torques and env_mask must live on the same side (torques on the %s, env_mask on the %s)"
                                 % (('host', 'device')[t_dev], ('host', 'device')[m_dev]))
        return tp, t_dev, mp, m_dev, keep

    def set_joint_torques(self, torques=None, env_mask=None):
        """Joint torques for the step (rr_set_joint_torques; pybullet's setJointMotorControl2(TORQUE_CONTROL, force=tau) for the whole
        batch): a table tau float32 [N, 11] over the eleven independent joints in the order of q[11] of the state (N m), all zero on a
        fresh handle.  Every step from now on solves with qd*' = qd* + dt M^-1 tau, the motors, joint limits and contacts on top as
        before: `set_env_actuators(max_force=0)` on a joint plus tau is torque control of that joint, default motors plus tau is
        feed-forward under the position motor, tau = `posture_dynamics()['bias']` holds the arm against gravity.  Joint damping is not
        compensated, values are not clamped.  PERSISTENT, unlike pybullet: nothing clears the table after a step, and `reset`,
        auto-resets, `write_state`, `state = ...`, `fork`, `load_snapshot` and `restore` keep it (a command-side setting that stays
        with its env, like the motor targets; snapshots and checkpoints do not carry it).
        torques: a numpy array that broadcasts to [N, 11] (checked for finiteness in the rows of env_mask, staged, synchronous), or a
        CUDA torch tensor / `__cuda_array_interface__` object of the full shape [N, 11] -- or [N, 1, 11], the view `posture_dynamics()`
        returns at the present state, taken without a copy --, float32, C-contiguous, read in place on the library's stream without
        waiting and not validated (produce it on that stream or synchronise first).  env_mask: uint8 / bool [N] (None: all envs), on
        the same side as the torques; the other envs keep their rows.  torques=None zeroes the rows of env_mask; torques=None without a
        mask zeroes the table and turns the feature off: the steps then launch exactly what they launched before.  An env whose row
        is all zero is not touched by the step -- bit for bit as without torques --, neither is a frozen env.  The look-ahead stays
        valid: new torques every step cost one small launch.
        For torques over the nine entries of a joint command, `torques9 @ _native.Q_FROM_CMD.T` ([N, 9] -> [N, 11]) applies entry 7 to
        q[7] and q[9] and minus entry 8 to q[8] and q[10]; `torques11 @ _native.Q_FROM_CMD` is the generalised force on the command
        entries."""
        tp, t_dev, mp, m_dev, keep = self._torque_args(self.N, torques, env_mask)
        nat.check(self.L.rr_set_joint_torques(self.h, tp, t_dev, mp, m_dev))
        del keep

    def joint_torques(self):
        """Host copy (after a wait) of the joint torque table in force: float32 [N, 11]."""
        out = np.empty((self.N, nat.N_JOINTS), np.float32)
        nat.check(self.L.rr_get_joint_torques(self.h, out.ctypes.data))
        return out

    @property
    def joint_torque_buffer(self):
        """The joint torque table as a device view, float32 [N, 11] (zero copy, DLPack / `__cuda_array_interface__`; the pointer
        never changes).  A write made in the library's stream order is used by the next step, provided the feature is on
        (`set_joint_torques` with a table since the last clearing call)."""
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(self.L.rr_joint_torque_buffer(self.h, C.byref(p), C.byref(n)))
        return nat.DeviceBuffer(p.value, (self.N, nat.N_JOINTS), '<f4', self)

    # ------------------------------------------------------------------ external wrenches of the step
    @staticmethod
    def _wrench_rows(n_objects=3):
        """The names of the rows of the wrench table: robot row j is the first name of LINK_NAMES whose link_body is j (the body joint
        j of q[11] moves), then the objects of a handle with `n_objects` objects."""
        from .model import load_model
        link_body = [int(b) for b in load_model()['link_body']]
        return [nat.LINK_NAMES[link_body.index(j)] for j in range(nat.N_JOINTS)] + list(OBJECT_NAMES[:int(n_objects)])

    @classmethod
    def _wrench_args(cls, N, wrenches, env_mask, n_objects=3):
        """The arguments of `set_external_wrenches` for a handle of N envs and `n_objects` objects -> (address or None, wrenches on the
        device, address or None, mask on the device, keep-alive objects).  Every violation -- shape, dtype, contiguity, a non-finite
        host value in a masked row, an unknown row name, an object the handle does not have, wrenches and mask on different sides --
        is a ValueError raised here, before the native call; nothing of a handle is needed."""
        wp = mp = None
        w_dev = m_dev = 0
        keep = []
        full = (N, nat.XW_BODIES, 6)
        if env_mask is not None:
            if _on_device(env_mask):
                mp, m_dev, k = cls._state_arg(None, env_mask, 'env_mask', ('uint8', 'bool'), (N,))
            else:
                k, mp = _env_mask(env_mask, N)
            keep.append(k)
        if wrenches is not None:
            if _on_device(wrenches):
                wp, w_dev, k = cls._state_arg(None, wrenches, 'wrenches', ('float32',), full)
            else:
                if isinstance(wrenches, dict):
                    names = cls._wrench_rows(n_objects)
                    table = np.zeros(full, np.float64)
                    for key, v in wrenches.items():
                        if isinstance(key, str):
                            if key not in names:
                                raise ValueError("wrenches: unknown row %r (rows of this handle: %s)" % (key, ', '.join(names)))
                            row = names.index(key)
                        elif isinstance(key, (int, np.integer)) and 0 <= int(key) < nat.N_JOINTS + int(n_objects):
                            row = int(key)
                        else:
                            raise ValueError("wrenches: a row is a name of wrench_row_names() or an index in [0, %d), not %r" % (nat.N_JOINTS + int(n_objects), key))
                        if hasattr(v, 'is_cuda') and hasattr(v, 'numpy'):
                            v = v.numpy()
                        try:
                            table[:, row] = np.broadcast_to(np.asarray(v, dtype=np.float64), (N, 6))
                        except (ValueError, TypeError):
                            raise ValueError("wrenches[%r]: cannot broadcast an array of shape %s to %s" % (key, np.shape(v), (N, 6)))
                    wrenches = table
                if hasattr(wrenches, 'is_cuda') and hasattr(wrenches, 'numpy'):      # a CPU torch tensor
                    wrenches = wrenches.numpy()
                try:
                    with np.errstate(over='ignore'):
                        a = np.ascontiguousarray(np.broadcast_to(np.asarray(wrenches, dtype=np.float64).astype(np.float32), full))
                except (ValueError, TypeError):
                    raise ValueError("wrenches: cannot broadcast an array of shape %s to %s" % (np.shape(wrenches), full))
                rows = a if env_mask is None or m_dev else a[keep[0] != 0]      # (a host mask: only its envs' rows have to be finite)
                if not np.isfinite(rows).all():
                    raise ValueError("wrenches must be finite (in float32) in the rows of env_mask")
                wp, w_dev, k = a.ctypes.data, 0, a
            keep.append(k)
            if env_mask is not None and w_dev != m_dev:
                raise ValueError("set_external_wrenches: wrenches and env_mask must live on the same side (wrenches on the %s, env_mask on the %s)"
                                 % (('host', 'device')[w_dev], ('host', 'device')[m_dev]))
        return wp, w_dev, mp, m_dev, keep

    def set_external_wrenches(self, wrenches=None, env_mask=None):
        """External wrenches on robot bodies and objects for the step (rr_set_external_wrenches; pybullet's applyExternalForce /
        applyExternalTorque for the whole batch): a table float32 [N, 14, 6], all zero on a fresh handle.  Rows 0..10 are the eleven
        moving robot bodies -- row j the body that joint j of q[11] moves --, rows 11..13 objects 0..2 (`wrench_row_names()`); a row
        is {Fx, Fy, Fz, Tx, Ty, Tz} in the WORLD frame (N, N m), the force at the body's centre of mass, the torque about it.  Every
        step from now on adds, behind the preparation and in front of the solve, v*' = v* + dt F / m and w*' = w* + dt Iinv T for an
        object (the env's own mass and world inverse inertia) and qd*' = qd* + dt M^-1 tau for the robot, tau_k the sum over the
        bodies b that joint k moves of a_k . ((c_b - p_k) x F_b + T_b); contacts, motors and joint limits act on top as before.
        Values are not clamped.  With joint torques also set the torque term is added first.  PERSISTENT, unlike pybullet: nothing
        clears the table after a step, and `reset`, auto-resets, `write_state`, `state = ...`, `fork`, `load_snapshot` and `restore`
        keep it (snapshots and checkpoints do not carry it).
        wrenches: a numpy array that broadcasts to [N, 14, 6]; or a dict {row name or index: array broadcasting to [N, 6]}, the
        other rows zero (naming an object the handle does not have raises) -- both checked for finiteness in the rows of env_mask,
        staged, synchronous --; or a CUDA torch tensor / `__cuda_array_interface__` object of the full shape, float32, C-contiguous,
        read in place on the library's stream without waiting and not validated.  env_mask: uint8 / bool [N] (None: all envs), on
        the same side as the wrenches; the other envs keep their rows.  wrenches=None zeroes the rows of env_mask; wrenches=None
        without a mask zeroes the table and turns the feature off: the steps then launch exactly what they launched before.  The
        zero rule holds per target: an env whose robot rows are all zero keeps the bits of its qd*, an object whose row is zero those
        of its v* and w*; a frozen env is not touched.  The look-ahead stays valid: new wrenches every step cost one small launch.
        A force at a point or in a body frame: compose T += r x F, or rotate with `link_pose` / the object poses, in torch, then
        write `external_wrench_buffer`."""
        wp, w_dev, mp, m_dev, keep = self._wrench_args(self.N, wrenches, env_mask, self.n_objects)
        nat.check(self.L.rr_set_external_wrenches(self.h, wp, w_dev, mp, m_dev))
        del keep

    def external_wrenches(self):
        """Host copy (after a wait) of the wrench table in force: float32 [N, 14, 6]."""
        out = np.empty((self.N, nat.XW_BODIES, 6), np.float32)
        nat.check(self.L.rr_get_external_wrenches(self.h, out.ctypes.data))
        return out

    @property
    def external_wrench_buffer(self):
        """The wrench table as a device view, float32 [N, 14, 6] (zero copy, DLPack / `__cuda_array_interface__`; the pointer never
        changes).  A write made in the library's stream order is used by the next step, provided the feature is on
        (`set_external_wrenches` with a table since the last clearing call)."""
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(self.L.rr_external_wrench_buffer(self.h, C.byref(p), C.byref(n)))
        return nat.DeviceBuffer(p.value, (self.N, nat.XW_BODIES, 6), '<f4', self)

    def wrench_row_names(self):
        """The bodies of the rows of the wrench table that this handle's step reads: the eleven moving robot bodies, each under the
        first name of `_native.LINK_NAMES` on it, then this handle's objects (the rows of the objects it does not have, up to 14,
        are stored and never read)."""
        return self._wrench_rows(self.n_objects)

    def body_row_names(self):
        """The bodies of the rows of body_force / body_partners: the 17 URDF links, then this handle's objects (the rows of the
        objects it does not have, up to 20, stay zero)."""
        return list(nat.LINK_NAMES) + list(self.object_names)

    # ------------------------------------------------------------------ IK / macro plans (K8)
    def ik(self, targets):
        """Batched DLS IK of the gripper base from every env's current joints. targets [N, 7] (xyz + xyzw quat).
        Returns (q [N, 11], residual [N])."""
        t = np.ascontiguousarray(targets, dtype=np.float32)
        assert t.shape == (self.N, 7)
        q = np.empty((self.N, 11), np.float32)
        err = np.empty(self.N, np.float32)
        nat.check(self.L.rr_ik(self.h, t.ctypes.data, q.ctypes.data, err.ctypes.data))
        return q, err

    def plan_macro(self, macro_actions, env_mask=None):
        """Builds the 1000-step plans of macro actions [N, 2, 2] on the device (env.py:388-454)."""
        m = np.ascontiguousarray(macro_actions, dtype=np.float32).reshape(self.N, 4)
        mk = None
        if env_mask is not None:
            mk = np.ascontiguousarray(env_mask, dtype=np.uint8)
            assert mk.shape == (self.N,)
        nat.check(self.L.rr_plan_macro(self.h, m.ctypes.data, mk.ctypes.data if mk is not None else None))

    def get_plan(self, env):
        out = np.empty((1000, 9), np.float32)
        nat.check(self.L.rr_get_plan(self.h, int(env), out.ctypes.data))
        return out

    def step_plan(self, render=False, idle=None):
        """Every env consumes the next row of its plan; envs flagged in `idle` (uint8 [N]) take zeros(9) instead and
        keep their place (macro_action None, env.py:391-393)."""
        flags = None
        if isinstance(render, np.ndarray) and render.size > 1:
            flags = np.ascontiguousarray(render, dtype=np.uint8)
            mode = 2
        else:
            mode = 1 if np.any(render) else 0
        if idle is not None:
            idle = np.ascontiguousarray(idle, dtype=np.uint8)
            assert idle.shape == (self.N,)
        nat.check(self.L.rr_step_plan_masked(self.h, idle.ctypes.data if idle is not None else None, mode,
                                             flags.ctypes.data if flags is not None else None))

    def step_macro(self, macro_actions, render=False):
        """Batched REALRobotEnv.step_macro (env.py:388-412): a new macro action (or an exhausted plan) triggers
        re-planning for that env; every env then consumes the next row of its plan.  `macro_actions` is an array
        [N, 2, 2] or a sequence whose entries may be None (that env steps with zeros(9), env.py:391-393)."""
        none = np.array([a is None for a in macro_actions], dtype=bool) if not isinstance(macro_actions, np.ndarray) \
            else np.zeros(self.N, bool)
        if none.any():
            macro_actions = [np.zeros((2, 2)) if a is None else a for a in macro_actions]
        m = np.ascontiguousarray(macro_actions, dtype=np.float64).reshape(self.N, 4)
        if not hasattr(self, '_macro_req'):
            self._macro_req = np.full((self.N, 4), np.nan)
            self._macro_step = np.zeros(self.N, np.int64)
        need = ((~np.all(m == self._macro_req, axis=1)) | (self._macro_step >= 1000)) & ~none
        if need.any():
            if not hasattr(self, '_macro_any'):       # the plan buffers exist after the first plan_macro
                self._macro_any = True
            self.plan_macro(m, need.astype(np.uint8))
            self._macro_req[need] = m[need]
            self._macro_step[need] = 0
        if none.all() and not hasattr(self, '_macro_any'):
            self.step(None, render=render)             # nobody has a plan yet: plain zeros step
            return
        self.step_plan(render, idle=none.astype(np.uint8) if none.any() else None)
        self._macro_step[~none] += 1

    # ------------------------------------------------------------------ macro actions decided on the device
    @classmethod
    def _macro_args(cls, N, macro_actions, idle):
        """The arguments of `step_macro_device` for a handle of N envs -> (address, on the device, address or None, keep-alive
        objects).  Every violation -- shape, dtype, contiguity, requests and idle mask on different sides -- is a ValueError raised
        here, before the native call; nothing of a handle is needed."""
        keep = []
        if _on_device(macro_actions):
            shape = tuple(macro_actions.shape) if hasattr(macro_actions, 'shape') else tuple(macro_actions.__cuda_array_interface__['shape'])
            full = (N, 2, 2) if shape == (N, 2, 2) else (N, 4)       # the same memory either way
            mp, m_dev, k = cls._state_arg(None, macro_actions, 'macro_actions', ('float32',), full)
        else:
            if hasattr(macro_actions, 'is_cuda') and hasattr(macro_actions, 'numpy'):      # a CPU torch tensor
                macro_actions = macro_actions.numpy()
            a = np.asarray(macro_actions)
            if a.dtype.kind not in 'fiu':
                raise ValueError("macro_actions must be a real numeric array of shape (%d, 2, 2) or (%d, 4), not dtype %s" % (N, N, a.dtype))
            if a.shape not in ((N, 2, 2), (N, 4)):
                raise ValueError("macro_actions must have shape (%d, 2, 2) or (%d, 4), not %s" % (N, N, a.shape))
            with np.errstate(over='ignore'):
                k = np.ascontiguousarray(a, dtype=np.float32).reshape(N, 4)
            mp, m_dev = k.ctypes.data, 0
        keep.append(k)
        ip = None
        if idle is not None:
            if hasattr(idle, 'is_cuda') and hasattr(idle, 'numpy') and not idle.is_cuda:
                idle = idle.numpy()
            ip, i_dev, k = cls._state_arg(None, idle, 'idle', ('uint8', 'bool'), (N,))
            keep.append(k)
            if i_dev != m_dev:
                raise ValueError("step_macro_device: macro_actions and idle must live on the same side (macro_actions on the %s, idle on the %s)"
                                 % (('host', 'device')[m_dev], ('host', 'device')[i_dev]))
        return mp, m_dev, ip, keep

    def step_macro_device(self, macro_actions, idle=None, render=False):
        """Batched REALRobotEnv.step_macro (env.py:388-467) with the re-plan decision taken on the device (rr_step_macro): one call
        per step, no host bookkeeping.  macro_actions: [N, 2, 2] or [N, 4] {p1x, p1y, p2x, p2y} -- a float32 CUDA torch tensor or
        `__cuda_array_interface__` object (C-contiguous; read in place on the library's stream without waiting and without a
        read-back: produce it on that stream or synchronise first), or a numpy array (converted to float32, staged, synchronous).
        idle: bool / uint8 [N] on the same side, or None: a flagged env steps with zeros(9) and keeps its request record, plan and
        position (`macro_action is None`, env.py:391-393).  Every other env re-plans from its present joints when its request
        differs from its record (IEEE ==: -0.0 equals 0.0, NaN never equals) or its plan is exhausted (position >= 1000), then takes
        the next row of its plan.  render as in `step_plan`.  Resets, `write_state`, forks, snapshots and checkpoints keep record,
        plan and position (policy state): `macro_invalidate` asks for a re-plan.  `step_macro` keeps its own host bookkeeping and
        does not know the record; the two share the plans and positions (`macro_buffer`)."""
        flags = None
        if isinstance(render, np.ndarray) and render.size > 1:
            flags = np.ascontiguousarray(render, dtype=np.uint8)
            if flags.shape != (self.N,):
                raise ValueError("render flags must have shape (%d,)" % self.N)
            mode = 2
        else:
            mode = 1 if np.any(render) else 0
        mp, m_dev, ip, keep = self._macro_args(self.N, macro_actions, idle)
        nat.check(self.L.rr_step_macro(self.h, mp, m_dev, ip, m_dev, mode, flags.ctypes.data if flags is not None else None))
        del keep

    def macro_invalidate(self, env_mask=None):
        """NaN into the request record of the masked envs (bool / uint8 [N], host or device; None: all envs): the next non-idle
        `step_macro_device` re-plans them from their present joints -- "re-plan after a reset" (rr_macro_invalidate)."""
        if env_mask is None:
            nat.check(self.L.rr_macro_invalidate(self.h, None, 0))
            return
        if hasattr(env_mask, 'is_cuda') and hasattr(env_mask, 'numpy') and not env_mask.is_cuda:
            env_mask = env_mask.numpy()
        mp, m_dev, keep = self._state_arg(env_mask, 'env_mask', ('uint8', 'bool'), (self.N,))
        nat.check(self.L.rr_macro_invalidate(self.h, mp, m_dev))
        del keep

    def macro_buffer(self, name, host=False):
        """A buffer of the device-resident macro actions (rr_macro_buffer), by name (`_native.MACRO_NAMES`: request float32 [N, 4],
        position int32 [N], replanned uint8 [N] -- 1 where the last `step_macro_device` planned --, plan float32 [N, 1000, 9]) or
        MACRO_* constant: a device view (DLPack / __cuda_array_interface__, zero copy; ordering as for the other device buffers),
        or with host=True a numpy copy after a wait."""
        which = nat.MACRO_NAMES.index(name) if isinstance(name, str) and name in nat.MACRO_NAMES else name
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or not 0 <= which < len(nat.MACRO_NAMES):
            raise ValueError("unknown macro buffer %r (known: %s)" % (name, ', '.join(nat.MACRO_NAMES)))
        N = self.N
        shape, dt = {nat.MACRO_REQUEST: ((N, 4), np.float32), nat.MACRO_POSITION: ((N,), np.int32), nat.MACRO_REPLANNED: ((N,), np.uint8),
                     nat.MACRO_PLAN: ((N, nat.PLAN_LEN, 9), np.float32)}[int(which)]
        if host:
            out = np.empty(shape, dt)
            nat.check(self.L.rr_macro_copy_to_host(self.h, int(which), out.ctypes.data, out.nbytes))
            return out
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(self.L.rr_macro_buffer(self.h, int(which), C.byref(p), C.byref(n)))
        return nat.DeviceBuffer(p.value, shape, np.dtype(dt).str, self)

    # ------------------------------------------------------------------ cartesian actions decided on the device
    @classmethod
    def _cartesian_args(cls, N, cartesian_commands, gripper_commands, idle):
        """The arguments of `step_cartesian_device` for a handle of N envs -> (address of the targets, address of the gripper
        commands, address of the idle mask or None, on the device, keep-alive objects).  Every violation -- shape, dtype, contiguity,
        the three arrays not on one side -- is a ValueError raised here, before the native call; nothing of a handle is needed."""
        keep, ptrs, sides = [], [], []
        for a, name, shape in ((cartesian_commands, 'cartesian_commands', (N, 7)), (gripper_commands, 'gripper_commands', (N, 2))):
            if _on_device(a):
                p, d, k = cls._state_arg(None, a, name, ('float32',), shape)
            else:
                if hasattr(a, 'is_cuda') and hasattr(a, 'numpy'):      # a CPU torch tensor
                    a = a.numpy()
                a = np.asarray(a)
                if a.dtype.kind not in 'fiu':
                    raise ValueError("%s must be a real numeric array of shape %s, not dtype %s" % (name, shape, a.dtype))
                if a.shape != shape:
                    raise ValueError("%s must have shape %s, not %s" % (name, shape, a.shape))
                with np.errstate(over='ignore'):
                    k = np.ascontiguousarray(a, dtype=np.float32)
                p, d = k.ctypes.data, 0
            keep.append(k), ptrs.append(p), sides.append((name, d))
        ip = None
        if idle is not None:
            if hasattr(idle, 'is_cuda') and hasattr(idle, 'numpy') and not idle.is_cuda:
                idle = idle.numpy()
            ip, d, k = cls._state_arg(None, idle, 'idle', ('uint8', 'bool'), (N,))
            keep.append(k), sides.append(('idle', d))
        if len({d for _, d in sides}) != 1:
            raise ValueError("step_cartesian_device: cartesian_commands, gripper_commands and idle must live on the same side (%s)"
                             % ', '.join("%s on the %s" % (n, ('host', 'device')[d]) for n, d in sides))
        return ptrs[0], ptrs[1], ip, sides[0][1], keep

    def step_cartesian_device(self, cartesian_commands, gripper_commands, idle=None, render=False):
        """Batched REALRobotEnv.step_cartesian (env.py:358-386) with the IK decision taken on the device (rr_step_cartesian): one
        call per step, no host bookkeeping.  cartesian_commands: [N, 7] xyz + xyzw quaternion, gripper_commands: [N, 2] -- float32
        CUDA torch tensors or `__cuda_array_interface__` objects (C-contiguous; read in place on the library's stream without
        waiting and without a read-back: produce them on that stream or synchronise first), or numpy arrays / CPU tensors (converted
        to float32, staged, synchronous); idle: bool / uint8 [N] or None.  The three live on one side.  A flagged env steps with
        zeros(9) and keeps its request record and solution (`cartesian_command is None`, env.py:359-361).  Every other env whose
        request differs from its record (IEEE ==: -0.0 equals 0.0, NaN never equals) is solved from its present joints by `ik()`'s
        rule, bit for bit; an env whose request equals its record is commanded to the stored solution and NOT solved again, as the
        reference reuses last_ik.  The command is [solution, gripper]: the gripper is read every step and is no part of the
        record.  render as in `step_plan`.  Resets, `write_state`, forks, snapshots and checkpoints keep record and solution (policy
        state): `cartesian_invalidate` asks for a new solve.  `ik()` and `REALRobotEnv.step_cartesian` do not know the record."""
        flags = None
        if isinstance(render, np.ndarray) and render.size > 1:
            flags = np.ascontiguousarray(render, dtype=np.uint8)
            if flags.shape != (self.N,):
                raise ValueError("render flags must have shape (%d,)" % self.N)
            mode = 2
        else:
            mode = 1 if np.any(render) else 0
        cp, gp, ip, on_dev, keep = self._cartesian_args(self.N, cartesian_commands, gripper_commands, idle)
        nat.check(self.L.rr_step_cartesian(self.h, cp, gp, ip, on_dev, mode, flags.ctypes.data if flags is not None else None))
        del keep

    def cartesian_invalidate(self, env_mask=None):
        """NaN into the request record of the masked envs (bool / uint8 [N], host or device; None: all envs): the next non-idle
        `step_cartesian_device` solves them from their present joints -- "solve again after a reset" (rr_cartesian_invalidate)."""
        if env_mask is None:
            nat.check(self.L.rr_cartesian_invalidate(self.h, None, 0))
            return
        if hasattr(env_mask, 'is_cuda') and hasattr(env_mask, 'numpy') and not env_mask.is_cuda:
            env_mask = env_mask.numpy()
        mp, m_dev, keep = self._state_arg(env_mask, 'env_mask', ('uint8', 'bool'), (self.N,))
        nat.check(self.L.rr_cartesian_invalidate(self.h, mp, m_dev))
        del keep

    def cartesian_buffer(self, name, host=False):
        """A buffer of the device-resident cartesian actions (rr_cartesian_buffer), by name (`_native.CARTESIAN_NAMES`: request
        float32 [N, 7], solution float32 [N, 7], residual float32 [N], solved uint8 [N] -- 1 where the last `step_cartesian_device`
        solved) or CART_* constant: a device view (DLPack / __cuda_array_interface__, zero copy; ordering as for the other device
        buffers), or with host=True a numpy copy after a wait."""
        which = nat.CARTESIAN_NAMES.index(name) if isinstance(name, str) and name in nat.CARTESIAN_NAMES else name
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or not 0 <= which < len(nat.CARTESIAN_NAMES):
            raise ValueError("unknown cartesian buffer %r (known: %s)" % (name, ', '.join(nat.CARTESIAN_NAMES)))
        N = self.N
        shape, dt = {nat.CART_REQUEST: ((N, 7), np.float32), nat.CART_SOLUTION: ((N, 7), np.float32), nat.CART_RESIDUAL: ((N,), np.float32),
                     nat.CART_SOLVED: ((N,), np.uint8)}[int(which)]
        if host:
            out = np.empty(shape, dt)
            nat.check(self.L.rr_cartesian_copy_to_host(self.h, int(which), out.ctypes.data, out.nbytes))
            return out
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(self.L.rr_cartesian_buffer(self.h, int(which), C.byref(p), C.byref(n)))
        return nat.DeviceBuffer(p.value, shape, np.dtype(dt).str, self)

    def set_camera(self, view, proj):
        """Row-major 4x4 OpenGL view / projection matrices replacing the eye camera of this batch (None, None: the default eye)."""
        if view is None and proj is None:
            nat.check(self.L.rr_set_camera(self.h, None, None))
            return
        v = np.ascontiguousarray(view, dtype=np.float32).reshape(16)
        p = np.ascontiguousarray(proj, dtype=np.float32).reshape(16)
        nat.check(self.L.rr_set_camera(self.h, v.ctypes.data, p.ctypes.data))

    def set_env_cameras(self, views, projs, env_mask=None):
        """Per-env cameras (rr_set_env_cameras): row-major 4x4 OpenGL view / projection matrices, [N, 4, 4] or [4, 4] for every
        env, for the envs of env_mask (uint8 / bool [N], None: all); the other envs keep theirs.  Same conventions and limits as
        set_camera.  Does not render: a masked env keeps its last frame until its next render.  A non-finite matrix of a masked
        env raises and changes nothing; set_camera puts every env back on one camera.  The cameras outlive reset(),
        `state = ...`, teleports and restore().  A sharded batch gathers full image slabs after this call, as after set_camera."""
        N = self.N

        def arg(m, name):
            a = np.asarray(m, dtype=np.float32)
            if a.shape == (4, 4):
                a = np.broadcast_to(a, (N, 4, 4))
            if a.shape != (N, 4, 4):
                raise ValueError("%s must have shape (%d, 4, 4) or (4, 4), not %s" % (name, N, a.shape))
            return np.ascontiguousarray(a)
        v, p = arg(views, 'views'), arg(projs, 'projs')
        m, mp = _env_mask(env_mask, N)
        nat.check(self.L.rr_set_env_cameras(self.h, v.ctypes.data, p.ctypes.data, mp))

    # ------------------------------------------------------------------ appearance (changeVisualShape / lightDirection)
    def render_instances(self):
        """The render instances of the model (rr_render_instances): int32 [n_inst, 4] rows {owner type 0 static / 1 robot body /
        2 object, index of that body or object, uid (the value in the mask image), texture index or -1}.  Instances of objects
        that this handle does not draw (objects < 3) have a row too."""
        n = C.c_int32()
        nat.check(self.L.rr_render_instances(self.h, C.byref(n), None))
        out = np.empty((n.value, 4), np.int32)
        nat.check(self.L.rr_render_instances(self.h, C.byref(n), out.ctypes.data))
        return out

    def _n_inst(self):
        if getattr(self, '_n_inst_cached', None) is None:
            n = C.c_int32()
            nat.check(self.L.rr_render_instances(self.h, C.byref(n), None))
            self._n_inst_cached = int(n.value)
        return self._n_inst_cached

    def env_appearance(self):
        """Every env's appearance in force: {'colours': float32 [N, n_inst, 3], 'light_dirs': float32 [N, 3] (unit vectors)}."""
        col = np.empty((self.N, self._n_inst(), 3), np.float32)
        light = np.empty((self.N, 3), np.float32)
        nat.check(self.L.rr_get_env_appearance(self.h, col.ctypes.data, light.ctypes.data))
        return {'colours': col, 'light_dirs': light}

    def default_env_appearance(self):
        """The model's appearance (what a fresh handle has), same layout as `env_appearance()`."""
        return {k: v.copy() for k, v in self._app_default.items()}

    def set_env_appearance(self, colours=None, light_dirs=None, env_mask=None):
        """Per-env appearance (rr_set_env_appearance; pybullet's changeVisualShape(rgbaColor=...) and getCameraImage(
        lightDirection=...)).  colours broadcasts to [N, n_inst, 3] -- the colour that replaces the model's for every render
        instance (`render_instances()` tells what each belongs to), finite and >= 0, no alpha; light_dirs broadcasts to [N, 3] --
        the direction towards the light, finite and longer than 1e-6, normalised by the library; None keeps what is in force.
        env_mask (uint8 / bool [N], None: all envs) selects the envs that change.  Anything else raises ValueError before the
        library is called, and nothing changes.  All three None: back to the model's appearance for every env.
        Does not render: a masked env keeps its last frame until its next render, which shows the whole env in its new appearance.
        The appearance outlives reset(), `state = ...`, teleports and restore(); set_camera keeps it.  A sharded batch gathers
        full image slabs after this call, as after set_camera."""
        N = self.N
        if colours is None and light_dirs is None:
            if env_mask is not None:
                raise ValueError("set_env_appearance: an env_mask needs colours or light_dirs")
            nat.check(self.L.rr_set_env_appearance(self.h, None, None, None))
            return
        c = l = None
        if colours is not None:
            c = _float32_arg(colours, 'colours', (N, self._n_inst(), 3))
            if (c < 0).any():
                raise ValueError("colours must be >= 0")
        if light_dirs is not None:
            l = _float32_arg(light_dirs, 'light_dirs', (N, 3))
            with np.errstate(over='ignore'):
                n2 = (l * l).sum(-1, dtype=np.float32)
            if not np.isfinite(n2).all() or not (np.sqrt(n2) > 1e-6).all():
                raise ValueError("light_dirs must be longer than 1e-6 (and their float32 norm finite)")
        m, mp = _env_mask(env_mask, N)
        nat.check(self.L.rr_set_env_appearance(self.h, c.ctypes.data if c is not None else None, l.ctypes.data if l is not None else None, mp))

    def set_timing(self, on):
        nat.check(self.L.rr_set_timing(self.h, int(on)))

    def get_timing(self):
        ms = np.zeros(nat.NUM_KERNELS, np.float32)
        n = np.zeros(nat.NUM_KERNELS, np.int32)
        nat.check(self.L.rr_get_timing(self.h, ms.ctypes.data, n.ctypes.data))
        return dict(zip(nat.KERNEL_NAMES, zip(ms.tolist(), n.tolist())))
