"""The inputs of the device-resident cartesian action tests (tests/test_gpu_cartesian_device.py), made from fixed seeds so that
tests/test_cartesian_device_host.py can check their conditions on the CPU with oracle/kinematics.py (float64): every target is the
forward kinematics of a posture within +-0.3 rad of the env's scattered posture."""
import functools

import numpy as np

from oracle.kinematics import EE_LINK, ik_candidates, link_pose

N = 67              # neither a multiple of 64 nor of the 32 slots of a solver wave
POSTURE_SEED = 5    # the scattered postures of the handles (scatter_postures)
TARGET_SEED = 31    # the targets of step 0 / of the float64 check
IK_TOL = 1e-3       # tests/test_gpu_ik_macro.py: device (float32) vs checker (float64) on the same branch, both converged
NEAR = 0.3          # rad
DRAWS = 40          # perturbations tried per row of separated_targets()


def mat_to_quat(R):
    """xyzw quaternion of a rotation matrix (float64), w >= 0"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    x, y, z = np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])
    q = np.array([x, y, z, w])
    return q / np.linalg.norm(q)


def postures(n=N, seed=POSTURE_SEED):
    """float32 [n, 7]: every env's scattered arm posture (the draw of tests/test_gpu_macro_device.py's scatter_postures)"""
    return np.random.default_rng(seed).uniform(-0.8, 0.8, size=(n, 7)).astype(np.float32)


def near_postures(n=N, seed=TARGET_SEED, posture_seed=POSTURE_SEED):
    """float64 [n, 7]: a posture within +-NEAR of every env's scattered posture"""
    return postures(n, posture_seed).astype(np.float64) + np.random.default_rng(seed).uniform(-NEAR, NEAR, size=(n, 7))


def targets(n=N, seed=TARGET_SEED, posture_seed=POSTURE_SEED):
    """float32 [n, 7] xyz + xyzw quaternion: the gripper base's pose at near_postures(n, seed)"""
    out = np.empty((n, 7), np.float32)
    q11 = np.zeros(11)
    for i, q in enumerate(near_postures(n, seed, posture_seed)):
        q11[:7] = q
        R, p = link_pose(q11, EE_LINK)
        out[i, :3], out[i, 3:] = p, mat_to_quat(R)
    return out


@functools.lru_cache(maxsize=None)
def separated_targets():
    """(near postures float64 [N, 7], targets float32 [N, 7]) of the N = 67 handles: as targets(), but a row's perturbation is drawn
    again (its own generator, at most DRAWS times) until the row's two float64 candidates both meet the solver's threshold within 200
    updates and their elbow heights differ by 5 IK_TOL or more -- a float32 solver then has no near-tie to decide the other way.  A
    row that never gets there keeps its last draw; the host test counts such rows against the 5 % it allows."""
    q0 = postures()
    near, out = np.empty((N, 7)), np.empty((N, 7), np.float32)
    q11 = np.zeros(11)
    for i in range(N):
        rng = np.random.default_rng([TARGET_SEED, i])
        for _ in range(DRAWS):
            near[i] = q0[i].astype(np.float64) + rng.uniform(-NEAR, NEAR, size=7)
            q11[:7] = near[i]
            R, p = link_pose(q11, EE_LINK)
            out[i, :3], out[i, 3:] = p, mat_to_quat(R)
            q11[:7] = q0[i]
            c = ik_candidates(q11, out[i, :3].astype(np.float64), out[i, 3:].astype(np.float64))
            if all(x[1] < 1e-3 and x[5] < 200 for x in c) and abs(c[0][2] - c[1][2]) >= 5 * IK_TOL:
                break
    return near, out


def grippers(rng, n=N):
    return rng.uniform(0.0, 0.5, size=(n, 2)).astype(np.float32)
