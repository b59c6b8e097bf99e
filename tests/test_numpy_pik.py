"""The float64 restatement of rr_posture_ik (tests/numpy_pik.py) against the checker of rr_ik (oracle/kinematics.py `_dls`), and the
conditions the GPU tests' fixture has to meet (tests/test_gpu_posture_ik.py).  No GPU."""
import numpy as np
import pytest

from oracle import kinematics as ok
from real_robots_amd import _native as nat
from tests import numpy_pik as npk
from tests import numpy_step as ns

# the four configurations of the GPU tests' closed loop: (name, link, local offset, position_only, clamp)
FINGER_LINK = nat.LINK_NAMES.index('skin_01')
FINGER_LOCAL = (0.03, -0.02, 0.05)
CONFIGS = [('full_clamped', npk.EE_LINK, None, False, True), ('full_wrapped', npk.EE_LINK, None, False, False),
           ('position_only', npk.EE_LINK, None, True, True), ('finger_point', FINGER_LINK, FINGER_LOCAL, False, True)]


def test_restatement_equals_the_dls_checker():
    """Point 0 (gripper base), full pose, no clamp, default options: q and residual to 1e-9, the same update count, 50 seeded cases.
    `_dls` evaluates the residual before each update only: where it ends at its cap (max_iters updates) its `err` belongs to the
    iterate before the last update, so the residual is compared with the checker's own residual of the returned posture
    (`ee_residual`), which is `err` itself on every converged case."""
    lim = ns.model()['body_limits']
    rng = np.random.default_rng(7)
    goal = rng.uniform(lim.min(1), lim.max(1), (50, 11))
    seed = goal.copy()
    seed[:, :7] += rng.uniform(-0.5, 0.5, (50, 7))
    Re, x, _ = npk.tool_frame(goal)
    from tests.numpy_kinematics import mat_to_quat
    targets = np.concatenate([x, mat_to_quat(Re) * 1.7], -1)            # (not normalised: both sides normalise)
    out = npk.solve(targets, seed, max_iterations=32, clamp=False)
    converged = 0
    for i in range(50):
        Rt = ok.quat_to_mat(targets[i, 3:] / np.linalg.norm(targets[i, 3:]))
        q, err, iters = ok._dls(seed[i].copy(), targets[i, :3], Rt, 32, 1e-3, 0.1)
        assert iters == out['iterations'][i], i
        assert np.abs(q - out['posture'][i]).max() <= 1e-9, i
        assert abs(ok.ee_residual(q, targets[i, :3], targets[i, 3:]) - out['residual'][i]) <= 1e-9, i
        if iters < 32:
            converged += 1
            assert abs(err - out['residual'][i]) <= 1e-9 and out['status'][i] == 0, i
        else:
            assert out['status'][i] == (0 if out['residual'][i] < 1e-3 and out['cos'][i] > 0 else 1), i
    assert converged >= 40


@pytest.mark.parametrize('name,link,local,position_only,clamp', CONFIGS)
def test_fixture_conditions(name, link, local, position_only, clamp):
    """160 rows: at a cap of 64 the restatement converges on >= 95 % of them, and within 32 updates (the clear-cut rows) on >= 90 %."""
    targets, seeds, goal = npk.fixture(link, local)
    lim = ns.model()['body_limits']
    assert targets.shape == (5, 32, 7) and seeds.shape == (5, 32, 11) and targets.dtype == seeds.dtype == np.float32
    assert (goal[..., :7] >= lim[:7, 0]).all() and (goal[..., :7] <= lim[:7, 1]).all()
    assert (seeds[..., :7] >= lim[:7, 0]).all() and (seeds[..., :7] <= lim[:7, 1]).all()
    assert np.abs(seeds[..., :7] - goal[..., :7]).max() <= 0.3 + 1e-6 and (seeds[..., 7:] == goal[..., 7:]).all()
    out = npk.solve(targets.reshape(-1, 7), seeds.reshape(-1, 11), link, local, max_iterations=npk.FIX_MAX_ITERATIONS,
                    position_only=position_only, clamp=clamp)
    ok_rows = out['status'] == 0
    clear = ok_rows & (out['iterations'] <= npk.CLEAR_CUT)
    print(name, 'converged %.4f clear-cut %.4f mean iterations %.2f' % (ok_rows.mean(), clear.mean(), out['iterations'].mean()))
    assert ok_rows.mean() >= 0.95 and clear.mean() >= 0.90
    assert (out['status'] != 2).all() and (out['iterations'] <= npk.FIX_MAX_ITERATIONS).all()
    if clamp:
        assert (out['posture'][:, :7] >= lim[:7, 0]).all() and (out['posture'][:, :7] <= lim[:7, 1]).all()
    else:
        assert (out['posture'][:, :7] > -np.pi).all() and (out['posture'][:, :7] <= np.pi).all()


def test_a_point_on_link_3_moves_three_joints():
    """The arm joints behind the link keep their seed value; the solve is over joints 0..2."""
    targets, seeds, _ = npk.fixture(3, (0.0, 0.05, 0.1), N=1, K=8)
    out = npk.solve(targets[0], seeds[0], 3, (0.0, 0.05, 0.1), max_iterations=64)
    assert (out['posture'][:, 3:] == seeds[0][:, 3:].astype(np.float64)).all()
    assert (out['status'] == 0).mean() >= 0.5 and (out['iterations'] > 0).any()
