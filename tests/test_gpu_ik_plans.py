"""GPU tests (-m gpu) of rr_ik.inc per env and per row: k_ik from every env's OWN joints and fingers, k_plan_macro's whole
[1000, 9] plan of every env against the recorded float64 plans of tests/golden/ik_plan_cases.json (made by
tests/golden/make_ik_plan_cases.py from oracle/kinematics.py under conditions that keep every way point away from any decision
the two precisions could take differently), and the env mask of rr_plan_macro, the idle path and the last-row clamp of
k_plan_fetch as bitwise twins of plain steps."""
import json

import numpy as np
import pytest

from real_robots_amd.batched import BatchedREALRobotEnv
from oracle.kinematics import ee_residual, ik_candidates, quat_from_euler
from tests.test_ik_plan_cases import ARM_LIMIT, FIXTURE

pytestmark = pytest.mark.gpu
ORIENT = quat_from_euler(0, 3.14, -1.57)
IK_TOL = 1e-3            # rad: device (float32) vs checker (float64) on the same branch, both converged (tests/test_gpu_ik_macro.py)
# Residual returned by the device vs the float64 residual of the q it returns: the project's float32 frame ceiling is 2e-6 per
# entry (prep_ratios, tests/test_gpu_numpy_step.py), times sqrt(6) components, doubled = 1e-5.
RES_TOL = 1e-5
HOME2 = np.array([0, 0, 0, 0, 0, np.pi / 2, np.pi / 2, 0, 0])
IK_SEED = 7              # the seeded draw of (a): checked for the float64 checker alone (shares of converged envs, see _ik_reference)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _postures(rng, n):
    """Distinct postures inside the joint limits, fingers non-zero and different per env (and per finger)."""
    q = np.zeros((n, 11))
    q[:, :7] = rng.uniform(-0.5, 0.5, (n, 7)) * ARM_LIMIT
    q[:, 7:] = rng.uniform(0.05, 1.5, (n, 4))
    return q.astype(np.float32)


def _set_postures(env, q11):
    s = env.state
    s[:, :11] = q11
    s[:, 11:22] = 0.0          # velocities
    env.state = s
    back = env.state
    assert np.array_equal(_bits(back[:, :11]), _bits(q11))
    return back


_ik_ref = {}


def _ik_reference(n):
    """The seeded draw of (a) for n envs and the checker's runs for it, computed once: postures [n, 11] f32, targets [n, 7] f32,
    per env the candidates of the default mode from that env's own joints [(q, residual, key, q one update earlier, its residual,
    updates)] (seed 0 = the env's joints: the single-seed answer), and the single-seed run from the NEIGHBOUR's joints."""
    if n not in _ik_ref:
        rng = np.random.default_rng(IK_SEED)
        q0 = _postures(rng, n)
        pos = np.stack([rng.uniform(-0.25, 0.05, n), rng.uniform(-0.4, 0.4, n), rng.uniform(0.42, 0.6, n)], 1)
        tg = np.concatenate([pos, np.tile(ORIENT, (n, 1))], 1).astype(np.float32)
        t64 = tg.astype(np.float64)                    # what the device is handed
        cands = [ik_candidates(q0[i].astype(np.float64), t64[i, :3], t64[i, 3:]) for i in range(n)]
        other = [ik_candidates(q0[(i + 1) % n].astype(np.float64), t64[i, :3], t64[i, 3:], single_seed=True, max_iters=500)[0]
                 for i in range(n)] if n > 1 else []
        _ik_ref[n] = (q0, tg, cands, other)
    return _ik_ref[n]


def _distance(c, q7):
    """Joint distance of a device solution from a checker run: from its final iterate, or from the iterate before it when that
    one's residual is within float32 rounding of the threshold (the two precisions stop one update apart there)."""
    d = np.abs(c[0][:7] - q7).max()
    return min(d, np.abs(c[3][:7] - q7).max()) if abs(c[4] - 1e-3) < 2e-5 else d


def ik_shares(n):
    """(share of envs the single-seed mode compares, share the default mode can compare) for the checker alone."""
    _, _, cands, _ = _ik_reference(n)
    return (np.mean([c[0][5] < 500 for c in cands]), np.mean([any(x[1] < 1e-2 for x in c) for c in cands]))


@pytest.mark.parametrize('N', [70, 1])
@pytest.mark.parametrize('single', [True, False])
def test_ik_solves_from_every_envs_own_joints_and_keeps_its_fingers(N, single):
    """k_ik for a batch whose envs all differ (N = 70: one full block and a partial one; N = 1): every env's fingers come back bit
    for bit, the returned residual is the float64 residual (position AND orientation) of the returned q, and the solution is
    the checker's for the same seed from THAT env's joints -- not its neighbour's (negative control)."""
    q0, tg, cands, other = _ik_reference(N)
    t64 = tg.astype(np.float64)
    env = BatchedREALRobotEnv(N, objects=1, width=64, height=64, solver={'ik_single_seed': single})
    st = _set_postures(env, q0)
    q, err = env.ik(tg)
    env.close()
    assert np.array_equal(_bits(q[:, 7:11]), _bits(st[:, 7:11])) and (q[:, 7:11] != 0).all()
    assert len({tuple(f) for f in q[:, 7:11]}) == N
    worst_res, worst_q, n_cmp, n_res, n_far = 0.0, 0.0, 0, 0, 0
    for i in range(N):
        if err[i] < 1e-3:
            r64 = ee_residual(q[i].astype(np.float64), t64[i, :3], t64[i, 3:])
            worst_res = max(worst_res, abs(r64 - err[i]))
            assert abs(r64 - err[i]) <= RES_TOL and r64 < 1e-3 + RES_TOL, (i, r64, err[i])
            n_res += 1
        if single:
            c = cands[i][0]
            if not c[5] < 500:                         # the float64 run did not converge before update 500: not compared
                continue
            d = _distance(c, q[i][:7])
            assert d < IK_TOL and err[i] < 1e-3 + RES_TOL, (i, d, err[i], c[1])
            n_far += N > 1 and _distance(other[i], q[i][:7]) > 10 * IK_TOL
        else:
            conv = [c for c in cands[i] if c[1] < 1e-2]
            if not conv or not err[i] < 1e-2:
                assert not conv and not err[i] < 1e-2, (i, err[i], [c[1] for c in cands[i]])   # both sides: nothing converged
                continue
            dd = [_distance(c, q[i][:7]) for c in conv]
            k = int(np.argmin(dd))
            d = dd[k]
            assert d < IK_TOL, (i, dd, err[i])
            best = max(conv, key=lambda c: c[2])
            assert conv[k][2] > best[2] - 1e-4, (i, "device picked another branch", conv[k][2], best[2])
        worst_q = max(worst_q, d)
        n_cmp += 1
    print("k_ik N=%d single_seed=%s: %d envs compared, worst |q - checker| %.2e rad; %d residuals, worst |err - float64| %.2e; "
          "%d envs further than %.0e rad from the neighbour's solution" % (N, single, n_cmp, worst_q, n_res, worst_res, n_far, 10 * IK_TOL))
    if single:
        assert n_cmp == sum(c[0][5] < 500 for c in cands) and n_cmp >= 0.7 * N
        if N > 1:
            assert n_far > N // 2              # an env-index slip would show: the neighbour's joints lead somewhere else
    else:
        assert n_cmp >= 0.9 * N
    assert n_res >= 0.7 * N


# ---------------------------------------------------------------------------------------------------------------- (b) plans
def _cases(single):
    return [c for c in json.load(open(FIXTURE))['cases'] if c['single_seed'] == single]


def _case_of_env(e, ncases):
    """Which fixture case env e holds: consecutive envs hold consecutive cases; the second block is shifted (by one for a list of
    four, by five for a list of ten) so that envs 0, 63, 64 and 69 hold four different cases (asserted where it is used)."""
    return (e + (e // 64) * (1 if ncases < 8 else 5)) % ncases


def plan_failures(plan, fingers, case):
    """Everything that is wrong with one env's [1000, 9] plan for one fixture case, as a list of strings (empty: the plan is
    right), and the worst joint difference from the fixture's rows and the worst float64 way-point residual."""
    bad = []
    if np.abs(plan[:100] - HOME2).max() > 1e-6 or np.abs(plan[800:900] - HOME2).max() > 1e-6 or np.abs(plan[900:]).max() > 1e-6:
        bad.append("constant rows")
    rows = case['rows']
    starts = [r['first_row'] for r in rows] + [800]
    if starts != [100, 200] + [250 + i * case['chunk'] for i in range(case['pieces'])] + [750, 800]:
        bad.append("fixture")
    if starts[-3] + case['chunk'] + 500 % case['pieces'] != 750:
        bad.append("fixture remainder")
    worst_q, worst_r = 0.0, 0.0
    for k, r in enumerate(rows):
        a, b = starts[k], starts[k + 1]
        if not (_bits(plan[a:b]) == _bits(plan[a])).all():
            bad.append("rows %d-%d are not one run" % (a, b - 1))
        want = np.array(r['q'])
        # a run boundary where the fixture's rows differ: the device's rows differ there too
        if k and np.abs(want - np.array(rows[k - 1]['q'])).max() > 2 * IK_TOL and np.array_equal(_bits(plan[a]), _bits(plan[a - 1])):
            bad.append("no run boundary at row %d" % a)
        d = np.abs(plan[a, :7].astype(np.float64) - want).max()
        worst_q = max(worst_q, d)
        if not d < IK_TOL:
            bad.append("row %d differs from the fixture by %.2e rad" % (a, d))
        q11 = np.zeros(11)
        q11[:7] = plan[a, :7]
        res = ee_residual(q11, r['target'], ORIENT)
        worst_r = max(worst_r, res)
        if not res < 1e-3 + RES_TOL:
            bad.append("row %d misses its way point: residual %.2e" % (a, res))
    if not (_bits(plan[100:800, 7:]) == _bits(fingers)).all():
        bad.append("finger columns")
    return bad, worst_q, worst_r


@pytest.mark.parametrize('single', [False, True])
def test_every_envs_whole_plan_against_the_recorded_float64_plans(single):
    """k_plan_macro, N = 70 (a full block and a partial one), every env from its own posture and fingers with its own pair: the
    whole [1000, 9] plan of EVERY env -- constants, run boundaries where the independent float64 count puts them, remainder rows,
    finger columns bit for bit, every distinct IK row to IK_TOL of the recorded float64 row and, by float64 FK, on its way point
    in position and orientation -- and the plan position back at row 0.  Negative control: held to its neighbour's case, every
    env fails."""
    cases = _cases(single)
    N = 70
    own = [_case_of_env(e, len(cases)) for e in range(N)]
    assert len({own[e] for e in (0, 63, 64, 69)}) == 4 and all(own[e] != own[(e + 1) % N] for e in range(N))
    assert set(own) == set(range(len(cases)))
    q0 = np.array([cases[c]['q_start'] for c in own], dtype=np.float32)
    macro = np.array([cases[c]['pair'] for c in own], dtype=np.float32)
    assert np.array_equal(macro.astype(np.float64), np.array([cases[c]['pair'] for c in own]))
    env = BatchedREALRobotEnv(N, objects=1, width=64, height=64, solver={'ik_single_seed': single})
    twin = BatchedREALRobotEnv(N, objects=1, width=64, height=64, solver={'ik_single_seed': single})
    # leave every env's plan position inside the IK rows of an earlier plan, so that "back at row 0" below says something
    env.plan_macro(np.tile(np.array([[-0.1, -0.2], [0.0, 0.2]], dtype=np.float32), (N, 1, 1)))
    for _ in range(150):
        env.step_plan()
    assert np.abs(env.get_plan(0)[150] - HOME2).max() > 0.1
    st = _set_postures(env, q0)
    env.plan_macro(macro)
    plans = np.stack([env.get_plan(e) for e in range(N)])
    worst_q, worst_r = 0.0, 0.0
    for e in range(N):
        bad, wq, wr = plan_failures(plans[e], st[e, 7:9], cases[own[e]])
        assert not bad, (e, cases[own[e]]['name'], bad)
        worst_q, worst_r = max(worst_q, wq), max(worst_r, wr)
        other = cases[own[(e + 1) % N]]
        assert plan_failures(plans[e], st[e, 7:9], other)[0], (e, "passes with the neighbour's case", other['name'])
        assert plan_failures(plans[e], st[(e + 1) % N, 7:9], cases[own[e]])[0] == ["finger columns"] or \
            np.array_equal(_bits(st[e, 7:9]), _bits(st[(e + 1) % N, 7:9]))
    print("k_plan_macro single_seed=%s: %d envs, %d cases, worst |row - float64 row| %.2e rad, worst float64 way-point residual %.2e"
          % (single, N, len(cases), worst_q, worst_r))
    # plan_step == 0 for every env: the next step_plan applies row 0 (home2), not row 150 of the earlier plan -- a twin with the
    # same continuation state that is handed row 0 through step() ends in the same state bit for bit
    twin.restore(env.checkpoint())
    env.step_plan()
    twin.step(plans[:, 0])
    a, b = env.state, twin.state
    env.close()
    twin.close()
    assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------- (c) mask, idle and clamp
def test_plan_mask_idle_and_clamp_are_bitwise_twins_of_plain_steps():
    """rr_plan_macro(env_mask) re-plans the masked envs only -- from the joints and fingers they have NOW, to start at row 0 --
    and leaves the others' plans and places alone; k_plan_fetch hands idle envs zeros and keeps their place, and repeats row 999
    past the end: handle A follows its plans on the device for 1005 steps under a seeded idle mask, handle B gets the same
    commands through step(cmd), built on the host from get_plan rows; their states are equal bit for bit.
    (The handles solve with ik_single_seed: every way point then starts from the env's current joints, so a plan made NOW cannot
    equal the plan made at reset.  With the default seeds it can, bit for bit: where the elbow-up seed wins the first way point,
    no later row depends on the current joints.)"""
    N = 5
    rng = np.random.default_rng(11)
    A, B, C = (BatchedREALRobotEnv(N, objects=1, width=64, height=64, solver={'ik_single_seed': True}) for _ in range(3))
    # (C stays at reset: what the new pairs give from there)
    q0 = np.zeros((N, 11), np.float32)
    q0[:, 7:] = rng.uniform(0.3, 1.2, (N, 1))                            # open fingers: still non-zero after 30 steps
    q0[:, :7] = rng.uniform(-0.2, 0.2, (N, 7))
    for h in (A, B):
        _set_postures(h, q0)
    first = np.array([[[-0.2, -0.3], [0.0, 0.1]], [[-0.1, 0.2], [-0.1, 0.2]], [[0.0, 0.0], [-0.2, -0.4]], [[-0.25, 0.4], [-0.05, -0.1]],
                      [[-0.15, 0.1], [-0.12, 0.12]]], dtype=np.float32)
    new = np.array([[[-0.1, 0.3], [-0.2, -0.2]], [[0.0, -0.1], [-0.2, 0.3]], [[-0.22, 0.1], [-0.05, 0.35]], [[-0.1, -0.3], [0.0, 0.2]],
                    [[-0.2, 0.2], [-0.1, -0.2]]], dtype=np.float32)
    A.plan_macro(first)
    plans = np.stack([A.get_plan(i) for i in range(N)])
    place = np.zeros(N, np.int64)

    def follow(idle=None):
        idle_b = np.zeros(N, bool) if idle is None else idle.astype(bool)
        cmd = plans[np.arange(N), np.minimum(place, 999)].copy()
        cmd[idle_b] = 0.0
        A.step_plan(idle=idle)
        B.step(cmd)
        place[~idle_b] += 1

    for _ in range(30):
        follow()
    now = A.state
    assert np.array_equal(_bits(now), _bits(B.state))
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    A.plan_macro(new, env_mask=mask)
    C.plan_macro(new)
    after = np.stack([A.get_plan(i) for i in range(N)])
    at_reset = np.stack([C.get_plan(i) for i in range(N)])
    C.close()
    for i in range(N):
        if not mask[i]:
            assert np.array_equal(_bits(after[i]), _bits(plans[i])), i                     # untouched plan
            continue
        assert np.abs(after[i][:100] - HOME2).max() < 1e-6 and np.abs(after[i][900:]).max() < 1e-6
        assert np.array_equal(_bits(after[i][100:800, 7:]), np.broadcast_to(_bits(now[i, 7:9]), (700, 2))), i     # the fingers it has now
        assert (now[i, 7:9] != 0).all() and not np.array_equal(_bits(now[i, 7:9]), _bits(q0[i, 7:9]))
        assert np.array_equal(_bits(at_reset[i][100:800, 7:]), np.zeros((700, 2), np.uint32))
        # made from the joints the env has now: not the plan the same pair gets at reset (the IK there starts from other joints)
        assert not np.array_equal(_bits(after[i][100:800, :7]), _bits(at_reset[i][100:800, :7])), i
        assert np.abs(after[i][100:800, :7] - plans[i][100:800, :7]).max() > 0.01           # and not the old pair's
    plans = after
    place[mask.astype(bool)] = 0                                                            # masked envs start over; the others keep their place
    checked = 0
    for t in range(1005):
        # (1005 steps for 1000 rows: an env that is to run into the clamp can only idle a few times -- the envs that started over
        # cannot get there anyway and idle often)
        follow(idle=(rng.random(N) < np.where(mask, 0.3, 0.02)).astype(np.uint8))
        if (t + 1) % 50 == 0 or t == 1004:
            assert np.array_equal(_bits(A.state), _bits(B.state)), t
            checked += 1
    assert checked == 21
    # the twin says something: envs started over and kept their place ended on different rows, and most ran into the clamp
    assert len(set(place.tolist())) > 1 and (place[~mask.astype(bool)] > 1000).any()
    print("plan positions after 30 + 1005 steps under the idle masks: %s (rows past 999 repeat row 999)" % place.tolist())
    A.close()
    B.close()
