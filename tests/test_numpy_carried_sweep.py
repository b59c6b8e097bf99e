"""CPU tests (-m "not gpu") of the float64 restatement of the swept clearance with carried objects (tests/numpy_carried_sweep.py) on
the committed fixture (tests/golden/carried_sweep.npz): the fixture holds the rows it was built for, the carried reach bounds every
profile, the restatement keeps the guarantees and is what the fixture recorded, env 0 is numpy_sweep's, each negative control breaks
a guarantee on some row, and no decision is borderline -- so the device and float64 can be compared row for row."""
import numpy as np
import pytest

from tests import numpy_carried_sweep as cs
from tests import numpy_collide as ncol
from tests import numpy_sweep as sw
from tests.test_gpu_carry import MEASURED_D
from tests.test_gpu_posture_query import TOL as TOL_D

SLACK = max(TOL_D, 4 * MEASURED_D)          # the distance ceiling of tests/test_gpu_carried_sweep.py


def test_fixture_has_its_shapes_its_pairs_and_its_rows():
    f = cs.fixture()
    Q = len(f['pairs'])
    assert f['states'].shape == (4, 61) and f['segments'].shape == (4, 8, 2, 11) and f['profile'].shape == (4, 8, cs.SAMPLES, Q) and 16 <= Q <= 20
    assert f['arm_nearest'].shape == (4, 8, cs.SAMPLES) and f['rel'].shape == f['rel_given'].shape == (4, 3, 7) and f['restated'].shape == (4, 8, 4)
    assert f['states'].dtype == f['segments'].dtype == f['rel_given'].dtype == np.float32 and f['profile'].dtype == f['rel'].dtype == np.float64
    assert f['safety'] == 0.01 and f['tolerance'] == 1e-3
    # the kinds of pairs, per env: carried x table, x shelf, x free object, x a shape on its own body, x a finger on another body, carried x carried, robot x static
    S, m = ncol.shapes(), cs.ns.model()
    kinds = set()
    for e in range(cs.N):
        car = cs.carried_pairs(f['pairs'], f['links'][e])
        M, _ = cs.masks_and_reach(f['pairs'], f['links'][e], f['rel'][e])
        for j, (a, b) in enumerate(f['pairs'].tolist()):
            held = [S[s]['kind'] == 2 and f['links'][e][S[s]['idx']] >= 0 for s in (a, b)]
            if car[j] and S[b]['kind'] == 0:
                kinds.add('carried x %s' % ('table' if b == 0 else 'shelf'))
            if sum(held) == 1 and S[b if held[0] else a]['kind'] == 2:
                kinds.add('carried x free object')
            if sum(held) == 1 and S[b if held[0] else a]['kind'] == 1:
                kinds.add('carried x own body' if not (M[j, 0] ^ M[j, 1]).any() else 'carried x finger on another body')
            if sum(held) == 2:
                kinds.add('carried x carried, one body' if not (M[j, 0] ^ M[j, 1]).any() else 'carried x carried, two bodies')
            if not car[j] and S[a]['kind'] == 1 and S[b]['kind'] == 0:
                kinds.add('robot x static')
    assert kinds == {'carried x table', 'carried x shelf', 'carried x free object', 'carried x own body', 'carried x finger on another body',
                     'carried x carried, one body', 'carried x carried, two bodies', 'robot x static'}, kinds
    cls = cs.classes()
    carried_env = lambda c: [r for r, v in cls.items() if c in v and r[0] > 0]
    assert len(carried_env('carried_hits_arm_free')) >= 6 and len(carried_env('tunnel')) >= 3 and len(carried_env('free')) >= 3 and len(carried_env('start_in_collision')) >= 3
    for e, k in carried_env('tunnel'):          # both ends free by more than 1 cm, the interior negative
        d = f['profile'][e, k].min(axis=1)
        assert d[0] > f['safety'] + 1e-2 and d[-1] > f['safety'] + 1e-2 and d[1:-1].min() < 0


def test_carried_reach_bounds_the_rate_of_every_profile():
    f = cs.fixture()
    worst = 0.0
    for e, k in cs.ROWS:
        B = cs.pair_bounds(f['segments'][e, k, 1].astype(np.float64) - f['segments'][e, k, 0], f['pairs'], f['links'][e], f['rel'][e])
        ratio, still = sw.rate_ratio(f['profile'][e, k], B)
        worst = max(worst, ratio)
        assert ratio <= 1.0 and still <= 1e-12, (e, k, ratio, still)          # (B = 0: the carried x own-body pair among them does not move)
    print('largest |delta d| / (delta t B) over the fixture: %.3f' % worst)
    assert worst > 0.5
    e = 1                                                                      # without the carried masks the cube's pairs would have no bound at all
    B = sw.pair_bounds(f['segments'][e, 2, 1].astype(np.float64) - f['segments'][e, 2, 0], f['pairs'])
    assert B[cs.carried_pairs(f['pairs'], f['links'][e])][:3].max() == 0.0


@pytest.mark.parametrize('e', range(cs.N))
def test_restatement_keeps_the_guarantees_and_is_the_recorded_one(e):
    f = cs.fixture()
    cls = cs.classes()
    for k in range(cs.K):
        r = cs.run(e, k)
        bad, slack = sw.violations(r, f['profile'][e, k], f['safety'])
        print('row (%d, %d) %s: status %d fraction %.4f pair %d steps %d evaluations %d, smallest covered d - safety %.4g'
              % (e, k, ','.join(sorted(cls[e, k])), r['status'], r['fraction'], r['pair'], r['steps'], r['evaluations'], slack))
        assert bad == 0, (e, k, bad, slack)
        assert [r['status'], r['pair'], r['steps'], r['evaluations']] == f['restated'][e, k].tolist()
        assert r['steps'] < sw.MAX_STEPS and r['status'] in (0, 1)
        if 'free' in cls[e, k]:
            assert r['status'] == 0 and r['fraction'] == 1.0 and r['pair'] == -1 and (r['free'] == 1.0).all()
        if 'tunnel' in cls[e, k] or 'hit_midway' in cls[e, k]:
            assert r['status'] == 1 and 0.0 < r['fraction'] < 1.0
        if 'start_in_collision' in cls[e, k]:
            assert r['status'] == 1 and r['fraction'] == 0.0 and r['steps'] == 1
        if 'carried_hits_arm_free' in cls[e, k]:          # the carried object hits, the arm alone (numpy_sweep.advance on the same segment) is free
            # (without the device's step cap: the cube left at the finger tips keeps numpy_sweep's steps short, and the question is "free", not "how fast")
            alone = sw.advance(f['states'][e], f['segments'][e, k, 0], f['segments'][e, k, 1], f['pairs'], f['safety'], f['tolerance'], max_steps=4096)
            assert r['status'] == 1 and cs.carried_pairs(f['pairs'], f['links'][e])[r['pair']] and alone['status'] == 0, (e, k, alone['status'])
        if r['status'] == 1:
            assert cs.lower_bounds(f['states'][e], r['q_stop'], f['pairs'][r['pair']:r['pair'] + 1], f['links'][e], f['rel'][e])[0] <= f['safety'] + f['tolerance']
        if e == 0:                                         # nothing attached: numpy_sweep's advancement, number for number
            o = sw.advance(f['states'][e], f['segments'][e, k, 0], f['segments'][e, k, 1], f['pairs'], f['safety'], f['tolerance'])
            assert all(np.array_equal(np.asarray(o[key]), np.asarray(r[key])) for key in ('status', 'fraction', 'pair', 'steps', 'evaluations', 'free', 'q_stop'))


@pytest.mark.parametrize('control', cs.CONTROLS)
def test_every_control_breaks_a_guarantee(control):
    f = cs.fixture()
    broken = []
    for e, k in ((1, 2), (2, 2), (3, 2)):                  # the tunnel rows of the three carrying envs
        r = cs.run(e, k, control)
        bad, slack = sw.violations(r, f['profile'][e, k], f['safety'])
        print('%s on row (%d, %d): status %d fraction %.4f steps %d, %d covered samples at or below safety, worst d - safety %.4g'
              % (control, e, k, r['status'], r['fraction'], r['steps'], bad, slack))
        broken.append(bad > 0)
    assert any(broken)


@pytest.mark.parametrize('e', range(cs.N))
def test_no_decision_is_borderline(e):
    """Every B scaled by 1 +- 1e-5 and every lower bound moved by -+ the distance ceiling (the two extremes: the longest and the
    shortest steps a device within those bounds could take) changes no row's status or step count."""
    f = cs.fixture()
    for k in range(cs.K):
        for scale, shift in ((1.0 + 1e-5, -SLACK), (1.0 - 1e-5, SLACK)):
            r = cs.run(e, k, None, scale, shift)
            assert [r['status'], r['steps']] == f['restated'][e, k, [0, 2]].tolist(), (e, k, scale, shift, r['status'], r['steps'])
