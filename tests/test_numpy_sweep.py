"""CPU tests (-m "not gpu") of the float64 restatement of the swept clearance (tests/numpy_sweep.py) on the committed fixture
(tests/golden/swept_clearance.npz): the fixture holds the classes it was built for, the reach table bounds every profile, the
restatement keeps the header's guarantees and decides every short row well inside the step cap, and each negative control breaks a
guarantee on some row -- so a device test that holds the kernel to these guarantees can tell a wrong kernel from a right one."""
import numpy as np
import pytest

from tests import numpy_sweep as sw

ROWS = [(e, k) for e in range(3) for k in range(8)]


def _classes():
    f = sw.fixture()
    return {(e, k): sw.classify(f['profile'][e, k], f['segments'][e, k].astype(np.float64), f['safety']) for e, k in ROWS}


def test_fixture_has_its_shapes_and_at_least_two_rows_of_every_class():
    f = sw.fixture()
    Q = len(f['pairs'])
    assert f['states'].shape == (3, 61) and f['segments'].shape == (3, 8, 2, 11) and f['profile'].shape == (3, 8, sw.SAMPLES, Q) and 16 <= Q <= 20
    assert f['states'].dtype == f['segments'].dtype == np.float32 and f['profile'].dtype == np.float64
    assert f['safety'] == 0.01 and f['tolerance'] == 1e-3
    cls = _classes()
    for c in sw.CLASSES:
        assert sum(c in v for v in cls.values()) >= 2, c
    zero = [r for r, v in cls.items() if 'zero_length' in v]
    assert any('free' in cls[r] for r in zero) and any('start_in_collision' in cls[r] for r in zero)
    for (e, k), v in cls.items():
        span = np.abs(f['segments'][e, k, 1].astype(np.float64) - f['segments'][e, k, 0]).max()
        assert (span >= 2.0) if 'long' in v else (span <= 0.5 + 1e-6), (e, k, span)
    # the table: a link x link pair that shares ancestors, an object x table pair that nothing moves
    M = sw.joint_masks()
    assert any((M[a] & M[b]).any() and (M[a] ^ M[b]).any() for a, b in f['pairs'].tolist())
    assert any(not M[a].any() and not M[b].any() for a, b in f['pairs'].tolist())


def test_reach_table_bounds_the_rate_of_every_profile():
    f = sw.fixture()
    R = sw.reach_table()
    assert R.shape == (11, len(sw.joint_masks())) and (R >= 0).all() and ((R > 0) == sw.joint_masks().T).all()
    worst = 0.0
    for e, k in ROWS:
        B = sw.pair_bounds(f['segments'][e, k, 1].astype(np.float64) - f['segments'][e, k, 0], f['pairs'])
        ratio, still = sw.rate_ratio(f['profile'][e, k], B)
        worst = max(worst, ratio)
        assert ratio <= 1.0 and still <= 1e-12, (e, k, ratio, still)
    print('largest |delta d| / (delta t B) over the fixture: %.3f' % worst)
    assert worst > 0.5          # (a fixture in which no profile comes near its bound could not catch a bound that is too small)


@pytest.mark.parametrize('e', range(3))
def test_restatement_keeps_the_guarantees_and_decides_short_rows_in_half_the_cap(e):
    f = sw.fixture()
    cls = _classes()
    for k in range(8):
        if 'long' in cls[e, k]:
            continue
        r = sw.run(e, k)
        bad, slack = sw.violations(r, f['profile'][e, k], f['safety'])
        print('row (%d, %d) %s: status %d fraction %.4f pair %d steps %d evaluations %d, smallest covered d - safety %.4g'
              % (e, k, ','.join(sorted(cls[e, k])), r['status'], r['fraction'], r['pair'], r['steps'], r['evaluations'], slack))
        assert bad == 0, (e, k, bad, slack)
        assert r['steps'] <= sw.MAX_STEPS // 2 and r['status'] in (0, 1), (e, k, r['steps'], r['status'])
        if 'free' in cls[e, k]:
            assert r['status'] == 0 and r['fraction'] == 1.0 and r['pair'] == -1 and (r['free'] == 1.0).all()
        if 'tunnel' in cls[e, k] or 'hit_midway' in cls[e, k]:
            assert r['status'] == 1 and 0.0 < r['fraction'] < 1.0
        if 'start_in_collision' in cls[e, k]:
            assert r['status'] == 1 and r['fraction'] == 0.0 and r['steps'] == 1
        if r['status'] == 1:          # tight: the reported pair is within safety + tolerance where the row stopped
            assert sw.lower_bounds(f['states'][e], r['q_stop'], f['pairs'][r['pair']:r['pair'] + 1])[0] <= f['safety'] + f['tolerance']


def test_long_row_keeps_the_guarantees_within_the_cap():
    f = sw.fixture()
    r = sw.run(2, 6)
    bad, slack = sw.violations(r, f['profile'][2, 6], f['safety'])
    print('row (2, 6): status %d fraction %.4f steps %d evaluations %d, smallest covered d - safety %.4g' % (r['status'], r['fraction'], r['steps'], r['evaluations'], slack))
    assert bad == 0 and r['steps'] <= sw.MAX_STEPS and r['status'] in (0, 1, 3)


@pytest.mark.parametrize('control,rows', [('bound_halved', ((2, 1), (2, 2))), ('common_ancestors_counted_twice_ignored', ((0, 7), (2, 7))),
                                          ('end_postures_only', ((0, 2), (1, 2), (2, 2)))])
def test_every_control_breaks_a_guarantee(control, rows):
    f = sw.fixture()
    cls = _classes()
    broken = []
    for e, k in rows:
        r = sw.run(e, k, control)
        bad, slack = sw.violations(r, f['profile'][e, k], f['safety'])
        print('%s on row (%d, %d): status %d fraction %.4f steps %d, %d covered samples at or below safety, worst d - safety %.4g'
              % (control, e, k, r['status'], r['fraction'], r['steps'], bad, slack))
        broken.append(bad > 0)
        if control == 'end_postures_only':
            assert 'tunnel' in cls[e, k] and bad > 0 and r['status'] == 0      # every tunnel row catches it
    assert any(broken)
