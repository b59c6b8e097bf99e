"""Host checks (no GPU) of tests/golden/ik_plan_cases.json -- the float64 plans that tests/test_gpu_ik_plans.py holds the device's
plans to -- and of the segment count of a macro plan in the two precisions."""
import importlib.util
import json
import os

import numpy as np

from oracle.kinematics import plan_way_points, segment_count

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'ik_plan_cases.json')
ARM_LIMIT = np.array([2.96, 2.09, 2.96, 2.09, 2.96, 2.09, 3.05])


def _generator():
    spec = importlib.util.spec_from_file_location('make_ik_plan_cases', os.path.join(HERE, 'golden', 'make_ik_plan_cases.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def perimeter_pairs():
    pts = [(a, b) for a in (-0.25, 0.05) for b in (-0.5, 0.0, 0.5)]
    return [(p1, p2) for p1 in pts for p2 in pts]


def pieces_float32(pair):
    """k_plan_macro's arithmetic (rr_ik.inc): every operation in float32 on the float32 inputs."""
    p = np.asarray(pair, dtype=np.float32)
    dx, dy = p[1, 0] - p[0, 0], p[1, 1] - p[0, 1]
    dist = np.sqrt(dx * dx + dy * dy, dtype=np.float32)
    assert dist.dtype == np.float32
    return min(int(dist / np.float32(0.05)) + 1, 500)


def pieces_float64_on_float32(pair):
    """The checker's arithmetic (float64) on what plan_macro hands the device (the pair rounded to float32)."""
    p = np.asarray(pair, dtype=np.float32).astype(np.float64)
    return segment_count(p[0], p[1])


def perimeter_segment_counts():
    """Segments of the p1 -> p2 rows for the reference script's 36 pairs, as the device cuts them."""
    return [pieces_float64_on_float32(pr) for pr in perimeter_pairs()]


def test_fixture_cases_cover_the_segment_arithmetic_and_keep_their_margins():
    fx = json.load(open(FIXTURE))
    cases = fx['cases']
    assert os.path.getsize(FIXTURE) < 100 * 1024
    default = [c for c in cases if not c['single_seed']]
    single = [c for c in cases if c['single_seed']]
    assert len(default) >= 10 and len(single) >= 4
    assert {1, 2, 7, 21} <= {c['pieces'] for c in default}
    gen = _generator()
    dists = []
    for c in cases:
        pair = np.array(c['pair'])
        assert np.array_equal(pair.astype(np.float32).astype(np.float64), pair), c['name']       # float32 values, as plan_macro passes them
        assert (pair[:, 0] >= -0.25).all() and (pair[:, 0] <= np.float32(0.05)).all() and (np.abs(pair[:, 1]) <= 0.5).all()
        dist = np.linalg.norm(pair[1] - pair[0])
        dists.append(dist)
        assert gen.pieces_margin(pair) >= 1e-3, c['name']
        assert c['pieces'] == int(dist / 0.05) + 1 == pieces_float32(pair) == pieces_float64_on_float32(pair), c['name']
        assert c['chunk'] == 500 // c['pieces']
        way = plan_way_points(pair)
        assert [r['first_row'] for r in c['rows']] == [w[0] for w in way] == [100, 200] + [250 + i * c['chunk'] for i in range(c['pieces'])] + [750]
        assert np.abs(np.array([r['target'] for r in c['rows']]) - np.array([w[1] for w in way])).max() < 1e-15
        for r in c['rows']:
            assert r['residual'] < 1e-3 - 2e-5 and r['updates'] < 500, (c['name'], r['first_row'])
            assert r['lead'] is None or r['lead'] >= 1e-3, (c['name'], r['first_row'])
        assert all((r['lead'] is None) == c['single_seed'] for r in c['rows'])
        q0 = np.array(c['q_start'])
        assert (np.abs(q0[:7]) <= ARM_LIMIT).all()
    dists = np.array(dists)
    assert (dists == 0).sum() >= 2                                       # p1 == p2
    for d, pieces in ((0.04, 1), (0.06, 2), (0.33, 7)):
        hit = [c for c, dd in zip(cases, dists) if abs(dd - d) < 1e-6]
        assert hit and all(c['pieces'] == pieces for c in hit), d
    assert any(c['pieces'] == 7 and c['chunk'] == 71 and 250 + 7 * 71 == 747 for c in default)      # rows 747-749: remainder
    # postures: the reset posture, and at least two others with non-zero, distinct fingers
    starts = np.array([c['q_start'] for c in cases])
    assert (np.abs(starts).max(1) == 0).any()
    moved = starts[np.abs(starts[:, :7]).max(1) > 0.1]
    assert len({tuple(q) for q in moved}) >= 2 and len({tuple(q) for q in starts[[not c['single_seed'] for c in cases]]}) >= 3
    for q in moved:
        assert (q[7:] > 0).all() and len(set(q[7:])) == 4


def test_cheapest_case_recomputes_to_1e_12():
    fx = json.load(open(FIXTURE))
    c = next(c for c in fx['cases'] if c['name'] == 'reset_same_point')
    assert c['pair'][0] == c['pair'][1] and c['pieces'] == 1 and len(c['rows']) == 4
    rows, why = _generator().trace_plan(np.array(c['q_start']), np.array(c['pair']), c['single_seed'])
    assert why is None
    assert np.abs(np.array([r['q'] for r in rows]) - np.array([r['q'] for r in c['rows']])).max() < 1e-12
    assert np.abs(np.array([r['residual'] for r in rows]) - np.array([r['residual'] for r in c['rows']])).max() < 1e-12
    assert [r['updates'] for r in rows] == [r['updates'] for r in c['rows']]


def test_segment_counts_float32_equals_float64_on_float32_inputs():
    """The device counts the segments in float32 (k_plan_macro); float64 arithmetic on the same float32 inputs gives the same
    count for every fixture pair and for the reference script's 36 perimeter pairs -- the count depends on the rounding of the
    INPUTS only.  With exact float64 inputs (the reference, env.py:433) the six pairs at distance 0.3 get 6 segments, because
    0.3 / 0.05 is 5.999999999999999 in float64; the float32 inputs give 7 (a known, harmless deviation)."""
    fx = json.load(open(FIXTURE))
    for c in fx['cases']:
        assert pieces_float32(c['pair']) == pieces_float64_on_float32(c['pair']) == c['pieces']
    pairs = perimeter_pairs()
    table = perimeter_segment_counts()
    assert [pieces_float32(pr) for pr in pairs] == table
    exact = [segment_count(np.array(p1), np.array(p2)) for p1, p2 in pairs]
    at_03 = [i for i, (p1, p2) in enumerate(pairs) if p1[1] == p2[1] and p1[0] != p2[0]]
    assert len(at_03) == 6
    for i, (p1, p2) in enumerate(pairs):
        dy, dx = abs(p1[1] - p2[1]), p1[0] != p2[0]
        # (0, 0.5, 1.0 along y; 0.3 across: sqrt(0.09 + 0.25) = 0.583 -> 12, sqrt(0.09 + 1) = 1.044 -> 21)
        want = {(0.0, False): 1, (0.5, False): 11, (1.0, False): 21, (0.0, True): 7, (0.5, True): 12, (1.0, True): 21}[(dy, dx)]
        assert table[i] == want, (p1, p2)
        assert exact[i] == (6 if i in at_03 else want), (p1, p2)
    assert [table[i] for i in at_03] == [7] * 6 and [exact[i] for i in at_03] == [6] * 6


def test_the_seeded_ik_draw_converges_for_the_checker_alone():
    """The shares tests/test_gpu_ik_plans.py asks of the device hold for the float64 checker on the same seeded draw: the
    single-seed solve from every env's own joints converges before update 500 for at least 70 % of the envs (here: all), and a
    default-mode candidate converges for at least 90 %."""
    from tests.test_gpu_ik_plans import ik_shares
    for n in (70, 1):
        single, default = ik_shares(n)
        assert single >= 0.7 and default >= 0.9, (n, single, default)
    assert ik_shares(70) == (1.0, 1.0)
