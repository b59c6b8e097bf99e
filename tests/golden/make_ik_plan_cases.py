#!/usr/bin/env python3
"""Generates tests/golden/ik_plan_cases.json: macro plans of the float64 checker (oracle/kinematics.py) for CASES of
(start joints [11], macro pair, single_seed) -- the rows that tests/test_gpu_ik_plans.py holds every env's device plan
(k_plan_macro, rr_ik.inc) to, row by row, without re-running the numpy solver on the GPU machine.

Per case: the inputs (the pair rounded to float32 first, as plan_macro does), the float64 segment count of the rounded pair, the
distinct IK rows in the order they are solved (above p1, at p1, the end of every p1 -> p2 segment, above p2) with the first plan
row of each, and per row the residual, the number of DLS updates and the winner's lead over the runner-up.

Cases cover what the segment arithmetic of the plan can get wrong: p1 == p2 (one piece), distances of 0.04 (1 piece, chunk 500),
0.06 (2 pieces, chunk 250) and 0.33 (7 pieces, chunk 71: rows 747-749 are remainder rows), a pair from one long edge of the
action space to the other (21 pieces, as many as the longest diagonal has -- whose corner (0.05, +-0.5) the arm does not reach:
every seed ends 6.8e-3 from it at z 0.46 and 6.2e-2 at z 0.6, so it cannot meet the first condition below) and ordinary pairs; from the reset posture and from drawn postures inside the joint limits with non-zero, distinct fingers; with the
default seeds and with single_seed.

A drawn case is REJECTED unless the float64 solve of every way point is far from every decision a float32 solver could take
differently -- properties of the checker alone, nothing is tuned on the device:
  * residual: the winning run's residual is < 1e-3;
  * lead: the winner's key leads the runner-up's by >= 1e-3 (the tests' IK_TOL: the most by which a row may differ at all), and
    no losing run's residual lies within a factor two of the 1e-2 that decides "converged" in the selection.  (A lead of 1e-2
    does not exist with this solver: from the second way point on, the run seeded with the previous way point and the run
    seeded elbow-up end 0.02-0.1 rad apart with keys that tie to a few 1e-3 -- the key, the largest joint distance from the
    previous way point, is set by the joint that has to travel; the best least lead of 800 drawn plans was 3.7e-3.)
  * threshold: neither of the last two residuals of any run that takes part in the selection lies within 2e-5 of 1e-3 (where
    the two precisions may stop one update apart);
  * iterations: the winning run stops before update 500 of 1000;
  * pieces: |dist / 0.05 - nearest positive integer| >= 1e-3 (the segment count does not hang on rounding).
So a test may compare EVERY row of a case.  The script prints how many draws it rejected and why.

Run here (CPU only, well under a minute on 8 cores):  python tests/golden/make_ik_plan_cases.py
"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.kinematics import ik_candidates, plan_way_points, quat_from_euler, segment_count     # noqa: E402

PATH = os.path.join(ROOT, 'tests', 'golden', 'ik_plan_cases.json')
ORIENT = quat_from_euler(0, 3.14, -1.57)
ARM_LIMIT = np.array([2.96, 2.09, 2.96, 2.09, 2.96, 2.09, 3.05])       # rad, the arm's joint limits
LEAD, NEAR, MAX_ITERS, PIECES_MARGIN = 1e-3, 2e-5, 500, 1e-3
BOX = ((-0.25, 0.05), (-0.5, 0.5))                                      # the macro action space (x, y)

# (name, posture, pair kind, single_seed): posture 'reset' or 'drawn'; pair kind a distance, 'diagonal' or 'ordinary'
CASES = [('reset_same_point', 'reset', 0.0, False), ('reset_0.33', 'reset', 0.33, False), ('reset_ordinary', 'reset', 'ordinary', False),
         ('drawn_same_point', 'drawn', 0.0, False), ('drawn_0.04', 'drawn', 0.04, False), ('drawn_0.06', 'drawn', 0.06, False),
         ('drawn_0.33', 'drawn', 0.33, False), ('drawn_long', 'drawn', 'long', False), ('drawn_ordinary', 'drawn', 'ordinary', False),
         ('reset_0.06', 'reset', 0.06, False),
         ('single_same_point', 'drawn', 0.0, True), ('single_0.06', 'drawn', 0.06, True), ('single_0.33', 'drawn', 0.33, True),
         ('single_ordinary', 'reset', 'ordinary', True)]


def pieces_margin(pair):
    """Distance of dist / 0.05 from the nearest POSITIVE integer, float64 on the inputs as given (the count int(x) + 1 steps at
    1, 2, ...; it does not step at 0, where x >= 0 cannot round to the other side: p1 == p2 gives x = 0 in any precision)."""
    x = np.linalg.norm(np.asarray(pair[1], dtype=np.float64) - np.asarray(pair[0], dtype=np.float64)) / 0.05
    return abs(x - max(round(x), 1))


def trace_plan(q_start, pair, single_seed):
    """Solves the way points of one plan like generate_plan does (each one from q_start, preferring the previous solution) and
    keeps what the conditions need.  Returns (rows, None) or (None, the name of the first condition that failed)."""
    if pieces_margin(pair) < PIECES_MARGIN:
        return None, 'pieces'
    rows, last = [], None
    for first_row, target in plan_way_points(pair):
        cands = ik_candidates(q_start, target, ORIENT, prefer=last, single_seed=single_seed)
        keys = [(c[1] < 1e-2, c[2]) for c in cands]
        w = max(range(len(cands)), key=lambda i: (keys[i], -i))            # the first of equal keys wins, as in inverse_kinematics
        q, err, key, _, prev_err, iters = cands[w]
        if not err < 1e-3:
            return None, 'residual'
        others = [c for i, c in enumerate(cands) if i != w]
        if any(5e-3 < c[1] < 2e-2 for c in others):
            return None, 'lead'
        lead = min([key - c[2] for c in others if c[1] < 1e-2], default=np.inf)
        if lead < LEAD:
            return None, 'lead'
        # (the band holds for every run that takes part in the selection: a runner-up that stops one update apart moves its key
        # by the size of that update, far more than LEAD)
        if any(c[1] > 1e-3 - NEAR or abs(c[4] - 1e-3) < NEAR for c in cands if c[1] < 1e-2):
            return None, 'threshold'
        if iters >= MAX_ITERS:
            return None, 'iterations'
        rows.append(dict(first_row=first_row, target=[float(v) for v in target], q=[float(v) for v in q[:7]], residual=float(err),
                         updates=int(iters), lead=None if np.isinf(lead) else float(lead)))
        last = q
    return rows, None


def draw_posture(rng):
    q = np.zeros(11)
    q[:7] = rng.uniform(-0.5, 0.5, 7) * ARM_LIMIT
    q[7:] = rng.uniform(0.05, 1.5, 4)                                      # non-zero, distinct fingers
    return q


def draw_pair(rng, kind):
    if kind == 'long':                                                      # one long edge to the other: 1.0 <= dist < 1.05, 21 pieces
        return [[rng.uniform(-0.25, -0.1), -0.5], [rng.uniform(-0.25, -0.1), 0.5]]
    while True:
        p1 = np.array([rng.uniform(*BOX[0]), rng.uniform(*BOX[1])])
        if kind == 'ordinary':
            p2 = np.array([rng.uniform(*BOX[0]), rng.uniform(*BOX[1])])
        else:
            a = rng.uniform(0, 2 * np.pi)
            p2 = p1 + kind * np.array([np.cos(a), np.sin(a)])
        if kind == 'ordinary' and np.linalg.norm(p2 - p1) < 0.1:
            continue
        if BOX[0][0] <= p2[0] <= BOX[0][1] and BOX[1][0] <= p2[1] <= BOX[1][1]:
            return [p1.tolist(), p2.tolist()]


def make_case(index, seed=2020):
    """Case `index` of CASES from its own random stream (so the cases can be drawn in parallel): (case, rejected draws by reason)."""
    name, posture, kind, single = CASES[index]
    rng = np.random.default_rng([seed, index])
    rejected = {}
    for attempt in range(2000):
        q0 = np.zeros(11) if posture == 'reset' else draw_posture(rng)
        pair = np.array(draw_pair(rng, kind), dtype=np.float32).astype(np.float64)       # rounded to float32 as plan_macro does
        rows, why = trace_plan(q0, pair, single)
        if rows is not None:
            break
        rejected[why] = rejected.get(why, 0) + 1
    else:
        raise SystemExit("no admissible draw for case %s: %s" % (name, rejected))
    pieces = segment_count(pair[0], pair[1])
    return dict(name=name, single_seed=single, q_start=[float(v) for v in q0], pair=pair.tolist(), pieces=int(pieces),
                chunk=500 // pieces, rows=rows), rejected


def make_cases():
    with mp.get_context('spawn').Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(make_case, range(len(CASES)), chunksize=1)
    rejected = {}
    for _, rj in res:
        for k, v in rj.items():
            rejected[k] = rejected.get(k, 0) + v
    return [c for c, _ in res], dict(sorted(rejected.items()))


def main():
    cases, rejected = make_cases()
    out = dict(orientation_xyzw=[float(v) for v in ORIENT],
               conditions=dict(residual=1e-3, lead=LEAD, threshold_band=NEAR, max_updates=MAX_ITERS, pieces_margin=PIECES_MARGIN),
               rejected_draws=rejected, cases=cases)
    with open(PATH, 'w') as f:
        json.dump(out, f, indent=0)
    print("%d cases, %d rows; rejected draws: %s" % (len(cases), sum(len(c['rows']) for c in cases), rejected or "none"))
    for c in cases:
        print("  %-18s pieces %2d chunk %3d  worst residual %.2e  most updates %3d  least lead %s" % (
            c['name'], c['pieces'], c['chunk'], max(r['residual'] for r in c['rows']), max(r['updates'] for r in c['rows']),
            min([r['lead'] for r in c['rows'] if r['lead'] is not None], default=None)))


if __name__ == '__main__':
    main()
