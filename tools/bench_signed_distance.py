#!/usr/bin/env python3
"""Cost and accuracy of rr_signed_distance on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; the
present state and K in {1, 8, 32} candidate postures per env drawn around each env's own (sigma 0.1 rad); the pair tables `fingers8`
(the four finger pads x cube and tomato, Q = 8) and `collision` (the step's whole collision table, Q = 92).  Per (table, form):
WARMUP calls, then REPS windows of back-to-back calls on the library's stream between two HIP events; the median window gives the
microseconds per call.  Beside each, on the same handle in the same process and timed the same way, the query that stops at the
surface: rr_closest_points for the present state, rr_posture_clearance for the postures.

Also, per (table, form), the share of overlapping items, the status counts (status 5: the expansion's caps), the histogram of
expansion trips and of polytope faces in use when the search ended -- a closed triangulated polytope of V vertices has 2 V - 4 faces
and a trip that goes on adds one vertex, so an item that ended in trip t had 4 + 2 (t - 1) faces --, and the accuracy on the seeded
cases of tests/test_gpu_signed_distance.py: the largest |-signed - exact depth| over their decided overlapping items against
tests/numpy_penetration.py (the MEASURED of that test, and TOL_SD = 4 x).

    python tools/bench_signed_distance.py [--out FILE.json] [--label TEXT] [--no-accuracy] [--controls]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped: a workgroup per row, a wave per pair, GJK then the expansion with a face per lane')
ap.add_argument('--no-accuracy', action='store_true')
ap.add_argument('--controls', action='store_true', help='also compute the negative controls of the seeded cases (CPU, about a minute)')
ap.add_argument('--reps', type=int, default=11)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, T0, WARMUP, KS = 4096, 170, 3, (1, 8, 32)
TABLES = {'fingers8': [(pad, obj) for obj in ('cube', 'tomato') for pad in ('skin_00', 'skin_01', 'skin_10', 'skin_11')], 'collision': 'collision'}

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
state = env.state
rng = np.random.default_rng(7)


def windows(fn, calls):
    """median / min / max microseconds per call over the windows"""
    for _ in range(WARMUP):
        fn()
    env.sync()
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return {"us_per_call_median": round(float(np.median(us)), 2), "us_per_call_min": round(float(min(us)), 2), "us_per_call_max": round(float(max(us)), 2)}


def workload(out):
    """what the items of one call were: statuses, the share of overlapping items, trips and faces"""
    st, ex, it = np.array(out['pair_status']), np.array(out['pair_expansions']), np.array(out['pair_iterations'])
    over = np.isin(st, (1, 5))
    trips = ex[over].astype(np.int64)
    hist = np.bincount(trips, minlength=33)
    return {"items": int(st.size), "status_counts": {str(s): int((st == s).sum()) for s in range(6)}, "overlapping_share": round(float(over.mean()), 5),
            "status5_items": int((st == 5).sum()), "mean_gjk_iterations": round(float(it.mean()), 2),
            "expansion_trips_histogram": {str(t): int(c) for t, c in enumerate(hist) if c},
            "faces_in_use_histogram": {str(4 + 2 * (t - 1)): int(c) for t, c in enumerate(hist) if c and t >= 1},
            "mean_expansion_trips": round(float(trips.mean()), 2) if trips.size else 0.0, "max_expansion_trips": int(trips.max()) if trips.size else 0}


res = {"label": args.label, "envs": N, "state": "step %d of synthetic_actions" % T0, "windows": args.reps, "posture_sigma_rad": 0.1, "tables": {}}
for name, pairs in TABLES.items():
    env.set_distance_pairs(pairs)
    Q = len(env.distance_pairs()[0])
    cp = windows(env.closest_points, 20)
    sd = windows(env.signed_distance, 20)
    row = {"calls_per_window": 20, "signed_distance": dict(sd, ns_per_pair=round(sd["us_per_call_median"] * 1e3 / (N * Q), 3)),
           "closest_points": dict(cp, ns_per_pair=round(cp["us_per_call_median"] * 1e3 / (N * Q), 3)),
           "signed_over_surface_query": round(sd["us_per_call_median"] / cp["us_per_call_median"], 3)}
    row.update(workload(env.signed_distance(host=True)))
    res["tables"][name] = {"Q": Q, "present": row, "K": {}}
    print(name, 'present', json.dumps(row), flush=True)
    for K in KS:
        po = (state[:, None, :11] + rng.normal(0.0, 0.1, size=(N, K, 11))).astype(np.float32)
        with torch.cuda.stream(stream):
            dev_po = torch.from_numpy(po).cuda()
        stream.synchronize()
        calls = max(2, 20 // K)
        pc = windows(lambda: env.posture_clearance(dev_po), calls)
        sd = windows(lambda: env.signed_distance(dev_po), calls)
        row = {"calls_per_window": calls, "signed_distance": dict(sd, ns_per_posture_pair=round(sd["us_per_call_median"] * 1e3 / (N * K * Q), 3)),
               "posture_clearance": dict(pc, ns_per_posture_pair=round(pc["us_per_call_median"] * 1e3 / (N * K * Q), 3)),
               "signed_over_surface_query": round(sd["us_per_call_median"] / pc["us_per_call_median"], 3)}
        row.update(workload(env.signed_distance(dev_po, host=True)))
        res["tables"][name]["K"][str(K)] = row
        print(name, 'K', K, json.dumps(row), flush=True)
assert env.state.tobytes() == state.tobytes()                             # no query wrote the state
env.close()
if not args.no_accuracy:
    from tests import numpy_penetration as pen
    from tests import numpy_posture as npo
    worst, items, trips = {}, 0, 0
    for name in pen.CASES:
        ref, pairs = pen.case(name)
        rows, cols = pen.overlapping(ref)
        if name == 'R':
            st, po, _ = npo.case_r_inputs()
            e = BatchedREALRobotEnv(4, objects=3, width=64, height=64)
            e.state = st
            e.set_distance_pairs(pairs)
            out = {k: np.array(v).reshape((16,) + np.array(v).shape[2:]) for k, v in e.signed_distance(po, host=True).items()}
        else:
            from tests import numpy_distance as nd
            st = nd.case(int(name))[0]
            e = BatchedREALRobotEnv(len(st), objects=3, width=64, height=64)
            e.state = st
            e.set_distance_pairs(pairs)
            out = {k: np.array(v) for k, v in e.signed_distance(host=True).items()}
        e.close()
        worst[name] = float(np.abs(-out['pair_distance'][rows, cols].astype(np.float64) + ref['d'][rows, cols]).max())
        items += len(rows)
        trips = max(trips, int(out['pair_expansions'][rows, cols].max()))
        assert (out['pair_status'][rows, cols] == 1).all(), name
    measured = max(worst.values())
    res["accuracy"] = {"cases": "1: N=1 Q=92; 5: N=5 Q=7; R: N=4 K=4 Q=80", "decided_overlapping_items": items, "max_abs_depth_error_m_by_case": worst,
                       "measured_max_abs_depth_error_m": measured, "tol_sd_m": 4 * measured, "status5_items": 0, "max_expansion_trips": trips}
    if args.controls:
        from tests.test_numpy_penetration import APPLIES
        controls = {c: {n: pen.control_error(n, c) for n in APPLIES[c]} for c in pen.CONTROLS}
        res["accuracy"].update(negative_control_errors_m=controls, tol_limit_m=0.1 * min(min(v.values()) for v in controls.values()))
    print(json.dumps(res["accuracy"]), flush=True)
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
