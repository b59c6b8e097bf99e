#!/usr/bin/env python3
"""Cost and accuracy of rr_posture_clearance on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; K in
{1, 8, 32} candidate postures per env drawn around each env's own (sigma 0.1 rad); the pair tables `fingers8` (the four finger pads x
cube and tomato, Q = 8) and `collision` (the step's whole collision table, Q = 92).  Per (table, K): WARMUP calls, then REPS windows
of back-to-back calls on the library's stream between two HIP events; the median window gives the microseconds per call.

In the same process, what a user did before on the same tree: K x (write_state(joint_pos) + closest_points()) on device tensors and
one final write-back of the present joints, timed the same way; and rr_closest_points alone, for the cost of a pair.

Also the iteration statistics from pair_iterations, the accuracy on case R of tests/test_gpu_posture_query.py (the largest
|distance - exact| over its decided items against tests/numpy_posture.py: the MEASURED of that test, and TOL = 4 x), and the number of
items of case R whose distance bits differ from rr_closest_points on a written twin handle.

    python tools/bench_posture_clearance.py [--out FILE.json] [--label TEXT] [--no-accuracy] [--controls]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped: a workgroup per (env, posture), a wave per pair, the nearest pair reduced through LDS')
ap.add_argument('--no-accuracy', action='store_true')
ap.add_argument('--controls', action='store_true', help='also compute the negative controls of case R (CPU, about a minute)')
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


res = {"label": args.label, "envs": N, "state": "step %d of synthetic_actions" % T0, "windows": args.reps, "posture_sigma_rad": 0.1, "tables": {}}
with torch.cuda.stream(stream):
    mask = torch.ones(N, dtype=torch.uint8, device='cuda')
    present = torch.from_numpy(state).cuda()
for name, pairs in TABLES.items():
    env.set_distance_pairs(pairs)
    Q = len(env.distance_pairs()[0])
    cp = windows(env.closest_points, 20)
    cp["ns_per_pair"] = round(cp["us_per_call_median"] * 1e3 / (N * Q), 3)
    res["tables"][name] = {"Q": Q, "closest_points": cp, "K": {}}
    print(name, 'closest_points', json.dumps(cp), flush=True)
    for K in KS:
        po = (state[:, None, :11] + rng.normal(0.0, 0.1, size=(N, K, 11))).astype(np.float32)
        rows = np.repeat(state[None], K, axis=0)
        rows[:, :, :11] = po.transpose(1, 0, 2)
        with torch.cuda.stream(stream):
            dev_po = torch.from_numpy(po).cuda()
            dev_rows = [torch.from_numpy(np.ascontiguousarray(rows[k])).cuda() for k in range(K)]
        stream.synchronize()
        calls = max(2, 20 // K)
        new = windows(lambda: env.posture_clearance(dev_po), calls)

        def loop():
            for k in range(K):
                env.write_state(dev_rows[k], mask, joint_pos=True)
                env.closest_points()
            env.write_state(present, mask, joint_pos=True)
        old = windows(loop, calls)
        assert env.state.tobytes() == state.tobytes()                     # the loop put the joints back
        out = env.posture_clearance(dev_po, host=True)
        it, st = np.array(out['pair_iterations']), np.array(out['pair_status'])
        row = {"calls_per_window": calls, "posture_clearance": dict(new, ns_per_posture_pair=round(new["us_per_call_median"] * 1e3 / (N * K * Q), 3)),
               "write_and_query_loop": dict(old, ns_per_posture_pair=round(old["us_per_call_median"] * 1e3 / (N * K * Q), 3)),
               "loop_over_query": round(old["us_per_call_median"] / new["us_per_call_median"], 2),
               "per_pair_against_closest_points": round(new["us_per_call_median"] * 1e3 / (N * K * Q) / cp["ns_per_pair"], 3),
               "status_counts": {str(s): int((st == s).sum()) for s in range(4)},
               "median_iterations": float(np.median(it)), "mean_iterations": round(float(it.mean()), 2), "max_iterations": int(it.max())}
        res["tables"][name]["K"][str(K)] = row
        print(name, 'K', K, json.dumps(row), flush=True)
env.close()
if not args.no_accuracy:
    from tests import numpy_distance as nd
    from tests import numpy_posture as npo
    st, po, pairs = npo.case_r_inputs()
    ref = npo.case_r()
    e = BatchedREALRobotEnv(4, objects=3, width=64, height=64)
    e.state = st
    e.set_distance_pairs(pairs)
    out = {k: np.array(v) for k, v in e.posture_clearance(po, host=True).items()}
    m = (ref['decided'] & (ref['d'] > 0)).reshape(4, 4, 80)
    err = float(np.abs(out['pair_distance'].astype(np.float64) - ref['d'].reshape(4, 4, 80))[m].max())
    rows = npo.rows(st, po).reshape(4, 4, 61)
    twin = []
    for k in range(4):
        e.write_state(np.ascontiguousarray(rows[:, k]), np.ones(4, np.uint8), joint_pos=True)
        twin.append(np.array(e.closest_points(host=True)['distance']))
    e.close()
    twin = np.stack(twin, 1)
    differ = int((out['pair_distance'].view(np.uint32) != twin.view(np.uint32)).sum())
    res["accuracy"] = {"case": "R: N=4 K=4 Q=80", "decided_separated_items": int(m.sum()), "measured_max_abs_distance_error_m": err, "tol_m": 4 * err,
                       "items_whose_bits_differ_from_closest_points": differ, "items": int(twin.size),
                       "max_abs_difference_from_closest_points_m": float(np.abs(out['pair_distance'].astype(np.float64) - twin).max())}
    if args.controls:
        controls = {c: nd.control_error(ref, npo.case_r(control=c)) for c in npo.CONTROLS}
        controls.update({v: nd.control_error(ref, npo.case_r(variant=v)) for v in nd.VARIANTS})
        res["accuracy"].update(negative_control_errors_m=controls, tol_limit_m=0.1 * min(controls.values()))
    print(json.dumps(res["accuracy"]), flush=True)
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
