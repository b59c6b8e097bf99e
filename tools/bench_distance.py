#!/usr/bin/env python3
"""Cost and accuracy of rr_closest_points on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; the
pair table `fingers8` (the four finger pads x cube and tomato, Q = 8) and `collision` (the step's whole collision table, Q = 92).
Per table: WARMUP calls, then REPS windows of CALLS back-to-back calls on the library's stream between two HIP events; the median
window gives the microseconds per call.  Also the status counts and the iteration histogram (median and maximum per vertex-count
class of the pair's larger shape), and the accuracy on the parity cases of tests/test_gpu_distance.py (the largest
|distance - exact| over their decided items against tests/numpy_distance.py: the MEASURED of that test, and TOL = 4 x).

    python tools/bench_distance.py [--out FILE.json] [--label TEXT] [--alternatives A.json B.json ...] [--no-accuracy]

--label names the build that is measured (RR_LIB selects another library: builds with -DDIST_ENVS=2, 4, 8);
--alternatives embeds the summaries of earlier outputs of this tool, the launch shapes that were measured and dropped."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped: 1 env per workgroup, a wave per (env, pair), vertices about the sphere centres, float64 norms')
ap.add_argument('--alternatives', nargs='*', default=[])
ap.add_argument('--no-accuracy', action='store_true')
ap.add_argument('--reps', type=int, default=11)
ap.add_argument('--calls', type=int, default=20)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, T0, WARMUP = 4096, 170, 5
names = {r['name']: r['index'] for r in BatchedREALRobotEnv.collision_shapes()}
nv = np.array([int(x) for x in __import__('real_robots_amd.model', fromlist=['load_model']).load_model()['shape_nv']])
TABLES = {'fingers8': [(pad, obj) for obj in ('cube', 'tomato') for pad in ('skin_00', 'skin_01', 'skin_10', 'skin_11')], 'collision': 'collision'}

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
res = {"label": args.label, "library": os.environ.get('RR_LIB', 'librealrobot_hip.so'), "envs": N, "state": "step %d of synthetic_actions" % T0,
       "calls_per_window": args.calls, "windows": args.reps, "tables": {}}
for name, pairs in TABLES.items():
    env.set_distance_pairs(pairs)
    table = env.distance_pairs()[0]
    for _ in range(WARMUP):
        env.closest_points()
    env.sync()
    us = []
    for rep in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.calls):
            env.closest_points()
        e1.record(stream)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    out = env.closest_points(host=True)
    it, status = np.array(out['iterations']), np.array(out['status'])
    big = np.maximum(nv[table[:, 0]], nv[table[:, 1]])
    hist = {}
    for cls in sorted(set(big.tolist())):
        x = it[:, big == cls]
        hist["larger shape has %d vertices" % cls] = {"pairs": int((big == cls).sum()), "median_iterations": float(np.median(x)), "max_iterations": int(x.max())}
    res["tables"][name] = {"Q": int(len(table)), "us_per_call_median": round(float(np.median(us)), 2), "us_per_call_min": round(float(min(us)), 2),
                           "us_per_call_max": round(float(max(us)), 2), "ns_per_pair": round(float(np.median(us)) * 1e3 / (N * len(table)), 3),
                           "status_counts": {str(s): int((status == s).sum()) for s in range(4)},
                           "median_iterations": float(np.median(it)), "max_iterations": int(it.max()), "iterations_by_class": hist}
    print(name, json.dumps(res["tables"][name]), flush=True)
env.close()
if not args.no_accuracy:
    from tests import numpy_distance as nd
    worst, per_case = 0.0, {}
    for n, _, pairs in nd.cases():
        st, pairs, ref = nd.case(n)
        e = BatchedREALRobotEnv(n, objects=3, width=64, height=64)
        e.state = st
        e.set_distance_pairs(pairs)
        out = e.closest_points(host=True)
        m = ref['decided'] & (ref['d'] > 0)
        err = float(np.abs(np.asarray(out['distance'], np.float64) - ref['d'])[m].max())
        vec = float(np.linalg.norm(np.asarray(out['point_a'], np.float64) - out['point_b'] - ref['v'], axis=-1)[m].max())
        per_case["N=%d Q=%d" % (n, len(pairs))] = {"decided_separated_items": int(m.sum()), "max_abs_distance_error_m": err, "max_closest_vector_error_m": vec}
        worst = max(worst, err)
        e.close()
    controls = {v: nd.control_error(nd.case(5)[2], nd.case(5, variant=v)[2]) for v in nd.VARIANTS}
    res["accuracy"] = {"cases": per_case, "measured_max_abs_distance_error_m": worst, "tol_m": 4 * worst,
                       "negative_control_errors_m": controls, "tol_limit_m": 0.1 * min(controls.values())}
    print(json.dumps(res["accuracy"]), flush=True)
if args.alternatives:
    res["alternatives_measured_and_dropped"] = []
    for path in args.alternatives:
        alt = json.load(open(path))
        res["alternatives_measured_and_dropped"].append({"label": alt["label"], "us_per_call_median": {k: v["us_per_call_median"] for k, v in alt["tables"].items()}})
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
