#!/usr/bin/env python3
"""Cost of rr_swept_clearance on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; K = 8 segments per
env from each env's own posture to one drawn around it with |dq|inf = 0.1 and 0.5 rad (uniform per joint, one joint at the full span);
the pair tables `collision` (the step's whole collision table, Q = 92) and `robot` (its 80 pairs with a robot shape on either side: what
a planner of the arm asks -- in `collision` the objects that rest on the table touch it, an object x table pair that no joint moves is
within any safety at t = 0, and every segment stops there after one step); safety 0.01 m, tolerance 1e-3 m.

Per span: WARMUP calls, then REPS rounds in which a window of back-to-back swept_clearance calls and a window of what a user does today
-- eight posture_clearance calls at K = 32, the 32 uniform samples of each of the eight segments -- alternate on the library's stream,
each between two HIP events; the medians give the milliseconds per call and their ratio.  Also the statuses, the steps and the pair
evaluations per segment (the sampling check spends 32 x Q = 2944 pair searches per segment whatever the segment), and how many segments
the sampling check calls free that the sweep stops (tunnels and grazes between samples, and stops within `tolerance`).

    python tools/bench_swept_clearance.py [--out FILE.json] [--reps 11]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped: one wave per (env, segment), the due pairs of a step one after the other, one LDS reduction per step')
ap.add_argument('--reps', type=int, default=11)
ap.add_argument('--envs', type=int, default=4096)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, T0, WARMUP, K, SAMPLES, SAFETY, TOLERANCE = args.envs, 170, 3, 8, 32, 0.01, 1e-3

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
state = env.state
rng = np.random.default_rng(11)
env.set_distance_pairs('collision')
collision = env.distance_pairs()[0]
robot_shape = np.array([0 <= r['body'] < 16 for r in env.collision_shapes()])
TABLES = (('collision', collision), ('robot', collision[robot_shape[collision[:, 0]] | robot_shape[collision[:, 1]]]))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(calls):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def stats(ms):
    return {"ms_per_call_median": round(float(np.median(ms)), 3), "ms_per_call_min": round(float(min(ms)), 3), "ms_per_call_max": round(float(max(ms)), 3)}


res = {"label": args.label, "envs": N, "K": K, "state": "step %d of synthetic_actions" % T0, "rounds": args.reps, "safety_m": SAFETY,
       "tolerance_m": TOLERANCE, "samples_per_segment_of_the_sampling_check": SAMPLES, "tables": {}}
for table, span in [(t, s) for t in TABLES for s in (0.1, 0.5)]:
    env.set_distance_pairs(table[1])
    Q = len(table[1])
    dq = rng.uniform(-span, span, size=(N, K, 11))
    dq[np.arange(N)[:, None], np.arange(K)[None, :], rng.integers(0, 11, size=(N, K))] = span
    seg = np.zeros((N, K, 2, 11), np.float32)
    seg[:, :, 0] = state[:, None, :11]
    seg[:, :, 1] = seg[:, :, 0] + dq.astype(np.float32)
    ts = (np.arange(SAMPLES) / (SAMPLES - 1.0)).astype(np.float32)
    samples = [np.ascontiguousarray(seg[:, k, None, 0] + ts[None, :, None] * (seg[:, k, None, 1] - seg[:, k, None, 0])) for k in range(K)]      # K x [N, 32, 11]
    with torch.cuda.stream(stream):
        dev_seg = torch.from_numpy(seg).cuda()
        dev_samples = [torch.from_numpy(s).cuda() for s in samples]
    stream.synchronize()

    def sweep():
        env.swept_clearance(dev_seg, SAFETY, TOLERANCE)

    def sampling():
        for k in range(K):
            env.posture_clearance(dev_samples[k])
    for _ in range(WARMUP):
        sweep()
        sampling()
    env.sync()
    new, old = [], []
    for _ in range(args.reps):
        new.append(window(sweep, 4))
        old.append(window(sampling, 1))
    out = {k: np.array(v) for k, v in env.swept_clearance(dev_seg, SAFETY, TOLERANCE, host=True).items()}
    sampled_min = np.stack([np.array(env.posture_clearance(dev_samples[k], host=True)['pair_distance']).min(axis=(1, 2)) for k in range(K)], 1)      # [N, K]
    sampled_free = sampled_min > SAFETY
    st = out['status']
    row = {"swept_clearance": stats(new), "eight_posture_clearance_calls_at_K_32": stats(old),
           "sampling_over_sweep": round(float(np.median(old) / np.median(new)), 2),
           "status_counts": {str(s): int((st == s).sum()) for s in (0, 1, 3)},
           "steps_per_segment": {"mean": round(float(out['steps'].mean()), 2), "median": float(np.median(out['steps'])), "max": int(out['steps'].max())},
           "pair_evaluations_per_segment": {"mean": round(float(out['evaluations'].mean()), 1), "median": float(np.median(out['evaluations'])), "max": int(out['evaluations'].max())},
           "mean_fraction_proved_free_at_the_step_cap": round(float(out['fraction'][st == 3].mean()), 3) if (st == 3).any() else None,
           "pair_evaluations_of_the_sampling_check_per_segment": SAMPLES * Q,
           "evaluations_sampling_over_sweep": round(SAMPLES * Q / float(out['evaluations'].mean()), 1),
           "segments_free_by_sampling": int(sampled_free.sum()), "segments_free_by_sweep": int((st == 0).sum()),
           "free_by_sampling_but_stopped_by_sweep": int((sampled_free & (st != 0)).sum()),
           "free_by_sweep_but_not_by_sampling": int((~sampled_free & (st == 0)).sum())}
    res["tables"].setdefault(table[0], {"Q": Q, "spans": {}})["spans"]["%.1f" % span] = row
    print(table[0], 'span', span, json.dumps(row), flush=True)
env.close()
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
