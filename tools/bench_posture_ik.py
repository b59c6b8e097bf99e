#!/usr/bin/env python3
"""Cost of rr_posture_ik on the MI355X: 4096 envs x 32 targets.  Goals are drawn uniformly within the joint limits; the targets are
their forward kinematics (posture_kinematics: the gripper base's position and its link's quaternion), the seeds the goals plus
U(-0.3, 0.3) rad on the arm joints, clipped to the limits -- the workload of tests/numpy_pik.py `fixture` at the batch's size.

  (a) posture_ik on device tensors at max_iterations 16, 32 and 64, full pose and position only: one launch per call, timed on the
      library's stream between two HIP events, the windows of the six variants ALTERNATING, WARMUP calls of each first; the median
      window gives the microseconds per call, min and max the spread.  Per variant also the share of rows per status and the mean and
      maximum `iterations`.  A wave of 64 rows runs as long as its slowest row: the rows at the cap set the time.
  (c) the two ends of (a) at a cap of 64: every row at the cap (every target moved 5 m away: the time of 64 updates on a full
      device) and ONE row of the batch at the cap (that target alone moved, every other seed its goal: the time of one wave's 64
      updates with the device to itself).
  (b) what one did before: 32 calls of ik() -- one target per env, seeded from the env's present joints -- on a handle created with
      solver={'ik_single_seed': True}, host arrays in and out, wall clock with the host round trip; the same targets, the envs at rest
      in their reset posture (ik() has no seed argument: a seed per target would cost a write_state each and disturb the simulation).
      Its residuals give the share of targets it solves (< 1e-3) from that one seed.

    python tools/bench_posture_ik.py [--out FILE.json] [--label TEXT] [--reps 11]"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped')
ap.add_argument('--reps', type=int, default=11)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.model import load_model  # noqa: E402

N, K, WARMUP, CALLS = 4096, nat.PC_MAX_POSTURES, 3, 20
CAPS = (16, 32, 64)

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
rng = np.random.default_rng(11)
lim = np.array(load_model()['body_limits'], np.float64)
goal = rng.uniform(lim.min(1), lim.max(1), (N, K, 11)).astype(np.float32)
seeds = goal.copy()
seeds[..., :7] = np.clip(goal[..., :7] + rng.uniform(-0.3, 0.3, (N, K, 7)).astype(np.float32), lim[:7, 0].astype(np.float32), lim[:7, 1].astype(np.float32))
pk = env.posture_kinematics(goal, host=True)
targets = np.ascontiguousarray(np.concatenate([pk['point_pos'][:, :, 0], pk['link_pose'][:, :, nat.EE_LINK, 3:]], -1))
with torch.cuda.stream(stream):
    dev_t, dev_s = torch.from_numpy(targets).cuda(), torch.from_numpy(seeds).cuda()
stream.synchronize()

VARIANTS = [(mode, cap) for mode in ('full_pose', 'position_only') for cap in CAPS]


def call(mode, cap, host=False):
    return env.posture_ik(dev_t, dev_s, max_iterations=cap, position_only=(mode == 'position_only'), host=host)


def window(mode, cap):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(CALLS):
        call(mode, cap)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


res = {"label": args.label, "envs": N, "targets": K, "rows": N * K, "windows": args.reps, "calls_per_window": CALLS,
       "workload": "goals uniform within the limits, targets their forward kinematics, seeds the goals + U(-0.3, 0.3) rad clipped; defaults "
                   "otherwise (tolerance 1e-3, damping 0.1, max_step 0.5, clamped)", "posture_ik": {}}
for v in VARIANTS:
    for _ in range(WARMUP):
        call(*v)
env.sync()
us = {v: [] for v in VARIANTS}
for _ in range(args.reps):
    for v in VARIANTS:
        us[v].append(window(*v))
for mode, cap in VARIANTS:
    out = call(mode, cap, host=True)
    st, it = out['status'], out['iterations']
    t = us[(mode, cap)]
    row = {"us_per_call_median": round(float(np.median(t)), 2), "us_per_call_min": round(float(min(t)), 2), "us_per_call_max": round(float(max(t)), 2),
           "ns_per_row": round(float(np.median(t)) * 1e3 / (N * K), 3),
           "share_status_0_converged": round(float((st == 0).mean()), 5), "share_status_1_cap": round(float((st == 1).mean()), 5),
           "share_status_2_not_finite": round(float((st == 2).mean()), 5), "iterations_mean": round(float(it.mean()), 3), "iterations_max": int(it.max()),
           "share_of_waves_with_a_row_at_the_cap": round(float((it.reshape(-1, 64) == cap).any(1).mean()), 4)}
    res["posture_ik"].setdefault(mode, {})[str(cap)] = row
    print(mode, cap, json.dumps(row), flush=True)
# (c) every row at the cap / one row at the cap
far = targets.copy()
far[..., 0] += 5.0
one = targets.copy()
one[0, 0, 0] += 5.0
with torch.cuda.stream(stream):
    ends = {"every_row_at_the_cap": (torch.from_numpy(far).cuda(), dev_s), "one_row_at_the_cap": (torch.from_numpy(one).cuda(), torch.from_numpy(goal).cuda())}
stream.synchronize()
res["ends_at_64"] = {}
for mode in ('full_pose', 'position_only'):
    for name, (t_, s_) in ends.items():
        def run(host=False):
            return env.posture_ik(t_, s_, max_iterations=64, position_only=(mode == 'position_only'), host=host)
        for _ in range(WARMUP):
            run()
        env.sync()
        t = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(CALLS):
                run()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / CALLS)
        st = run(host=True)['status']
        row = {"us_per_call_median": round(float(np.median(t)), 2), "us_per_call_min": round(float(min(t)), 2), "us_per_call_max": round(float(max(t)), 2),
               "rows_at_the_cap": int((st == 1).sum())}
        res["ends_at_64"].setdefault(mode, {})[name] = row
        print(mode, name, json.dumps(row), flush=True)
env.close()

# (b) the former road: one target per env and call, from the present joints, through the host
old = BatchedREALRobotEnv(N, objects=3, width=64, height=64, solver={'ik_single_seed': True})
old.reset()
old.ik(np.ascontiguousarray(targets[:, 0]))           # warm-up: the first call allocates
walls, solved = [], 0.0
for _ in range(3):
    t0 = time.perf_counter()
    r = [old.ik(np.ascontiguousarray(targets[:, k]))[1] for k in range(K)]
    walls.append((time.perf_counter() - t0) * 1e6)
    solved = float((np.stack(r, 1) < 1e-3).mean())
old.close()
res["ik_x32_single_seed_host_round_trip"] = {"us_per_32_calls_median": round(float(np.median(walls)), 1), "us_per_32_calls_min": round(float(min(walls)), 1),
                                              "us_per_32_calls_max": round(float(max(walls)), 1), "repeats": 3,
                                              "share_of_targets_with_residual_below_1e-3": round(solved, 5),
                                              "note": "seeded from the reset posture, up to 1000 iterations per target"}
print(json.dumps({"label": args.label, "posture_ik_us": {m: {c: r["us_per_call_median"] for c, r in d.items()} for m, d in res["posture_ik"].items()},
                  "ik_x32_us": res["ik_x32_single_seed_host_round_trip"]["us_per_32_calls_median"]}))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
