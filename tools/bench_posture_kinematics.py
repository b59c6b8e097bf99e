#!/usr/bin/env python3
"""Cost of rr_posture_kinematics on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; K = 32 candidate
postures per env drawn uniformly within the joint limits; P = 1 (the default point) and P = 8 kinematic points.  Three variants, timed
in the same process on the library's stream between two HIP events, their windows ALTERNATING; WARMUP calls of each first; the median
window gives the microseconds per call, min and max the spread:

  (a) posture_kinematics on a device tensor [N, 32, 11]: one launch;
  (b) 32 launches of kinematic_observations() alone -- the present-state kernel, which this query leaves untouched: a LOWER bound of
      what one did before (it evaluates the same posture 32 times and writes no candidate);
  (c) the full former loop: 32 x (write_state(joint_pos) + kinematic_observations()) on device tensors and the write-back of the
      present joints.

Also (a)'s achieved store bandwidth -- the bytes of the three buffers over its time -- against the copy bandwidth rr_device_microbench
(kind 0: bytes read + written per second) reports in the same run, and a check that row (e, k) of (a) has the bits of (c)'s
observations at posture k.

    python tools/bench_posture_kinematics.py [--out FILE.json] [--label TEXT] [--reps 11]"""
import argparse
import json
import os
import sys

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
from real_robots_amd.distributed import synthetic_actions  # noqa: E402
from real_robots_amd.model import load_model  # noqa: E402

N, T0, WARMUP, K = 4096, 170, 3, nat.PC_MAX_POSTURES
CALLS = {'a': 100, 'b': 10, 'c': 5}        # calls per window: 100 launches, 10 x 32 launches, 5 x 65 launches
POINTS8 = ([0, 4, 8, 8, 10, 16, 14, 11], np.linspace(-0.2, 0.2, 24).reshape(8, 3))

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
state = env.state
rng = np.random.default_rng(11)
lim = np.array(load_model()['body_limits'], np.float64)
po = rng.uniform(lim.min(1), lim.max(1), (N, K, 11)).astype(np.float32)
rows = np.repeat(state[None], K, axis=0)
rows[:, :, :11] = po.transpose(1, 0, 2)
with torch.cuda.stream(stream):
    mask = torch.ones(N, dtype=torch.uint8, device='cuda')
    present = torch.from_numpy(state).cuda()
    dev_po = torch.from_numpy(po).cuda()
    dev_rows = [torch.from_numpy(np.ascontiguousarray(rows[k])).cuda() for k in range(K)]
stream.synchronize()


def query():
    env.posture_kinematics(dev_po)


def launches():
    for _ in range(K):
        env.kinematic_observations()


def loop():
    for k in range(K):
        env.write_state(dev_rows[k], mask, joint_pos=True)
        env.kinematic_observations()
    env.write_state(present, mask, joint_pos=True)


VARIANTS = (('a', 'posture_kinematics', query), ('b', 'kinematic_observations_x32', launches), ('c', 'write_and_observe_loop', loop))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(calls):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


ubench = nat.device_microbench(0)
res = {"label": args.label, "envs": N, "postures": K, "state": "step %d of synthetic_actions" % T0, "windows": args.reps, "calls_per_window": CALLS,
       "device_microbench": ubench, "points": {}}
for P in (1, 8):
    env.set_kinematic_points(*(POINTS8 if P == 8 else (['base'], None)))
    for _, _, fn in VARIANTS:
        for _ in range(WARMUP):
            fn()
    env.sync()
    us = {key: [] for key, _, _ in VARIANTS}
    for _ in range(args.reps):
        for key, _, fn in VARIANTS:
            us[key].append(window(fn, CALLS[key]))
    assert env.state.tobytes() == state.tobytes()                     # the loop put the joints back
    row = {}
    for key, name, _ in VARIANTS:
        row[name] = {"us_per_call_median": round(float(np.median(us[key])), 2), "us_per_call_min": round(float(min(us[key])), 2),
                     "us_per_call_max": round(float(max(us[key])), 2)}
    a, b, c = (row[name]["us_per_call_median"] for _, name, _ in VARIANTS)
    out_bytes = N * K * (len(nat.LINK_NAMES) * 7 + 69 * P) * 4
    row.update(launches_over_query=round(b / a, 2), loop_over_query=round(c / a, 2), query_below_launches=bool(a < b), bytes_written=out_bytes,
               store_GBs=round(out_bytes / a / 1e3, 1), store_over_copy_bandwidth=round(out_bytes / a / 1e3 / ubench['hbm_copy_GBs'], 3),
               ns_per_row=round(a * 1e3 / (N * K), 3))
    # the rows of (a) are the observations of (c) at posture k, bit for bit (three postures looked at)
    out = env.posture_kinematics(dev_po, host=True)
    differ = 0
    for k in (0, K // 2, K - 1):
        env.write_state(dev_rows[k], mask, joint_pos=True)
        obs = env.kinematic_observations(host=True)
        differ += sum(int((out[name][:, k].view(np.uint32) != obs[name].view(np.uint32)).sum()) for name in nat.PK_FIELDS)
    env.write_state(present, mask, joint_pos=True)
    row["floats_whose_bits_differ_from_the_loop"] = differ
    res["points"][str(P)] = row
    print('P', P, json.dumps(row), flush=True)
env.close()
print(json.dumps({"label": args.label, "points": {p: {k: v for k, v in r.items() if not isinstance(v, dict)} for p, r in res["points"].items()}}))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
