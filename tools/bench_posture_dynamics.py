#!/usr/bin/env python3
"""Cost of rr_posture_dynamics on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; K = 32 rows per env
-- postures uniform within the joint limits, velocities in +-3 rad/s, accelerations in +-10 rad/s^2 -- on device tensors.  Four
variants: with and without (velocities and accelerations), with and without the inverse.  Timed in the same process on the library's
stream between two HIP events, the variants' windows ALTERNATING; WARMUP calls of each first; the median window gives the
microseconds per call, min and max the spread.

Every time is reported against two yardsticks:

  (1) the bytes the call writes (80.7 MB without the inverse, 144 MB with it) over the HBM bandwidth rr_device_microbench reports in
      the same run (kind 0: bytes read + written per second of a copy) -- `time_over_store_bound`;
  (2) 32 x the preparation's joint-space dynamics on the same 4096 envs: the same arithmetic on the same number of rows.
      rr_get_timing has ONE timer for the preparation, `k_prep` = k_prep_a16 + k_prep_b16 back to back (frames and object terms,
      then the dynamics); k_prep_b16 alone is not behind a timer of its own.  The tool reports `k_prep` as measured
      (`time_over_32_k_prep`: a yardstick that is too generous by k_prep_a16's share), and takes k_prep_b16 alone, in microseconds
      per launch, from a kernel trace of this very tool when one is given with --prep-b16-us (`time_over_32_k_prep_b16`; the source
      is recorded with --prep-b16-source).

    python tools/bench_posture_dynamics.py [--out FILE.json] [--label TEXT] [--reps 11] [--prep-b16-us X --prep-b16-source TEXT]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped')
ap.add_argument('--reps', type=int, default=11)
ap.add_argument('--prep-b16-us', type=float, default=None)
ap.add_argument('--prep-b16-source', default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402
from real_robots_amd.model import load_model  # noqa: E402

N, T0, WARMUP, K, CALLS, TIMED_STEPS = 4096, 170, 3, nat.PC_MAX_POSTURES, 100, 20

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
# yardstick (2): the preparation's timer over TIMED_STEPS timed steps (every kernel of a timed step runs alone on the main stream)
env.set_timing(True)
env.get_timing()
for t in range(TIMED_STEPS):
    env.step(cmd)
env.sync()
prep_ms, prep_n = env.get_timing()['k_prep']
env.set_timing(False)
env.sync()
state = env.state
k_prep_us = prep_ms * 1e3 / max(prep_n, 1)

rng = np.random.default_rng(11)
lim = np.array(load_model()['body_limits'], np.float64)
with torch.cuda.stream(stream):
    q = torch.from_numpy(rng.uniform(lim.min(1), lim.max(1), (N, K, 11)).astype(np.float32)).cuda()
    qd = torch.from_numpy(rng.uniform(-3, 3, (N, K, 11)).astype(np.float32)).cuda()
    qdd = torch.from_numpy(rng.uniform(-10, 10, (N, K, 11)).astype(np.float32)).cuda()
stream.synchronize()

VARIANTS = (('postures', (q, None, None), False), ('postures_inverse', (q, None, None), True),
            ('postures_velocities_accelerations', (q, qd, qdd), False), ('postures_velocities_accelerations_inverse', (q, qd, qdd), True))


def window(tensors, inverse):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(CALLS):
        env.posture_dynamics(*tensors, inverse=inverse)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


ubench = nat.device_microbench(0)
res = {"label": args.label, "envs": N, "rows_per_env": K, "state": "step %d of synthetic_actions" % T0, "windows": args.reps, "calls_per_window": CALLS,
       "warmup_calls": WARMUP, "device_microbench": ubench,
       "k_prep_us_per_launch": round(k_prep_us, 2), "k_prep_launches_timed": int(prep_n),
       "k_prep_is": "rr_get_timing's timer 0: k_prep_a16 + k_prep_b16 back to back on 4096 envs, alone on the main stream",
       "k_prep_b16_us_per_launch": args.prep_b16_us, "k_prep_b16_source": args.prep_b16_source, "variants": {}}
for _, tensors, inverse in VARIANTS:
    for _ in range(WARMUP):
        env.posture_dynamics(*tensors, inverse=inverse)
env.sync()
us = {name: [] for name, _, _ in VARIANTS}
for _ in range(args.reps):
    for name, tensors, inverse in VARIANTS:
        us[name].append(window(tensors, inverse))
assert env.state.tobytes() == state.tobytes()                     # nothing of the simulation was written
for name, _, inverse in VARIANTS:
    med = float(np.median(us[name]))
    out_bytes = N * K * ((2 if inverse else 1) * nat.N_JOINTS ** 2 + 3 * nat.N_JOINTS) * 4
    bound_us = out_bytes / (ubench['hbm_copy_GBs'] * 1e3)
    row = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(us[name])), 2), "us_per_call_max": round(float(max(us[name])), 2),
           "bytes_written": out_bytes, "store_bound_us": round(bound_us, 2), "time_over_store_bound": round(med / bound_us, 2),
           "store_GBs": round(out_bytes / med / 1e3, 1), "time_over_32_k_prep": round(med / (K * k_prep_us), 3),
           "time_over_32_k_prep_b16": None if args.prep_b16_us is None else round(med / (K * args.prep_b16_us), 3),
           "ns_per_row": round(med * 1e3 / (N * K), 3)}
    res["variants"][name] = row
    print(name, json.dumps(row), flush=True)
env.close()
print(json.dumps({"label": args.label, "k_prep_us_per_launch": res["k_prep_us_per_launch"],
                  "us_per_call": {name: r["us_per_call_median"] for name, r in res["variants"].items()}}))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
