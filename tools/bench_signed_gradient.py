#!/usr/bin/env python3
"""Cost of rr_signed_gradient beside the unchanged rr_signed_distance on the MI355X: 4096 envs, 3 objects, the states of step 170 of
`synthetic_actions`, the `collision` pair table (Q = 92); at the present state and at K = 8 candidate postures per env drawn around
each env's own (sigma 0.1 rad), margin 0.05 m.  Per form the two queries ALTERNATE on the same handle in the same process -- gradient,
distance, gradient, distance --, each turn WARMUP calls and then REPS windows of back-to-back calls on the library's stream between two
HIP events; a turn's figure is its median window, a query's figure the mean of its two turns, and the ratio gradient / distance is
what profiles/signed_gradient_bench.json and NOTEBOOK.md carry.  The two turns of a query are printed side by side: their spread is
the noise the ratio has to be read against.

    python tools/bench_signed_gradient.py [--out FILE.json] [--reps N]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=11)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, T0, WARMUP, K, MARGIN = 4096, 170, 3, 8, 0.05

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
state = env.state
rng = np.random.default_rng(7)
env.set_distance_pairs('collision')
Q = len(env.distance_pairs()[0])
L, h = env.L, env.h


def turn(fn, calls):
    """median microseconds per call over the windows of one turn"""
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
    return round(float(np.median(us)), 2)


def ab(grad, dist, calls, items):
    g, d = [], []
    for _ in range(2):
        g.append(turn(grad, calls))
        d.append(turn(dist, calls))
    gm, dm = float(np.mean(g)), float(np.mean(d))
    return {"calls_per_window": calls, "windows": args.reps, "signed_gradient_us_per_call_turns": g, "signed_distance_us_per_call_turns": d,
            "signed_gradient_us_per_call": round(gm, 2), "signed_distance_us_per_call": round(dm, 2), "gradient_over_distance": round(gm / dm, 4),
            "signed_gradient_ns_per_item": round(gm * 1e3 / items, 3)}


res = {"envs": N, "state": "step %d of synthetic_actions" % T0, "table": "collision", "Q": Q, "margin_m": MARGIN, "posture_sigma_rad": 0.1}
# the C calls themselves: the binding's dict of views is not part of either query
res["present"] = ab(lambda: L.rr_signed_gradient(h, None, 0, 0, MARGIN), lambda: L.rr_signed_distance(h, None, 0, 0), 20, N * Q)
print('present', json.dumps(res["present"]), flush=True)
po = (state[:, None, :11] + rng.normal(0.0, 0.1, size=(N, K, 11))).astype(np.float32)
with torch.cuda.stream(stream):
    dev_po = torch.from_numpy(po).cuda()
stream.synchronize()
ptr = dev_po.data_ptr()
res["K8"] = ab(lambda: L.rr_signed_gradient(h, ptr, K, 1, MARGIN), lambda: L.rr_signed_distance(h, ptr, K, 1), 3, N * K * Q)
print('K 8', json.dumps(res["K8"]), flush=True)
out = env.signed_distance_gradient(dev_po, margin=MARGIN, host=True)
res["K8"].update(mean_cost=round(float(np.mean(out['cost'])), 6), rows_with_a_cost=int((np.array(out['cost']) > 0).sum()),
                 overlapping_share=round(float(np.isin(np.array(out['pair_status']), (1, 5)).mean()), 5))
assert np.isfinite(out['cost_gradient']).all() and env.state.tobytes() == state.tobytes()      # no query wrote the state
env.close()
print(json.dumps(res), flush=True)
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
