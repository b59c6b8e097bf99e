#!/usr/bin/env python3
"""Cost of env forks and snapshot slots on the MI355X, at 4096 envs, 3 objects, 128x128, from the step-170 checkpoint of bench.py's
workload (`synthetic_actions`, rendered):

 (a) one copy of the running envs for three maps -- the MPC map (64 groups of 64 envs, each group's first env into its other 63: in
     place, so staged), the identity save_snapshot / load_snapshot, a random permutation (the worst gather; in place, staged) -- as one
     call followed by a synchronise, and as the per-call time of BURST calls in a row before one synchronise (the launch and wait
     latency of a single call is of the size of the copy itself);
 (b) the burst figures against the HBM roofline: the bytes actually moved, from the live contact counts (twice over for a staged
     copy), over the copy bandwidth rr_device_microbench(kind 0) reports in the same run;
 (c) identity save + load against checkpoint() + restore() of the same batch (the host route: PCIe both ways and two waits);
 (d) the step loop of bench.py's shape (steps 170-370, rendered), plain and with an MPC-map fork before every step: the difference
     is the fork plus the lost look-ahead overlap (the step after a fork prepares itself in line);
 (e) the plain loop alone (--plain-only uses no call of this feature, so the same file measures the parent commit's library:
     --root PARENT_TREE).

    python tools/bench_fork.py [--out FILE.json] [--reps 7] [--plain-only] [--root TREE]

Medians of wall-clock times around synchronising calls over alternating windows; the first repetition of every variant is a warm-up
and is dropped."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--envs', type=int, default=4096)
ap.add_argument('--burst', type=int, default=50)
ap.add_argument('--plain-only', action='store_true')
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, S, T0, T1 = args.envs, 128, 170, 370
env = BatchedREALRobotEnv(N, objects=3, width=S, height=S)
res = {"envs": N, "image": [S, S], "reps": args.reps, "burst": args.burst, "plain_only": bool(args.plain_only)}


def median(v):
    v = sorted(v[1:] if len(v) > 1 else v)
    return round(v[len(v) // 2], 5)


def spread(v):
    v = v[1:] if len(v) > 1 else v
    return round(max(v) - min(v), 5)


epochs, cmds = {}, []
for t in range(T1):
    k = t // 20
    if k not in epochs:
        epochs[k] = torch.from_numpy(synthetic_actions(list(range(N)), k * 20, hold_prob=0.05).astype(np.float32)).to('cuda:0')
    cmds.append(epochs[k])
for t in range(T0):
    env.step(device_ptr=cmds[t].data_ptr(), render=True)
env.sync()
ck = env.checkpoint()


def step_loop(fork_index=None):
    env.restore(ck)
    env.sync()
    t0 = time.perf_counter()
    for t in range(T0, T1):
        if fork_index is not None:
            env.fork(fork_index)
        env.step(device_ptr=cmds[t].data_ptr(), render=True)
    env.sync()
    return (time.perf_counter() - t0) * 1e3 / (T1 - T0)


if args.plain_only:
    ms = [step_loop() for _ in range(args.reps)]
    res["e_step_ms_plain"], res["e_step_ms_plain_all"], res["e_step_ms_plain_spread"] = median(ms), [round(x, 5) for x in ms], spread(ms)
    env.close()
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, 'w'), indent=1)
    sys.exit(0)

mpc = (np.arange(N) // 64 * 64).astype(np.int32)
mpc[::64] = -1
perm = np.random.default_rng(2020).permutation(N).astype(np.int32)
maps = {'mpc': mpc, 'permutation': perm}
dev = {k: torch.from_numpy(v).to('cuda:0') for k, v in maps.items()}
torch.cuda.synchronize()
env.snapshot_slots(1)
env.sync()

# ---- (a) one copy, three maps
calls = {'mpc': lambda: env.fork(dev['mpc']), 'mpc_host_index': lambda: env.fork(mpc), 'save': lambda: env.save_snapshot(0),
         'load': lambda: env.load_snapshot(0), 'permutation': lambda: env.fork(dev['permutation'])}
count = np.clip(env.host(nat.F_CONTACT_COUNT), 0, nat.MAX_CONTACTS).astype(np.int64)
res["contacts_per_env_mean"] = round(float(count.mean()), 2)
rec = 72 * 4 + 5 * 4 + 16 + count * 48 + (count + 3) // 4 * 16       # bytes of every env's record that a copy reads (and writes)
single, burst = {k: [] for k in calls}, {k: [] for k in calls}
for rep in range(args.reps):
    for name, call in calls.items():
        env.restore(ck)                     # (every window copies the same records)
        if name == 'load':
            env.save_snapshot(0)
        env.sync()
        t0 = time.perf_counter()
        call()
        env.sync()
        single[name].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(args.burst):
            call()
        env.sync()
        burst[name].append((time.perf_counter() - t0) * 1e3 / args.burst)
for name in calls:
    res["a_%s_ms_single" % name], res["a_%s_ms_burst" % name] = median(single[name]), median(burst[name])
    res["a_%s_ms_burst_spread" % name] = spread(burst[name])

# ---- (b) against the copy bandwidth of the same run
bw = nat.device_microbench(0)['hbm_copy_GBs']           # GB/s of read + write traffic
res["b_hbm_copy_GBs"] = bw
moved = {'mpc': 2 * 2 * int(rec[mpc[mpc >= 0]].sum()),       # (a record's size is its SOURCE's)
         'save': 2 * int(rec.sum()), 'load': 2 * int(rec.sum()), 'permutation': 2 * 2 * int(rec.sum())}
for name, b in moved.items():
    roof_ms = b / (bw * 1e9) * 1e3
    res["b_%s_bytes" % name], res["b_%s_roofline_ms" % name] = b, round(roof_ms, 5)
    res["b_%s_time_over_roofline" % name] = round(res["a_%s_ms_burst" % name] / roof_ms, 2)

# ---- (c) save + load on the device against checkpoint() + restore() over the host
d, h = [], []
for rep in range(args.reps):
    env.restore(ck)
    env.sync()
    t0 = time.perf_counter()
    env.save_snapshot(0)
    env.load_snapshot(0)
    env.sync()
    d.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    blob = env.checkpoint()
    env.restore(blob)
    env.sync()
    h.append((time.perf_counter() - t0) * 1e3)
res["c_save_load_ms_device"], res["c_checkpoint_restore_ms_host"] = median(d), median(h)

# ---- (d), (e) the step loop, plain and with an MPC-map fork before every step
ms = {'plain': [], 'fork': []}
for rep in range(args.reps):
    for variant in ('plain', 'fork'):
        ms[variant].append(step_loop(dev['mpc'] if variant == 'fork' else None))
        print('d', variant, rep, round(ms[variant][-1], 5), flush=True)
res["d_step_ms_plain"], res["d_step_ms_fork_every_step"] = median(ms['plain']), median(ms['fork'])
res["d_step_ms_plain_all"], res["d_step_ms_fork_all"] = [round(x, 5) for x in ms['plain']], [round(x, 5) for x in ms['fork']]
res["d_step_ms_plain_spread"], res["d_step_ms_fork_spread"] = spread(ms['plain']), spread(ms['fork'])
env.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
