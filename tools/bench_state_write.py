#!/usr/bin/env python3
"""Cost of device-side state writes on the MI355X: the step loop of 4096 envs, 3 objects, `synthetic_actions`, steps 170-370, without
the camera and with the 128x128 render --
  plain        the step loop alone;
  host_reset   after every step the envs of a DEVICE-resident done mask (about 1 % of the envs, seeded, another mask every step) are
               reset and their objects put on start poses by the host road, the only one before rr_write_state: mask.cpu(), rr_reset,
               rr_set_object_poses (a blocking round trip and a synchronising upload);
  dev_reset    the same through write_state(poses, mask, reset=True, obj_pose=True): one launch, nothing waits (when the build has it);
  host_empty / dev_empty   the same two calls with a mask that selects NO env (host: rr_reset of a host mask, no round trip): nothing is
               written, but the look-ahead is dropped and the next step prepares itself in line -- the cost every outside change of
               state has had since the look-ahead exists, apart from the write itself.
Every window starts from the same checkpoint (step 170) and ends in a synchronise; REPS windows per variant, alternating.
Behind the windows: `launches` back-to-back calls of write_state (device road, every env masked, all four column groups) and of
read_state between two events on the library's stream, as microseconds per call (the write's figure includes the observation refresh
that follows it; a kernel trace separates the two).

    python tools/bench_state_write.py [--root TREE] [--out FILE.json] [--variants plain,host_reset,host_empty]

--root: the tree whose `real_robots_amd` package (with its built library) is measured -- a checkout of the parent commit for the
parent's loops; default: this tree.  Run parent and this tree alternately, three processes each, for the spread."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--launches', type=int, default=200)
ap.add_argument('--variants', default='plain,host_reset,dev_reset,host_empty,dev_empty')
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import real_robots_amd  # noqa: E402
from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

assert os.path.abspath(real_robots_amd.__file__).startswith(root), real_robots_amd.__file__
N, T0, T1 = 4096, 170, 370
VARIANTS = ('plain', 'host_reset', 'dev_reset', 'host_empty', 'dev_empty')
epochs, cmds = {}, []
for t in range(T1):
    k = t // 20
    if k not in epochs:
        epochs[k] = torch.from_numpy(synthetic_actions(list(range(N)), k * 20, hold_prob=0.05).astype(np.float32)).to('cuda:0')
    cmds.append(epochs[k])
rng = np.random.default_rng(7)
done = [torch.from_numpy((rng.random(N) < 0.01).astype(np.uint8)).to('cuda:0') for _ in range(T1 - T0)]      # the "done" bits of a policy
none_dev, none_host = torch.zeros(N, dtype=torch.uint8, device='cuda:0'), np.zeros(N, np.uint8)
res = {"root": root, "envs": N, "window": [T0, T1], "done_share": round(float(np.mean([d.float().mean().item() for d in done])), 5), "runs": []}
for render in (False, True):
    env = BatchedREALRobotEnv(N, objects=3, width=128, height=128)
    has = hasattr(env, 'write_state')
    # start poses: every env's objects where its reset puts them, moved by a seeded few centimetres
    env.reset()
    poses = env.host(nat.F_OBJ_POSE).copy()
    poses[:, :, :2] += rng.uniform(-0.05, 0.05, (N, 3, 2)).astype(np.float32)
    rows = np.zeros((N, 61), np.float32)
    for o in range(3):
        rows[:, 22 + 13 * o:29 + 13 * o] = poses[:, o]
    rows_dev = torch.from_numpy(rows).to('cuda:0')
    for t in range(T0):
        env.step(device_ptr=cmds[t].data_ptr(), render=render)
    env.sync()
    ck = env.checkpoint()
    for rep in range(args.reps):
        for variant in [v for v in args.variants.split(',') if has or not v.startswith('dev_')]:
            env.restore(ck)
            env.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(T0, T1):
                env.step(device_ptr=cmds[t].data_ptr(), render=render)
                if variant == 'host_reset':
                    m = done[t - T0].cpu().numpy()
                    env.reset(m)
                    env.set_object_poses(poses, m)
                elif variant == 'dev_reset':
                    env.write_state(rows_dev, done[t - T0], reset=True, obj_pose=True)
                elif variant == 'host_empty':
                    env.reset(none_host)
                elif variant == 'dev_empty':
                    env.write_state(None, none_dev, reset=True)
            env.sync()
            ms = (time.perf_counter() - t0) * 1e3 / (T1 - T0)
            res["runs"].append({"render": render, "variant": variant, "rep": rep, "ms_per_step": round(ms, 5)})
            print(render, variant, rep, round(ms, 5), flush=True)
    if has and not render and args.launches > 0:
        env.restore(ck)
        state = torch.from_dlpack(env.read_state()).clone()
        for name, call in (('write_state', lambda: env.write_state(state, None, joint_pos=True, joint_vel=True, obj_pose=True, obj_vel=True)),
                           ('read_state', env.read_state)):
            us = []
            for rep in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                env.sync()
                e0.record()
                for _ in range(args.launches):
                    call()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / args.launches)
            res["us_per_call_back_to_back_" + name] = round(sorted(us)[len(us) // 2], 3)
    env.close()
for render in (False, True):
    for variant in VARIANTS:
        v = sorted(r["ms_per_step"] for r in res["runs"] if r["render"] == render and r["variant"] == variant)
        if v:
            res["median_ms_%s_%s" % ('render' if render else 'norender', variant)] = v[len(v) // 2]
print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
