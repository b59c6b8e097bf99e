#!/usr/bin/env python3
"""Cost of rr_kinematic_observations on the MI355X: the step loop of 4096 envs, 3 objects, `synthetic_actions`, steps 170-370, without
the camera and with the 128x128 render -- plain; with link_poses() after every step (k_link_poses plus a synchronising copy to the
host: the road to a link pose before this call existed); and (when the build has the call) with kinematic_observations() after every
step, for one point (`obs`) and for eight (`obs8`).
Every window starts from the same checkpoint (step 170) and ends in a synchronise; REPS windows per variant, alternating.

    python tools/bench_kinematic_obs.py [--root TREE] [--out FILE.json] [--variants plain,link_poses]

--root: the tree whose `real_robots_amd` package (with its built library) is measured -- a checkout of the parent commit for the
plain loop of the parent; default: this tree.  Run parent and this tree alternately, three processes each, for the spread.
--variants: a subset of plain,link_poses,obs,obs8 (default: all the build has) -- `plain,link_poses` gives this tree the windows of
the parent, in the parent's order."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--variants', default='plain,link_poses,obs,obs8')
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import real_robots_amd  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

assert os.path.abspath(real_robots_amd.__file__).startswith(root), real_robots_amd.__file__
N, T0, T1 = 4096, 170, 370
POINTS8 = ([0, 4, 8, 8, 10, 16, 14, 11], np.linspace(-0.2, 0.2, 24).reshape(8, 3))
epochs, cmds = {}, []
for t in range(T1):
    k = t // 20
    if k not in epochs:
        epochs[k] = torch.from_numpy(synthetic_actions(list(range(N)), k * 20, hold_prob=0.05).astype(np.float32)).to('cuda:0')
    cmds.append(epochs[k])
res = {"root": root, "envs": N, "window": [T0, T1], "runs": []}
for render in (False, True):
    env = BatchedREALRobotEnv(N, objects=3, width=128, height=128)
    has = hasattr(env, 'kinematic_observations')
    if has:
        env.kinematic_observations()          # the buffers are allocated outside the timed windows
    for t in range(T0):
        env.step(device_ptr=cmds[t].data_ptr(), render=render)
    env.sync()
    ck = env.checkpoint()
    for rep in range(args.reps):
        for variant in [v for v in args.variants.split(',') if has or v in ('plain', 'link_poses')]:
            if has:
                env.set_kinematic_points(*(POINTS8 if variant == 'obs8' else (['base'], None)))
            env.restore(ck)
            env.sync()
            t0 = time.perf_counter()
            for t in range(T0, T1):
                env.step(device_ptr=cmds[t].data_ptr(), render=render)
                if variant == 'link_poses':
                    env.link_poses()
                elif variant != 'plain':
                    env.kinematic_observations()
            env.sync()
            ms = (time.perf_counter() - t0) * 1e3 / (T1 - T0)
            res["runs"].append({"render": render, "variant": variant, "rep": rep, "ms_per_step": round(ms, 5)})
            print(render, variant, rep, round(ms, 5), flush=True)
    env.close()
for render in (False, True):
    for variant in ('plain', 'link_poses', 'obs', 'obs8'):
        v = sorted(r["ms_per_step"] for r in res["runs"] if r["render"] == render and r["variant"] == variant)
        if v:
            res["median_ms_%s_%s" % ('render' if render else 'norender', variant)] = v[len(v) // 2]
print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
