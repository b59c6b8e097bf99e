#!/usr/bin/env python3
"""Cost of rr_ray_cast on the MI355X: the step loop of 4096 envs, 3 objects, `synthetic_actions`, steps 170-370, without the camera
and with the 128x128 render -- plain; and (when the build has the call) with a cast after every step at R = 16 and R = 64 rays per
env, for the table's segments (`table16`, `table64`) and for a per-env device tensor read in place (`dev16`, `dev64`).
Every window starts from the same checkpoint (step 170) and ends in a synchronise; REPS windows per variant, alternating.

    python tools/bench_ray_cast.py [--root TREE] [--out FILE.json] [--variants plain]

--root: the tree whose `real_robots_amd` package (with its built library) is measured -- a checkout of the parent commit for the
plain loop of the parent; default: this tree.  Run parent and this tree alternately, three processes each, for the spread.
--variants: a subset of plain,table16,table64,dev16,dev64 (default: all the build has).

The rays are a sensor suite, the same for every env: half of them fan out from the gripper `base` (0.5 m), a quarter from the four
finger links (0.3 m), a quarter are world verticals from z = 0.9 m down through the table top on a grid over the work space."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--variants', default='plain,table16,table64,dev16,dev64')
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
VARIANTS = ('plain', 'table16', 'table64', 'dev16', 'dev64')


def sensor_suite(R):
    """(links, segments [R, 6]) of the benchmark's rays."""
    rng = np.random.default_rng(R)
    links, segs = [], np.zeros((R, 6), np.float32)
    for j in range(R):
        if j < R // 2:
            links.append('base')
            v = rng.normal(size=3)
            segs[j, 3:] = 0.5 * v / np.linalg.norm(v)
        elif j < 3 * R // 4:
            links.append(('finger_00', 'finger_01', 'finger_10', 'finger_11')[j % 4])
            v = rng.normal(size=3)
            segs[j, 3:] = 0.3 * v / np.linalg.norm(v)
        else:
            links.append('world')
            x, y = rng.uniform(-0.25, 0.25), rng.uniform(-0.45, 0.45)
            segs[j] = [x, y, 0.9, x, y, 0.2]
    return links, segs


epochs, cmds = {}, []
for t in range(T1):
    k = t // 20
    if k not in epochs:
        epochs[k] = torch.from_numpy(synthetic_actions(list(range(N)), k * 20, hold_prob=0.05).astype(np.float32)).to('cuda:0')
    cmds.append(epochs[k])
res = {"root": root, "envs": N, "window": [T0, T1], "runs": []}
for render in (False, True):
    env = BatchedREALRobotEnv(N, objects=3, width=128, height=128)
    has = hasattr(env, 'ray_cast')
    suites, tensors = {}, {}
    if has:
        for R in (16, 64):
            suites[R] = sensor_suite(R)
            tensors[R] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(suites[R][1], (N, R, 6)))).to('cuda:0')
        env.set_rays(*suites[64])
        env.ray_cast()                        # the buffers are allocated outside the timed windows
        torch.cuda.synchronize()
    for t in range(T0):
        env.step(device_ptr=cmds[t].data_ptr(), render=render)
    env.sync()
    ck = env.checkpoint()
    for rep in range(args.reps):
        for variant in [v for v in args.variants.split(',') if has or v == 'plain']:
            R = int(variant[-2:]) if variant != 'plain' else 0
            if R:
                env.set_rays(*suites[R])
            rays = tensors[R] if variant.startswith('dev') else None
            env.restore(ck)
            env.sync()
            t0 = time.perf_counter()
            for t in range(T0, T1):
                env.step(device_ptr=cmds[t].data_ptr(), render=render)
                if R:
                    env.ray_cast(rays)
            env.sync()
            ms = (time.perf_counter() - t0) * 1e3 / (T1 - T0)
            res["runs"].append({"render": render, "variant": variant, "rep": rep, "ms_per_step": round(ms, 5)})
            print(render, variant, rep, round(ms, 5), flush=True)
    if has:
        hit_rate = {R: None for R in (16, 64)}
        for R in (16, 64):
            env.set_rays(*suites[R])
            hit_rate[R] = round(float((env.ray_cast(host=True)['id'][..., 3] >= 0).mean()), 4)
        res["hit_rate_render" if render else "hit_rate_norender"] = hit_rate
    env.close()
for render in (False, True):
    for variant in VARIANTS:
        v = sorted(r["ms_per_step"] for r in res["runs"] if r["render"] == render and r["variant"] == variant)
        if v:
            res["median_ms_%s_%s" % ('render' if render else 'norender', variant)] = v[len(v) // 2]
print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
