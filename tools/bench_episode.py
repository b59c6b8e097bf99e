#!/usr/bin/env python3
"""Cost of the device-resident goals and episodes on the MI355X, at 4096 envs, 3 objects, 128x128, a table of 512 goals with images:

 (a) the step loop of bench.py's shape (`synthetic_actions`, steps 170-370, with the render), plain and with episode_update(False)
     after every step -- every window starts from the same checkpoint and ends in a synchronise, REPS windows per variant, alternating;
 (b) a goal change of ALL envs: episode_update(True) with every env truncated (one launch + the image kernel + the observation
     refresh, then a synchronise) against the host route it replaces -- reset() + set_object_poses(start poses of the next goals) +
     evaluate._goal_images (the numpy gather of the goal retinas), then a synchronise;
 (c) the image kernel: set_env_goals of all envs and of 1 % of the envs with an image table, against the same calls with a table
     WITHOUT images (upload of the indices, k_env_goals and the wait are in both; the difference is k_goal_image).

    python tools/bench_episode.py [--out FILE.json] [--reps 7]

Medians of wall-clock times around synchronising calls; the first repetition of every variant is a warm-up and is dropped."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--envs', type=int, default=4096)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402
from real_robots_amd.envs.env import Goal  # noqa: E402
from real_robots_amd.evaluate import _goal_images  # noqa: E402

N, G, S, T0, T1 = args.envs, 512, 128, 170, 370
rng = np.random.default_rng(2020)
env = BatchedREALRobotEnv(N, objects=3, width=S, height=S)
env.reset()
home = env.host(nat.F_OBJ_POSE)[0]
start = np.tile(home, (G, 1, 1)).astype(np.float32)
start[:, :, :2] += rng.uniform(-0.05, 0.05, size=(G, 3, 2)).astype(np.float32)
final = np.tile(home[:, :3], (G, 1, 1)).astype(np.float32)
final[:, :, :2] += rng.uniform(-0.1, 0.1, size=(G, 3, 2)).astype(np.float32)
flags = np.full((G, 3), 3, np.uint8)
rgb = rng.integers(0, 256, size=(G, S, S, 3), dtype=np.uint8)
goals = [Goal(retina=rgb[k]) for k in range(G)]
idx = (np.arange(N) % G).astype(np.int32)
res = {"envs": N, "goals": G, "image": [S, S], "reps": args.reps}


def median(v):
    v = sorted(v[1:] if len(v) > 1 else v)
    return round(v[len(v) // 2], 5)


# ---- (a) the step loop, plain and with an update after every step
env.set_goals(start, final, flags, rgb)
env.set_env_goals(idx)
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
ms = {'plain': [], 'update': []}
for rep in range(args.reps):
    for variant in ('plain', 'update'):
        env.restore(ck)
        env.sync()
        t0 = time.perf_counter()
        for t in range(T0, T1):
            env.step(device_ptr=cmds[t].data_ptr(), render=True)
            if variant == 'update':
                env.episode_update(False)
        env.sync()
        ms[variant].append((time.perf_counter() - t0) * 1e3 / (T1 - T0))
        print('a', variant, rep, round(ms[variant][-1], 5), flush=True)
res["a_step_ms_plain"], res["a_step_ms_with_update"] = median(ms['plain']), median(ms['update'])
res["a_step_ms_plain_all"], res["a_step_ms_with_update_all"] = [round(x, 5) for x in ms['plain']], [round(x, 5) for x in ms['update']]

# ---- (b) a goal change of all envs: on the device / over the host
env.set_episode(1, 1)                      # every env is truncated after one step
dev, hst = [], []
for rep in range(args.reps):
    env.step(device_ptr=cmds[T0].data_ptr(), render=False)
    env.sync()
    t0 = time.perf_counter()
    env.episode_update(True)
    env.sync()
    dev.append((time.perf_counter() - t0) * 1e3)
    env.step(device_ptr=cmds[T0].data_ptr(), render=False)
    env.sync()
    gi = (idx + rep + 1) % G
    t0 = time.perf_counter()
    env.reset()
    env.set_object_poses(start[gi])
    img = _goal_images(goals, gi, S, S)
    env.sync()
    hst.append((time.perf_counter() - t0) * 1e3)
    print('b', rep, round(dev[-1], 4), round(hst[-1], 4), flush=True)
assert img.shape == (N, S, S, 3)
assert (env.episode_buffer('episode', host=True) == args.reps).all()
res["b_goal_change_ms_device"], res["b_goal_change_ms_host_route"] = median(dev), median(hst)
env.set_episode(0, 1)

# ---- (c) the image kernel: all envs / 1 % of the envs, with and without images in the table
one = np.zeros(N, np.uint8)
one[::100] = 1
for images in (True, False):
    env.set_goals(start, final, flags, rgb if images else None)
    env.set_env_goals(idx)
    for name, mask in (('all', None), ('1pct', one)):
        v = []
        for rep in range(args.reps):
            gi = ((idx + rep + 1) % G).astype(np.int32)
            env.sync()
            t0 = time.perf_counter()
            env.set_env_goals(gi, mask)
            v.append((time.perf_counter() - t0) * 1e3)
        res["c_set_env_goals_ms_%s_%s" % (name, 'images' if images else 'noimages')] = median(v)
for name in ('all', '1pct'):
    res["c_image_kernel_ms_%s" % name] = round(res["c_set_env_goals_ms_%s_images" % name] - res["c_set_env_goals_ms_%s_noimages" % name], 5)
# bytes WRITTEN per second when all envs change (the table -- 25 MB for 512 goals -- is read many times over and stays in cache)
res["c_image_kernel_written_GBs_all"] = round(N * S * S * 3 / 1e9 / max(res["c_image_kernel_ms_all"] * 1e-3, 1e-9), 1)
env.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
