#!/usr/bin/env python3
"""Cost of carried objects in the posture queries on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`,
K = 32 candidate postures per env drawn around each env's own (sigma 0.1 rad), margin 0.05 m; on the `collision` pair table (Q = 92)
and on `carry_pairs(['cube'], exclude_links=<the two finger tips>)`.  Per table, time per call of
  (a) signed_distance_gradient with the feature off -- k_signed_gradient<false>, the kernel as it was before carried objects (its per-item time is to be read against
      profiles/signed_gradient_bench.json; (a) is also taken at that file's K = 8 on the collision table);
  (b) the same call with every env's cube attached to link 8 (captured from the state) -- k_signed_gradient<true>, the other
      instantiation of the one kernel template;
  (c) what one did before: 32 x (write_state of the posture and the composed cube pose + a present-state signed_distance_gradient),
      the composed poses prepared beforehand on the device (link poses of posture_kinematics o rel), not timed.
(a) and (b) ALTERNATE on the same handle -- off, on, off, on --, each turn WARMUP calls and then REPS windows of back-to-back calls on
the library's stream between two HIP events; a turn's figure is its median window, a figure the mean of its two turns.  The ratios
(b)/(a) and (c)/(b) are what profiles/carry_bench.json and NOTEBOOK.md carry.

    python tools/bench_carry.py [--out FILE.json] [--reps N]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--reps', type=int, default=7)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, T0, WARMUP, K, MARGIN, LINK = 4096, 170, 2, 32, 0.05, 8

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
state = env.state
rng = np.random.default_rng(7)
po = (state[:, None, :11] + rng.normal(0.0, 0.1, size=(N, K, 11))).astype(np.float32)
with torch.cuda.stream(stream):
    dev_po = torch.from_numpy(po).cuda()
stream.synchronize()
ptr = dev_po.data_ptr()
L, h = env.L, env.h
links = np.full((N, 3), -1, np.int32)
links[:, 0] = LINK


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


def quat_mul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def rotate(q, v):
    u, w = q[..., :3], q[..., 3:]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def composed_states(rel):
    """[K][N, 61] device tensors: the state with posture k in the joints and the cube at link_pose(posture k) o rel"""
    lp = np.array(env.posture_kinematics(dev_po, host=True)['link_pose'], dtype=np.float64)[:, :, LINK]      # [N, K, 7]
    r = rel[:, None, 0].astype(np.float64)
    pos = lp[..., :3] + rotate(lp[..., 3:], np.broadcast_to(r[..., :3], lp[..., :3].shape))
    quat = quat_mul(lp[..., 3:], np.broadcast_to(r[..., 3:], lp[..., 3:].shape))
    out = []
    for k in range(K):
        s = state.copy()
        s[:, :11], s[:, 22:25], s[:, 25:29] = po[:, k], pos[:, k], quat[:, k]
        with torch.cuda.stream(stream):
            out.append(torch.from_numpy(s).cuda())
    stream.synchronize()
    return out


def table(name, pairs, with_k8):
    env.detach_objects()
    env.set_distance_pairs(pairs)
    Q = len(env.distance_pairs()[0])
    call = lambda: L.rr_signed_gradient(h, ptr, K, 1, MARGIN)
    a, b = [], []
    for _ in range(2):
        env.detach_objects()
        a.append(turn(call, 2))
        env.attach_objects(links)
        b.append(turn(call, 2))
    am, bm = float(np.mean(a)), float(np.mean(b))
    res = {"Q": Q, "calls_per_window": 2, "windows": args.reps, "a_feature_off_us_per_call_turns": a, "b_cube_attached_us_per_call_turns": b,
           "a_feature_off_us_per_call": round(am, 2), "b_cube_attached_us_per_call": round(bm, 2), "a_ns_per_item": round(am * 1e3 / (N * K * Q), 3),
           "b_over_a": round(bm / am, 4)}
    carried = {k: np.array(v) for k, v in env.signed_distance_gradient(dev_po, margin=MARGIN, host=True).items()}
    # (c): the loop this feature retires, on the same handle with the feature off
    rel = env.attachments()[1]
    env.detach_objects()
    rows = composed_states(rel)

    def loop():
        for k in range(K):
            env.write_state(rows[k], joint_pos=True, obj_pose=True)
            L.rr_signed_gradient(h, None, 0, 0, MARGIN)
    c = [turn(loop, 1) for _ in range(2)]
    cm = float(np.mean(c))
    env.write_state(rows[K - 1], joint_pos=True, obj_pose=True)
    last = np.array(env.signed_distance_gradient(margin=MARGIN, host=True)['pair_distance'])
    env.state = state
    res.update(c_write_and_query_loop_us_per_K_turns=c, c_write_and_query_loop_us_per_K=round(cm, 2), c_over_b=round(cm / bm, 4),
               b_against_c_last_row_max_abs_m=float(np.abs(carried['pair_distance'][:, K - 1] - last).max()),
               overlapping_share=round(float(np.isin(carried['pair_status'], (1, 5)).mean()), 5), mean_cost=round(float(carried['cost'].mean()), 6))
    if with_k8:
        with torch.cuda.stream(stream):
            po8 = dev_po[:, :8].contiguous()
        stream.synchronize()
        p8 = po8.data_ptr()
        t8 = [turn(lambda: L.rr_signed_gradient(h, p8, 8, 1, MARGIN), 3) for _ in range(2)]
        res.update(a_K8_us_per_call_turns=t8, a_K8_ns_per_item=round(float(np.mean(t8)) * 1e3 / (N * 8 * Q), 3))
    print(name, json.dumps(res), flush=True)
    return res


tips = ('finger_01', 'finger_11')
res = {"envs": N, "state": "step %d of synthetic_actions" % T0, "K": K, "margin_m": MARGIN, "posture_sigma_rad": 0.1, "attached": "cube -> link %d (%s), captured" % (LINK, nat.LINK_NAMES[LINK]),
       "collision": table('collision', 'collision', True),
       "carry_pairs": dict(table('carry_pairs', BatchedREALRobotEnv.carry_pairs(['cube'], exclude_links=tips), False), exclude_links=list(tips))}
assert env.state.tobytes() == state.tobytes()
env.close()
print(json.dumps(res), flush=True)
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
