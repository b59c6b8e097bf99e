#!/usr/bin/env python3
"""Cost of rr_carried_sweep on the MI355X: 4096 envs, 3 objects, the states of step 170 of `synthetic_actions`; every env's cube attached
to the gripper base at a given pose past the finger tips; the pair table `carry_pairs(['cube'], exclude_links=the two finger tips)`;
K = 8 segments per env from each env's own posture to one drawn around it with |dq|inf = 0.1 and 0.5 rad (uniform per joint, one joint
at the full span); safety 0.01 m, tolerance 1e-3 m.

Per span, WARMUP calls, then REPS rounds in which windows of back-to-back calls alternate on the library's stream, each between two HIP
events; the medians give the milliseconds per call:
  (a) one carried_sweep call on the attached handle;
  (b) what one does today: eight posture_clearance calls at K = 32, the 32 uniform samples of each of the eight segments, on the
      attached handle;
  (c) the cost of the CARRY instantiation alone: carried_sweep on an attached handle whose envs are all masked free
      (k_swept_clearance<true> runs, every row stages its objects from the state) against swept_clearance on a handle that never
      attached (k_swept_clearance<false>, the other instantiation of the one kernel template), the same states, table and segments;
      their bytes are compared as well (`restated_over_original` in the output: the key keeps the name it has in the recorded profile).
Also the statuses, the steps and the pair evaluations per segment, the share of rows at the step cap, and how many segments the
sampling check calls free that the sweep stops.

    python tools/bench_carried_sweep.py [--out FILE.json] [--reps 11]"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--label', default='shipped: k_swept_clearance<true>, the objects re-staged at every step from the table rows in LDS')
ap.add_argument('--reps', type=int, default=11)
ap.add_argument('--envs', type=int, default=4096)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

N, T0, WARMUP, K, SAMPLES, SAFETY, TOLERANCE = args.envs, 170, 3, 8, 32, 0.01, 1e-3
REL = (0.0, 0.0, 0.24, 0.0, 0.0, 0.0, 1.0)          # the cube in the COM frame of the gripper base: past the finger tips

stream = torch.cuda.Stream()
env = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)
for t in range(T0):
    if t % 20 == 0:
        cmd = synthetic_actions(list(range(N)), t, hold_prob=0.05).astype(np.float32)
    env.step(cmd)
env.sync()
state = env.state
plain = BatchedREALRobotEnv(N, objects=3, width=64, height=64, stream=stream.cuda_stream)          # never attaches
plain.state = state
pairs = BatchedREALRobotEnv.carry_pairs(['cube'], exclude_links=('finger_01', 'finger_11'))
Q = len(pairs)
for h in (env, plain):
    h.set_distance_pairs(pairs)
rng = np.random.default_rng(11)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(calls):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def stats(ms):
    return {"ms_per_call_median": round(float(np.median(ms)), 3), "ms_per_call_min": round(float(min(ms)), 3), "ms_per_call_max": round(float(max(ms)), 3)}


res = {"label": args.label, "envs": N, "K": K, "Q": Q, "state": "step %d of synthetic_actions" % T0, "rounds": args.reps, "safety_m": SAFETY, "tolerance_m": TOLERANCE,
       "attachment": "every env's cube on the gripper base, rel pose %s" % (REL,), "samples_per_segment_of_the_sampling_check": SAMPLES, "spans": {}}
for span in (0.1, 0.5):
    dq = rng.uniform(-span, span, size=(N, K, 11))
    dq[np.arange(N)[:, None], np.arange(K)[None, :], rng.integers(0, 11, size=(N, K))] = span
    seg = np.zeros((N, K, 2, 11), np.float32)
    seg[:, :, 0] = state[:, None, :11]
    seg[:, :, 1] = seg[:, :, 0] + dq.astype(np.float32)
    ts = (np.arange(SAMPLES) / (SAMPLES - 1.0)).astype(np.float32)
    samples = [np.ascontiguousarray(seg[:, k, None, 0] + ts[None, :, None] * (seg[:, k, None, 1] - seg[:, k, None, 0])) for k in range(K)]      # K x [N, 32, 11]
    with torch.cuda.stream(stream):
        dev_seg = torch.from_numpy(seg).cuda()
        dev_samples = [torch.from_numpy(s).cuda() for s in samples]
    stream.synchronize()

    def carried():
        env.carried_sweep(dev_seg, SAFETY, TOLERANCE)

    def sampling():
        for k in range(K):
            env.posture_clearance(dev_samples[k])

    def original():
        plain.swept_clearance(dev_seg, SAFETY, TOLERANCE)

    # (c) first: the attached handle with every env masked free
    env.attach_objects({'cube': 'base'}, rel_pose=REL)
    env.detach_objects(env_mask=np.ones(N, np.uint8))
    for _ in range(WARMUP):
        carried()
        original()
    env.sync()
    free_new, free_old = [], []
    for _ in range(args.reps):
        free_new.append(window(carried, 4))
        free_old.append(window(original, 4))
    env.carried_sweep(dev_seg, SAFETY, TOLERANCE)
    plain.swept_clearance(dev_seg, SAFETY, TOLERANCE)
    same = all(env.sweep_buffer(w, host=True).tobytes() == plain.sweep_buffer(w, host=True).tobytes() for w in range(4))
    # (a) and (b): every cube on the gripper base
    env.attach_objects({'cube': 'base'}, rel_pose=REL)
    for _ in range(WARMUP):
        carried()
        sampling()
    env.sync()
    new, old = [], []
    for _ in range(args.reps):
        new.append(window(carried, 4))
        old.append(window(sampling, 1))
    out = {k: np.array(v) for k, v in env.carried_sweep(dev_seg, SAFETY, TOLERANCE, host=True).items()}
    sampled_min = np.stack([np.array(env.posture_clearance(dev_samples[k], host=True)['pair_distance']).min(axis=(1, 2)) for k in range(K)], 1)      # [N, K]
    sampled_free = sampled_min > SAFETY
    st = out['status']
    row = {"a_carried_sweep": stats(new), "b_eight_posture_clearance_calls_at_K_32": stats(old),
           "sampling_over_carried_sweep": round(float(np.median(old) / np.median(new)), 2),
           "c_carried_sweep_all_envs_masked_free": stats(free_new), "c_swept_clearance_never_attached": stats(free_old),
           "restated_over_original": round(float(np.median(free_new) / np.median(free_old)), 3), "c_bytes_equal": bool(same),
           "status_counts": {str(s): int((st == s).sum()) for s in (0, 1, 3)}, "share_of_rows_at_the_step_cap": round(float((st == 3).mean()), 4),
           "steps_per_segment": {"mean": round(float(out['steps'].mean()), 2), "median": float(np.median(out['steps'])), "max": int(out['steps'].max())},
           "pair_evaluations_per_segment": {"mean": round(float(out['evaluations'].mean()), 1), "median": float(np.median(out['evaluations'])), "max": int(out['evaluations'].max())},
           "mean_fraction_proved_free_at_the_step_cap": round(float(out['fraction'][st == 3].mean()), 3) if (st == 3).any() else None,
           "pair_evaluations_of_the_sampling_check_per_segment": SAMPLES * Q,
           "evaluations_sampling_over_sweep": round(SAMPLES * Q / float(out['evaluations'].mean()), 1),
           "segments_free_by_sampling": int(sampled_free.sum()), "segments_free_by_sweep": int((st == 0).sum()),
           "free_by_sampling_but_stopped_by_sweep": int((sampled_free & (st != 0)).sum()),
           "free_by_sweep_but_not_by_sampling": int((~sampled_free & (st == 0)).sum())}
    res["spans"]["%.1f" % span] = row
    print('span', span, json.dumps(row), flush=True)
env.close()
plain.close()
if args.out:
    json.dump(res, open(args.out, 'w'), indent=1)
