"""Cost of cartesian actions decided on the host and on the device (rr_step_cartesian), at 4096 envs x 3 objects, 128x128 RGB + depth every step.
Targets are the gripper base's pose at in-limit postures (the forward kinematics of uniform draws in +-0.8 rad, float64 on the host, made
before the timed region).

  workloads  every      every env gets a new target on every step
             sparse     each env redraws its target with probability 1/50 per step (torch.where on the device; the same draws for all rows)
             constant   the targets never change
  rows       device            step_cartesian_device(CUDA tensors)                        -- the decision on the device
             host_numpy        the host loop on numpy arrays: record, ik(), step(cmd)     -- the host path as it is
             host_from_torch   the same loop fed by tensor.cpu().numpy()                  -- what a policy that lives on the GPU pays today
      every row in a fresh child process, the rows alternated, --repeats times; ms per step = wall clock over the steps, one wait at the end.
  solver alone  k_ik (ik() of all N envs: the kernel has no mask) against k_cart_decide + k_cart_solve (cartesian_invalidate of K envs, then
      step_cartesian_device) for K = 4096, 256, 16, 1, every call from the same snapshot of scattered postures, no camera.  The device figure is
      the wall clock of the synchronous call minus that of the same call with K = 0 (the same launches and the step; a solver that leaves at
      once); the k_ik figure is ik()'s wall clock minus that of a state read (a copy and a wait), medians of --solver-reps calls.
Prints one JSON line; --out also writes it to a file (profiles/cartesian_device_bench.json).

    python tools/bench_cartesian_device.py [--envs 4096] [--steps 300] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402

ROWS = ('device', 'host_numpy', 'host_from_torch')
WORKLOADS = ('every', 'sparse', 'constant')
POOL = 8      # target sets the `every` and `sparse` workloads draw from


def pose_pool(N, seed):
    """POOL target sets float32 [POOL, N, 7]: the gripper base's pose at N uniform postures in +-0.8 rad (oracle.kinematics, float64),
    and the same poses handed round the envs (set a: env i takes pose i + 17 a)."""
    from oracle.kinematics import EE_LINK, link_pose
    rng = np.random.default_rng(seed)
    base = np.empty((N, 7), np.float32)
    q11 = np.zeros(11)
    for i in range(N):
        q11[:7] = rng.uniform(-0.8, 0.8, size=7)
        R, p = link_pose(q11, EE_LINK)
        w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
        x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
        y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
        z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
        base[i, :3], base[i, 3:] = p, np.array([x, y, z, w]) / np.linalg.norm([x, y, z, w])
    return np.stack([np.roll(base, -17 * a, axis=0) for a in range(POOL)])


def target_tensors(N, steps, workload, seed):
    """The targets of every step as a list of CUDA tensors [N, 7] (a step without a redraw shares its predecessor's tensor)."""
    import torch
    pool = torch.as_tensor(pose_pool(N, seed), device='cuda')
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    out = [pool[0].clone()]
    for t in range(1, steps):
        if workload == 'constant':
            out.append(out[-1])
        elif workload == 'every':
            out.append((pool[t % POOL] + 1e-4 * (t // POOL)).contiguous())      # (a new request for every env: no two steps share a row)
        else:
            redraw = torch.rand((N, 1), generator=g, device='cuda') < (1.0 / 50.0)
            out.append(torch.where(redraw, pool[t % POOL] + 1e-4 * (t // POOL), out[-1]).contiguous())
    torch.cuda.synchronize()
    return out


def run_row(args):
    import torch
    N = args.envs
    req = target_tensors(N, args.steps, args.workload, 1234)
    grip = torch.zeros((N, 2), device='cuda')
    grip_host = np.zeros((N, 2), np.float32)
    host = [r.cpu().numpy() for r in req] if args.row == 'host_numpy' else None
    e = BatchedREALRobotEnv(N, objects=3, width=128, height=128, want_mask=False)
    e.step(None, render=True)
    e.sync()
    rec, sol = np.full((N, 7), np.nan, np.float32), np.zeros((N, 7), np.float32)
    solves = 0
    t0 = time.perf_counter()
    for t in range(args.steps):
        if args.row == 'device':
            e.step_cartesian_device(req[t], grip, render=True)
            continue
        c = host[t] if args.row == 'host_numpy' else req[t].cpu().numpy()
        g = grip_host if args.row == 'host_numpy' else grip.cpu().numpy()
        need = ~np.all(c == rec, axis=1)
        if need.any():
            q, _ = e.ik(c)
            sol[need], rec[need] = q[need, :7], c[need]
            solves += int(need.sum())
        e.step(np.concatenate([sol, g], axis=1), render=True)
    e.sync()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    print(json.dumps({"row": args.row, "workload": args.workload, "ms_per_step": round(ms, 4), "host_solves": solves}))
    e.close()


def run_solver(args):
    import torch
    N = args.envs
    e = BatchedREALRobotEnv(N, objects=3, width=64, height=64, want_mask=False)
    rng = np.random.default_rng(0)
    s = e.state
    s[:, :7] = rng.uniform(-0.8, 0.8, size=(N, 7)).astype(np.float32)
    s[:, 7:22] = 0.0
    e.write_state(s, joint_pos=True, joint_vel=True)
    e.snapshot_slots(1)
    t = pose_pool(N, 5)[0]
    td, gd = torch.as_tensor(t, device='cuda'), torch.zeros((N, 2), device='cuda')
    torch.cuda.synchronize()
    e.step_cartesian_device(td, gd)          # the buffers exist, every record holds its request
    e.ik(t)
    e.sync()
    res = {}
    for K in [0] + [k for k in (4096, 256, 16, 1) if k <= N]:
        mask = np.zeros(N, np.uint8)
        mask[rng.choice(N, K, replace=False)] = 1
        mask_dev = torch.as_tensor(mask, device='cuda')
        torch.cuda.synchronize()
        t_ik, t_read, t_dev = [], [], []
        for _ in range(args.solver_reps):
            e.load_snapshot(0)
            e.sync()
            t0 = time.perf_counter()
            e.ik(t)
            t_ik.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            e.state
            t_read.append(1e3 * (time.perf_counter() - t0))
            e.load_snapshot(0)
            e.cartesian_invalidate(mask_dev)
            e.sync()
            t0 = time.perf_counter()
            e.step_cartesian_device(td, gd)
            e.sync()
            t_dev.append(1e3 * (time.perf_counter() - t0))
        res[K] = (float(np.median(t_ik)), float(np.median(t_read)), float(np.median(t_dev)))
    out = {"calls_ms": {str(k): {"ik": round(v[0], 4), "state_read": round(v[1], 4), "step_cartesian_device": round(v[2], 4)} for k, v in res.items()},
           "kernel_ms": {str(k): {"k_ik_all_envs": round(v[0] - v[1], 4), "k_cart_decide_solve": round(v[2] - res[0][2], 4)} for k, v in res.items() if k}}
    print(json.dumps(out))
    e.close()


def child(extra):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--solver-reps', type=int, default=7)
    ap.add_argument('--row', choices=ROWS + ('solver',), default=None)
    ap.add_argument('--workload', choices=WORKLOADS, default='every')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.row == 'solver':
        return run_solver(args)
    if args.row:
        return run_row(args)
    common = ['--envs', str(args.envs), '--steps', str(args.steps)]
    res = {"workload": "%d envs, 3 objects, 128x128 RGB+depth every step, %d steps; every: a new target for every env on every step; sparse: each env "
                       "redraws with probability 1/50 per step; constant: the targets never change" % (args.envs, args.steps),
           "solver": child(common + ['--row', 'solver', '--solver-reps', str(args.solver_reps)])}
    for w in WORKLOADS:
        times = {r: [] for r in ROWS}
        for _ in range(args.repeats):
            for r in ROWS:
                times[r].append(child(common + ['--row', r, '--workload', w])['ms_per_step'])
        med = {r: float(np.median(times[r])) for r in ROWS}
        res[w] = {"ms_per_step": {r: round(med[r], 4) for r in ROWS}, "runs_ms_per_step": times,
                  "device_over_host_numpy": round(med['device'] / med['host_numpy'], 4),
                  "device_over_host_from_torch": round(med['device'] / med['host_from_torch'], 4),
                  "spread": {r: round((max(times[r]) - min(times[r])) / med[r], 4) for r in ROWS}}
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
