"""Cost of macro actions decided on the host and on the device (rr_step_macro), at 4096 envs x 3 objects, 128x128 RGB + depth every step.

  (a) in phase      every env gets a new uniform request every 1000 steps (evaluate.py's RandomMacro), 2000 steps
  (b) out of phase  each env redraws its request with probability 1/250 per step (torch.where on the device; the same draws for all rows)
      rows: host_numpy        step_macro(numpy request)                       -- the host path as it is
            device            step_macro_device(CUDA tensor)                  -- the decision on the device
            host_from_torch   step_macro(tensor.cpu().numpy())                -- what a policy that lives on the GPU pays today
      the request tensors are produced by torch on the GPU before the timed region; every row in a fresh child process, the rows
      alternated, --repeats times; ms per step = wall clock over the steps, one wait at the end.
  (c) the planner alone  k_plan_macro (plan_macro with a mask of K envs) against k_macro_decide + k_macro_replan (macro_invalidate of the same
      K envs, then step_macro_device) for K = 4096, 256, 16, 1, every call from the same snapshot of scattered postures, no camera.  Each figure
      is the wall clock of the synchronous call minus that of the same call with K = 0 (the same copies, launches and waits; a planner
      that leaves at once), medians of --planner-reps calls.
Prints one JSON line; --out also writes it to a file (profiles/macro_device_bench.json).

    python tools/bench_macro_device.py [--envs 4096] [--steps 2000] [--repeats 3] [--out FILE]
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

ROWS = ('host_numpy', 'device', 'host_from_torch')
LOW, HIGH = [-0.25, -0.5, -0.25, -0.5], [0.05, 0.5, 0.05, 0.5]      # macro_space, env.py:49-52


def request_tensors(N, steps, phase, seed):
    """The request of every step as a list of CUDA tensors [N, 4] (a step without a redraw shares its predecessor's tensor)."""
    import torch
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    lo, hi = torch.tensor(LOW, device='cuda'), torch.tensor(HIGH, device='cuda')
    draw = lambda: lo + (hi - lo) * torch.rand((N, 4), generator=g, device='cuda')
    out = [draw()]
    for t in range(1, steps):
        if phase == 'in':
            out.append(draw() if t % 1000 == 0 else out[-1])
        else:
            redraw = torch.rand((N, 1), generator=g, device='cuda') < (1.0 / 250.0)
            out.append(torch.where(redraw, draw(), out[-1]))
    torch.cuda.synchronize()
    return out


def run_row(args):
    N = args.envs
    req = request_tensors(N, args.steps, args.phase, 1234)
    host = [r.cpu().numpy().reshape(N, 2, 2) for r in req] if args.row == 'host_numpy' else None
    e = BatchedREALRobotEnv(N, objects=3, width=128, height=128, want_mask=False)
    e.step(None, render=True)
    e.sync()
    t0 = time.perf_counter()
    for t in range(args.steps):
        if args.row == 'device':
            e.step_macro_device(req[t], render=True)
        elif args.row == 'host_numpy':
            e.step_macro(host[t], render=True)
        else:
            e.step_macro(req[t].cpu().numpy().reshape(N, 2, 2), render=True)
    e.sync()
    ms = 1e3 * (time.perf_counter() - t0) / args.steps
    print(json.dumps({"row": args.row, "phase": args.phase, "ms_per_step": round(ms, 4)}))
    e.close()


def run_planner(args):
    import torch
    N = args.envs
    e = BatchedREALRobotEnv(N, objects=3, width=64, height=64, want_mask=False)
    rng = np.random.default_rng(0)
    s = e.state
    s[:, :7] = rng.uniform(-0.8, 0.8, size=(N, 7)).astype(np.float32)
    s[:, 7:22] = 0.0
    e.write_state(s, joint_pos=True, joint_vel=True)
    e.snapshot_slots(1)
    m = rng.uniform(LOW, HIGH, size=(N, 4)).astype(np.float32)
    md = torch.as_tensor(m, device='cuda')
    torch.cuda.synchronize()
    e.step_macro_device(md)          # the buffers exist, every record holds its request
    e.sync()
    res = {}
    for K in [0] + [k for k in (4096, 256, 16, 1) if k <= N]:
        mask = np.zeros(N, np.uint8)
        mask[rng.choice(N, K, replace=False)] = 1
        mask_dev = torch.as_tensor(mask, device='cuda')
        torch.cuda.synchronize()
        t_plan, t_dev = [], []
        for _ in range(args.planner_reps):
            e.load_snapshot(0)
            e.sync()
            t0 = time.perf_counter()
            e.plan_macro(m.reshape(N, 2, 2), mask)
            t_plan.append(1e3 * (time.perf_counter() - t0))
            e.load_snapshot(0)
            e.macro_invalidate(mask_dev)
            e.sync()
            t0 = time.perf_counter()
            e.step_macro_device(md)
            e.sync()
            t_dev.append(1e3 * (time.perf_counter() - t0))
            # every call of either kind leaves the records equal to the requests
        res[K] = (float(np.median(t_plan)), float(np.median(t_dev)))
    out = {"calls_ms": {str(k): {"plan_macro": round(v[0], 4), "step_macro_device": round(v[1], 4)} for k, v in res.items()},
           "kernel_ms": {str(k): {"k_plan_macro": round(v[0] - res[0][0], 4), "k_macro_replan": round(v[1] - res[0][1], 4)} for k, v in res.items() if k}}
    print(json.dumps(out))
    e.close()


def child(extra):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--planner-reps', type=int, default=7)
    ap.add_argument('--row', choices=ROWS + ('planner',), default=None)
    ap.add_argument('--phase', choices=('in', 'out'), default='in')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.row == 'planner':
        return run_planner(args)
    if args.row:
        return run_row(args)
    common = ['--envs', str(args.envs), '--steps', str(args.steps)]
    res = {"workload": "%d envs, 3 objects, 128x128 RGB+depth every step, %d steps; in phase: a new uniform request for every env every 1000 "
                       "steps; out of phase: each env redraws with probability 1/250 per step" % (args.envs, args.steps),
           "planner": child(common + ['--row', 'planner', '--planner-reps', str(args.planner_reps)])}
    for phase in ('in', 'out'):
        times = {r: [] for r in ROWS}
        for _ in range(args.repeats):
            for r in ROWS:
                times[r].append(child(common + ['--row', r, '--phase', phase])['ms_per_step'])
        med = {r: float(np.median(times[r])) for r in ROWS}
        res[phase + '_phase'] = {"ms_per_step": {r: round(med[r], 4) for r in ROWS}, "runs_ms_per_step": times,
                                 "device_over_host_numpy": round(med['device'] / med['host_numpy'], 4),
                                 "device_over_host_from_torch": round(med['device'] / med['host_from_torch'], 4),
                                 "spread": {r: round((max(times[r]) - min(times[r])) / med[r], 4) for r in ROWS}}
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
