"""Cost of joint torque inputs on the headline workload (4096 envs, 3 objects, 128x128 RGB + depth every step, full-range commands,
default motors -- the torques are feed-forward under the position motors): the step with no torque set (today's launches), the step
with a device-resident table that changes every step (`set_joint_torques(tensor)` + `step`), and the gravity-compensated loop
`posture_dynamics()` -> `set_joint_torques(bias)` -> `step`.  The three are timed alternately, each block in a fresh child process
with one handle.  Prints one JSON line; --out also writes it to a file (profiles/joint_torques_bench.json).

    python tools/bench_joint_torques.py [--envs 4096] [--steps 200] [--blocks 5] [--presettle 150] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from real_robots_amd import _native as nat  # noqa: E402
from real_robots_amd.batched import BatchedREALRobotEnv  # noqa: E402
from real_robots_amd.distributed import synthetic_actions  # noqa: E402

MODES = ('none', 'table', 'gravity')
TORQUE_RANGE = 30.0      # N m, uniform in +- this on every joint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200, help='steps per timed block')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per mode (alternated, one child process each)')
    ap.add_argument('--presettle', type=int, default=150)
    ap.add_argument('--mode', choices=('all',) + MODES, default='all')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    N, W, H = args.envs, 128, 128
    if args.mode == 'all':
        times = {m: [] for m in MODES}
        for b in range(args.blocks):
            for m in MODES:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', m, '--blocks', '1', '--envs', str(N),
                                      '--steps', str(args.steps), '--presettle', str(args.presettle)],
                                     check=True, capture_output=True, text=True).stdout
                times[m].append(json.loads(out.strip().splitlines()[-1])['ms_per_step'])
        med = {m: float(np.median(times[m])) for m in MODES}
        res = {
            "workload": "%d envs, 3 objects, 128x128 RGB+depth every step, full-range commands, default motors; table: uniform +-%g N m, "
                        "two device tensors in turn; gravity: posture_dynamics() -> set_joint_torques(bias) -> step" % (N, TORQUE_RANGE),
            "ms_per_step": {m: round(med[m], 4) for m in MODES},
            "ratio_to_none": {m: round(med[m] / med['none'], 4) for m in MODES},
            "added_us_per_step": {m: round(1e3 * (med[m] - med['none']), 2) for m in MODES},
            "blocks_ms_per_step": times, "spread_none": round((max(times['none']) - min(times['none'])) / med['none'], 4),
            "steps_per_block": args.steps, "blocks": args.blocks}
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(json.dumps(res, indent=1) + '\n')
        return
    import torch
    epochs = {}

    def cmd(t):
        k = t // 20
        if k not in epochs:
            epochs.clear()
            epochs[k] = synthetic_actions(range(N), k * 20, hold_prob=0.05)
        return epochs[k]

    rng = np.random.default_rng(0)
    e = BatchedREALRobotEnv(N, objects=3, width=W, height=H, want_mask=False)
    tables = [torch.from_numpy(rng.uniform(-TORQUE_RANGE, TORQUE_RANGE, (N, nat.N_JOINTS)).astype(np.float32)).cuda() for _ in range(2)]
    torch.cuda.synchronize()

    def one(t, c):
        if args.mode == 'table':
            e.set_joint_torques(tables[t & 1])
        elif args.mode == 'gravity':
            e.set_joint_torques(e.posture_dynamics()['bias'])
        e.step(c, render=True)

    for t in range(args.presettle):
        one(t, cmd(t))
    e.sync()
    times, clock = [], args.presettle
    for b in range(args.blocks):
        cmds = [cmd(t) for t in range(clock, clock + args.steps)]
        e.sync()
        t0 = time.perf_counter()
        for t, c in enumerate(cmds):
            one(t, c)
        e.sync()
        times.append(1e3 * (time.perf_counter() - t0) / args.steps)
        clock += args.steps
    assert (e.host(nat.F_ERRFLAGS) & ~np.uint32(8) == 0).all()
    print(json.dumps({"mode": args.mode, "ms_per_step": round(float(np.median(times)), 4)}))
    e.close()


if __name__ == '__main__':
    main()
