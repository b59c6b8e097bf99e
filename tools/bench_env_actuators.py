"""Cost of per-env actuators on the headline workload (4096 envs, 3 objects, 128x128 RGB + depth every step, full-range commands):
one handle with the default table (the handle's motor constants in every row) and one whose envs and joints each have drawn values
(kp x 0.8-1.2, kd x 1.0-1.2, max_force x 0.5-1.0, damping x 0.5-2.0: REALRobotVectorEnv's actuator_randomization), timed alternately,
each block in a fresh child process with one handle; then the time of rr_set_env_actuators for all envs and for 64 of them.
Prints one JSON line.

    python tools/bench_env_actuators.py [--envs 4096] [--steps 200] [--blocks 5] [--presettle 150] [--mode both|default|per_env]
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

RANGES = {'kp': (0.8, 1.2), 'kd': (1.0, 1.2), 'max_force': (0.5, 1.0), 'damping': (0.5, 2.0)}


def drawn_actuators(env, rng):
    base = env.default_env_actuators()
    return {k: (base[k] * rng.uniform(lo, hi, size=base[k].shape)).astype(np.float32) for k, (lo, hi) in RANGES.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200, help='steps per timed block')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per mode (alternated, one child process each)')
    ap.add_argument('--presettle', type=int, default=150)
    ap.add_argument('--mode', choices=('both', 'default', 'per_env'), default='both')
    args = ap.parse_args()
    N, W, H = args.envs, 128, 128
    if args.mode == 'both':
        times = {'default': [], 'per_env': []}
        last = {}
        for b in range(args.blocks):
            for m in times:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', m, '--blocks', '1', '--envs', str(N),
                                      '--steps', str(args.steps), '--presettle', str(args.presettle)],
                                     check=True, capture_output=True, text=True).stdout
                last[m] = json.loads(out.strip().splitlines()[-1])
                times[m].append(last[m]['ms_per_step'])
        df, pv = float(np.median(times['default'])), float(np.median(times['per_env']))
        print(json.dumps({
            "workload": "%d envs, 3 objects, 128x128 RGB+depth every step, full-range commands; per-env actuators: %s" % (N, RANGES),
            "ms_per_step_default": round(df, 4), "ms_per_step_per_env": round(pv, 4), "ratio": round(pv / df, 4),
            "blocks_ms_per_step": times, "set_env_actuators_ms_all": last['per_env']['set_env_actuators_ms_all'],
            "set_env_actuators_ms_64": last['per_env']['set_env_actuators_ms_64'], "steps_per_block": args.steps, "blocks": args.blocks}))
        return
    epochs = {}

    def cmd(t):
        k = t // 20
        if k not in epochs:
            epochs.clear()
            epochs[k] = synthetic_actions(range(N), k * 20, hold_prob=0.05)
        return epochs[k]

    rng = np.random.default_rng(0)
    e = BatchedREALRobotEnv(N, objects=3, width=W, height=H, want_mask=False)
    if args.mode == 'per_env':
        e.set_env_actuators(**drawn_actuators(e, rng))
    for t in range(args.presettle):
        e.step(cmd(t), render=True)
    e.sync()
    times, clock = [], args.presettle
    for b in range(args.blocks):
        cmds = [cmd(t) for t in range(clock, clock + args.steps)]
        e.sync()
        t0 = time.perf_counter()
        for c in cmds:
            e.step(c, render=True)
        e.sync()
        times.append(1e3 * (time.perf_counter() - t0) / args.steps)
        clock += args.steps
    assert (e.host(nat.F_ERRFLAGS) & ~np.uint32(8) == 0).all()
    res = {"mode": args.mode, "ms_per_step": round(float(np.median(times)), 4)}
    if args.mode == 'per_env':
        set_all, set_64 = [], []
        m64 = np.zeros(N, np.uint8)
        m64[rng.choice(N, 64, replace=False)] = 1
        for r in range(3):
            a = drawn_actuators(e, rng)
            t0 = time.perf_counter()
            e.set_env_actuators(**a)
            set_all.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            e.set_env_actuators(env_mask=m64, **a)
            set_64.append(1e3 * (time.perf_counter() - t0))
        res.update(set_env_actuators_ms_all=round(float(np.median(set_all)), 2), set_env_actuators_ms_64=round(float(np.median(set_64)), 2))
    print(json.dumps(res))
    e.close()


if __name__ == '__main__':
    main()
