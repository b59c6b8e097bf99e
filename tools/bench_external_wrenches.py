"""Cost of external wrenches on the headline workload (4096 envs, 3 objects, 128x128 RGB + depth every step, full-range commands,
default motors): the step with no wrench set (today's launches), with a host-set constant table (`set_external_wrenches(array)` once,
then `step`), with a device-resident table that is rewritten every step (`set_external_wrenches(tensor)` + `step`, two tensors in
turn), and with joint torques and wrenches both on, both rewritten every step.  The four are timed alternately, each block in a fresh
child process with one handle.  Prints one JSON line; --out also writes it to a file (profiles/external_wrenches_bench.json).
--headline-parent / --headline record bench.py's headline (ms per step, runs taken alternately on the parent commit and on this one)
and --kernel-us the kernel's own time from a kernel trace taken in a run of its own, beside the tool's numbers.

    python tools/bench_external_wrenches.py [--envs 4096] [--steps 200] [--blocks 5] [--presettle 150] [--out FILE]
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
from real_robots_amd.model import load_model  # noqa: E402

MODES = ('none', 'host_constant', 'table', 'torques_and_table')
WEIGHTS = 1.0 / 3.0      # forces uniform within +- this x the body's weight, torques within that x 0.05 m
TORQUE_RANGE = 30.0      # N m, uniform in +- this on every joint (tools/bench_joint_torques.py)


def wrench_table(N, rng):
    m = load_model()
    wt = 9.81 * np.concatenate([np.asarray(m['body_mass'], np.float64), np.asarray(m['obj_mass'], np.float64)[:3]])
    w = rng.uniform(-WEIGHTS, WEIGHTS, (N, nat.XW_BODIES, 6)) * wt[None, :, None]
    w[:, :, 3:] *= 0.05
    return w.astype(np.float32)


def floats(s):
    return [float(x) for x in s.split(',')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200, help='steps per timed block')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per mode (alternated, one child process each)')
    ap.add_argument('--presettle', type=int, default=150)
    ap.add_argument('--mode', choices=('all',) + MODES, default='all')
    ap.add_argument('--headline-parent', type=floats, default=None, help="bench.py's ms per step on the parent commit, comma separated")
    ap.add_argument('--headline', type=floats, default=None, help="bench.py's ms per step on this commit, comma separated")
    ap.add_argument('--kernel-us', type=float, default=None, help="k_ext_wrench's own time per launch from a kernel trace")
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
            "workload": "%d envs, 3 objects, 128x128 RGB+depth every step, full-range commands, default motors; wrenches: forces uniform "
                        "within +-%.3g x the body's weight, torques within that x 0.05 m, on all fourteen rows; host_constant: set once "
                        "from a host array; table: two device tensors in turn, set every step; torques_and_table: joint torques (uniform "
                        "+-%g N m, two device tensors in turn) and wrenches both set every step" % (N, WEIGHTS, TORQUE_RANGE),
            "ms_per_step": {m: round(med[m], 4) for m in MODES},
            "ratio_to_none": {m: round(med[m] / med['none'], 4) for m in MODES},
            "added_us_per_step": {m: round(1e3 * (med[m] - med['none']), 2) for m in MODES},
            "blocks_ms_per_step": times, "spread_none": round((max(times['none']) - min(times['none'])) / med['none'], 4),
            "steps_per_block": args.steps, "blocks": args.blocks,
            "joint_torque_table_added_us_per_step": 9.5}
        if args.kernel_us is not None:
            res["k_ext_wrench_us_per_launch"] = args.kernel_us
            res["k_ext_wrench_source"] = "kernel trace of `--mode table` in a run of its own: mean over the launches"
        if args.headline_parent is not None and args.headline is not None:
            p, h = args.headline_parent, args.headline
            res["bench_py_ms_per_step"] = {"parent": p, "this": h, "parent_min_max": [min(p), max(p)],
                                           "within_parent_spread": bool(min(p) <= float(np.median(h)) <= max(p))}
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
    host = [wrench_table(N, rng) for _ in range(2)]
    tables = [torch.from_numpy(w).cuda() for w in host]
    torques = [torch.from_numpy(rng.uniform(-TORQUE_RANGE, TORQUE_RANGE, (N, nat.N_JOINTS)).astype(np.float32)).cuda() for _ in range(2)]
    torch.cuda.synchronize()
    if args.mode == 'host_constant':
        e.set_external_wrenches(host[0])

    def one(t, c):
        if args.mode in ('table', 'torques_and_table'):
            e.set_external_wrenches(tables[t & 1])
        if args.mode == 'torques_and_table':
            e.set_joint_torques(torques[t & 1])
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
