"""Cost of per-env cameras on the headline workload (4096 envs, 3 objects, 128x128 RGB + depth every step, full-range commands):
one handle with the shared eye camera and one whose envs each have a drawn camera (translation 3 cm, rotation 3 degrees, fov
75-85: REALRobotVectorEnv's camera_randomization), timed alternately, each block in a fresh child process with one handle (two
4096-env handles in one process share hardware queues: the handle created second is slower whatever its camera); then the time of
rr_set_env_cameras for all envs and for 64 of them.  Prints one JSON line.

    python tools/bench_env_cameras.py [--envs 4096] [--steps 200] [--blocks 5] [--presettle 150] [--mode both|shared|per_env]
(--mode shared / per_env: one handle only, e.g. for a kernel trace of each mode in a run of its own)
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
from real_robots_amd.mathutil import look_at, perspective  # noqa: E402
from real_robots_amd.model import load_model  # noqa: E402


def drawn_cameras(n, W, H, rng, translation=0.03, rotation=3.0, fov=(75.0, 85.0)):
    """[R | t] V0 with R = Rz Ry Rx, as REALRobotVectorEnv(camera_randomization=...) draws them."""
    v0 = look_at((0.01, 0.0, 1.2), np.asarray(load_model()['table_pos'], np.float64), (0.0, 0.0, 1.0))
    views, projs = np.empty((n, 4, 4), np.float32), np.empty((n, 4, 4), np.float32)
    for i in range(n):
        a = np.radians(rng.uniform(-rotation, rotation, 3))
        c, s = np.cos(a), np.sin(a)
        R = (np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]) @ np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
             @ np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]]))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, rng.uniform(-translation, translation, 3)
        views[i] = T @ v0
        projs[i] = perspective(rng.uniform(*fov), W / H, 0.1, 100.0)
    return views, projs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200, help='steps per timed block')
    ap.add_argument('--blocks', type=int, default=5, help='timed blocks per mode (alternated, one child process each)')
    ap.add_argument('--presettle', type=int, default=150)
    ap.add_argument('--mode', choices=('both', 'shared', 'per_env'), default='both')
    args = ap.parse_args()
    N, W, H = args.envs, 128, 128
    if args.mode == 'both':
        times = {'shared': [], 'per_env': []}
        last = {}
        for b in range(args.blocks):
            for m in times:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', m, '--blocks', '1', '--envs', str(N),
                                      '--steps', str(args.steps), '--presettle', str(args.presettle)],
                                     check=True, capture_output=True, text=True).stdout
                last[m] = json.loads(out.strip().splitlines()[-1])
                times[m].append(last[m]['ms_per_step'])
        sh, pv = float(np.median(times['shared'])), float(np.median(times['per_env']))
        print(json.dumps({
            "workload": "%d envs, 3 objects, 128x128 RGB+depth every step, full-range commands; per-env cameras: translation 3 cm, "
                        "rotation 3 deg, fov 75-85" % N,
            "ms_per_step_shared": round(sh, 4), "ms_per_step_per_env": round(pv, 4), "ratio": round(pv / sh, 4),
            "blocks_ms_per_step": times, "set_env_cameras_ms_all": last['per_env']['set_env_cameras_ms_all'],
            "set_env_cameras_ms_64": last['per_env']['set_env_cameras_ms_64'], "steps_per_block": args.steps, "blocks": args.blocks}))
        return
    epochs = {}

    def cmd(t):
        k = t // 20
        if k not in epochs:
            epochs.clear()
            epochs[k] = synthetic_actions(range(N), k * 20, hold_prob=0.05)
        return epochs[k]

    rng = np.random.default_rng(0)
    views, projs = drawn_cameras(N, W, H, rng)
    modes = {args.mode: BatchedREALRobotEnv(N, objects=3, width=W, height=H, want_mask=False)}
    if 'per_env' in modes:
        modes['per_env'].set_env_cameras(views, projs)
    for e in modes.values():
        for t in range(args.presettle):
            e.step(cmd(t), render=True)
        e.sync()
    times = {m: [] for m in modes}
    clock = {m: args.presettle for m in modes}
    for b in range(args.blocks):
        for m, e in modes.items():
            cmds = [cmd(t) for t in range(clock[m], clock[m] + args.steps)]
            e.sync()
            t0 = time.perf_counter()
            for c in cmds:
                e.step(c, render=True)
            e.sync()
            times[m].append(1e3 * (time.perf_counter() - t0) / args.steps)
            clock[m] += args.steps
    for e in modes.values():
        assert (e.host(nat.F_ERRFLAGS) & ~np.uint32(8) == 0).all()
    res = {"mode": args.mode, "ms_per_step": round(float(np.median(times[args.mode])), 4)}
    if args.mode == 'per_env':
        pe = modes['per_env']
        set_all, set_64 = [], []
        m64 = np.zeros(N, np.uint8)
        m64[rng.choice(N, 64, replace=False)] = 1
        for r in range(3):
            v, p = drawn_cameras(N, W, H, rng)
            t0 = time.perf_counter()
            pe.set_env_cameras(v, p)
            set_all.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            pe.set_env_cameras(v, p, env_mask=m64)
            set_64.append(1e3 * (time.perf_counter() - t0))
        res.update(set_env_cameras_ms_all=round(float(np.median(set_all)), 2), set_env_cameras_ms_64=round(float(np.median(set_64)), 2))
    print(json.dumps(res))
    modes[args.mode].close()


if __name__ == '__main__':
    main()
