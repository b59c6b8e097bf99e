"""GPU test (-m gpu) of bench.py's two kinds of run: a plain run prints the headline alone, `--full` adds the per-kernel timing
pass and the roofline on top of the same timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '6', '--warmup', '2', '--presettle', '4',
           '--envs-per-gpu', '64', '--dump-outputs', str(out_dir)] + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {p.stem: np.load(str(p)) for p in sorted(out_dir.glob('*.npy'))}


def test_bench_plain_run_and_full_run(tmp_path):
    """64 envs, 6 timed steps.  The plain run's line has the headline fields, `timed_steps` and `heavy_envs`, "roofline": null and
    neither `secondary` nor `cpu_baseline`.  `--full` (its CPU baseline switched off) adds the roofline with the HIP-event times of
    the kernels of a step, and the observations of the last timed step are the same in both runs."""
    plain, dump_plain = _bench(tmp_path / 'plain')
    full, dump_full = _bench(tmp_path / 'full', '--full', '--no-cpu-baseline')
    for out in (plain, full):
        assert out['unit'] == 'env-steps/s' and out['higher_is_better'] is True and out['dtype'] == 'f32'
        assert out['steps'] == 6 and out['warmup'] == 2 and out['timed_steps'] == [6, 12]
        assert out['value'] > 0 and abs(out['value'] - 64 * 6 / (out['ms_per_step'] * 6e-3)) < 1e-2 * out['value']
        assert out['heavy_envs']['of'] == 64
        assert 'secondary' not in out and 'cpu_baseline' not in out          # (secondary: 4096 envs only)
    assert plain['roofline'] is None
    kernels = full['roofline']['kernels']
    assert kernels['k_raster']['launches'] >= 6 and kernels['k_raster']['avg_ms'] > 0 and 'render_stage' in kernels
    assert full['roofline']['achieved'] > 0 and 'hbm_achievable_GBs' in full['roofline']
    assert sorted(dump_plain) == sorted(dump_full) == ['depth', 'env_ids', 'image_env_ids', 'joints', 'object_poses', 'rgb', 'touch']
    assert all(np.array_equal(dump_plain[k], dump_full[k]) for k in dump_plain)
