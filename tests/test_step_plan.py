"""The schedule of a step as a decision (real_robots_amd/csrc/rr_plan.inc, plan_step): which placement and which launch shapes a
(batch size, tiles, settings, reading of the two lagged list lengths) maps to -- checked on the CPU.  The file is compiled alone
with g++ into a program that reads PlanIn rows and prints StepPlan rows; its output is compared with a restatement of the
decisions in numpy, written from the expressions rr_host.inc held when they were spread over rr_step, step_split, step_single,
launch_solve_class and launch_render (each with its own read of the counters and its own fallback), over both sides of every
threshold; then the rows of DESIGN.md 5.2's table and the configurations the GPU tests force are looked up by name.
"""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'real_robots_amd', 'csrc')

IN_FIELDS = ('N', 'ntiles', 'render_mode', 'timing', 'split_heavy', 'lookahead', 'coop_all', 'split_max_pct', 'h', 'vh', 'known')
OUT_FIELDS = ('path', 'mostly_heavy', 'h_long', 'heavy_render', 'coop_h', 'coop_vh_beside', 'coop_vh_alone', 'la_on_vh', 'la_side',
              'vh_render_on_main', 'vh_render_on_aux', 'small_n', 'single_solve', 'la_beside')
SPLIT, SPLIT_TIMED, SINGLE = 0, 1, 2                      # StepPlan::path
WALKER, RASTER_LIST, GRID = 0, 1, 2                       # StepPlan::heavy_render
CHAIN_N1, SIDE_BY_SIDE, WAVE_PER_ENV, PACKED = 0, 1, 2, 3  # StepPlan::single_solve

DRIVER = r'''
#include <cstdio>
#include "rr_plan.inc"
int main() {
    int v[%d];
    for (;;) {
        for (int &x : v) if (scanf("%%d", &x) != 1) return 0;
        PlanIn in;
        in.N = v[0]; in.ntiles = v[1]; in.render_mode = v[2]; in.timing = v[3] != 0;
        in.split_heavy = v[4] != 0; in.lookahead = v[5] != 0; in.coop_all = v[6] != 0; in.split_max_pct = v[7];
        in.counts.h = v[8]; in.counts.vh = v[9]; in.counts.known = v[10] != 0;
        const StepPlan p = plan_step(in);
        const int out[] = {(int)p.path, p.mostly_heavy, p.h_long, (int)p.heavy_render, p.coop_h, p.coop_vh_beside, p.coop_vh_alone, p.la_on_vh, p.la_side,
                           p.vh_render_on_main, p.vh_render_on_aux, p.small_n, (int)p.single_solve, p.la_beside};
        char line[sizeof out / sizeof out[0] + 2];
        int n = 0;
        for (int x : out) line[n++] = (char)('0' + x);      // (every field is a single digit)
        line[n++] = '\n';
        fwrite(line, 1, n, stdout);
    }
}
''' % len(IN_FIELDS)


@pytest.fixture(scope='module')
def plan_program(tmp_path_factory):
    """rr_plan.inc compiled ALONE (no HIP, no rr_env) under -Wall -Wextra -Werror; returns rows of PlanIn -> rows of StepPlan."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    tmp = tmp_path_factory.mktemp('plan')
    src, exe = tmp / 'plan_main.cpp', tmp / 'plan_main'
    src.write_text(DRIVER)
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-O1', '-I', CSRC, str(src), '-o', str(exe)], check=True)

    def run(rows):
        rows = np.asarray(rows, np.int64).reshape(-1, len(IN_FIELDS))
        text = '\n'.join(' '.join(map(str, r)) for r in rows.tolist())
        out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True).stdout
        got = np.frombuffer(out, np.uint8).reshape(len(rows), len(OUT_FIELDS) + 1)
        assert (got[:, -1] == ord('\n')).all()
        return got[:, :-1].astype(np.int64) - ord('0')
    return run


def mirror(rows):
    """The decisions as the host code made them before there was a plan: `count(which, fallback)` is the old per-decision read."""
    r = {k: np.asarray(rows, np.int64).reshape(-1, len(IN_FIELDS))[:, i] for i, k in enumerate(IN_FIELDS)}
    N, nt, pct = r['N'], r['ntiles'], r['split_max_pct']
    render, timing, known = r['render_mode'] != 0, r['timing'] != 0, r['known'] != 0
    split_heavy, ahead, coop_all = (r[k] != 0 for k in ('split_heavy', 'lookahead', 'coop_all'))
    count = lambda which, fallback: np.where(known, r[('h', 'vh')[which]], fallback)
    o = {}
    # rr_step
    o['mostly_heavy'] = count(0, 0) * 100 > N * pct
    split = render & split_heavy & ~o['mostly_heavy'] & ~((N == 1) & ~timing)
    o['path'] = np.where(split, np.where(timing, SPLIT_TIMED, SPLIT), SINGLE)
    # launch_render (sel 2)
    walker = count(0, N) * nt <= 768
    grid = count(0, 0) * 3 > N
    o['heavy_render'] = np.where(walker, WALKER, np.where(grid, GRID, RASTER_LIST))
    # launch_solve_class (sel 2; sel 3 beside a raster; sel 3 in a step without camera)
    h_long = count(0, 0) * nt > 768
    o['h_long'] = h_long
    o['coop_h'] = count(0, N) <= 256
    o['coop_vh_beside'] = count(1, N) <= np.where(~h_long, 512, 256)
    o['coop_vh_alone'] = count(1, N) <= 512
    # step_split
    o['la_on_vh'] = ahead & ((count(1, 0) <= 64) | ~h_long)
    o['la_side'] = ahead & ~o['la_on_vh']
    o['vh_render_on_main'] = o['la_on_vh'] & h_long
    o['vh_render_on_aux'] = o['la_on_vh'] & ~o['vh_render_on_main']
    # step_single
    o['small_n'] = (N <= 64) & split_heavy & ~timing
    side = ~render & (N > 1024) & split_heavy & ~timing & (count(1, 0) >= 64)
    wave = coop_all & (N <= 1024) & split_heavy
    o['single_solve'] = np.where(o['small_n'] & (N == 1), CHAIN_N1, np.where(side, SIDE_BY_SIDE, np.where(wave, WAVE_PER_ENV, PACKED)))
    o['la_beside'] = ahead & render & ~timing & ~o['small_n']
    return np.stack([np.asarray(o[k], np.int64) for k in OUT_FIELDS], 1)


def product_rows():
    """Every N x tiles x render mode x timing x one setting off in turn x split_max_pct, with both sides of every threshold for h and
    vh (the threshold and the threshold + 1, and N), and the case of no reading at all."""
    settings = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)]     # split_heavy, lookahead, coop_all: the defaults, then each flipped
    rows = []
    for N, nt, pct in itertools.product((1, 2, 64, 65, 448, 1024, 1025, 1100, 4096), (1, 4, 12), (0, 2, 60)):
        thresholds = (0, 64, 256, 512, 768 // nt, N // 3, N * pct // 100)
        values = sorted({t + d for t in thresholds for d in (0, 1)} | {N})
        counts = [(h, vh, 1) for h in values for vh in values] + [(0, 0, 0)]
        for render, timing, s, c in itertools.product((0, 1, 2), (0, 1), settings, counts):
            rows.append((N, nt, render, timing) + s + (pct,) + c)
    return np.array(rows, np.int64)


def row(N, ntiles, h=0, vh=0, known=1, render_mode=1, timing=0, split_heavy=1, lookahead=1, coop_all=1, split_max_pct=60):
    return (N, ntiles, render_mode, timing, split_heavy, lookahead, coop_all, split_max_pct, h, vh, known)


def placement(inp, plan):
    """The row of DESIGN.md 5.2's table a plan is."""
    i, p = dict(zip(IN_FIELDS, inp)), dict(zip(OUT_FIELDS, plan))
    if p['path'] == SPLIT_TIMED:
        return '5'
    if p['path'] == SPLIT:
        return '2' if p['la_side'] else ("1'" if p['vh_render_on_main'] else ('1' if p['la_on_vh'] else '5'))
    if p['small_n']:
        return '4'
    if p['single_solve'] == SIDE_BY_SIDE:
        return '3b'
    return '3' if i['split_heavy'] and i['lookahead'] else '5'


def test_plan_is_the_decisions_the_host_code_made(plan_program):
    rows = product_rows()
    got, want = plan_program(rows), mirror(rows)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (len(bad), dict(zip(IN_FIELDS, rows[bad[0]])), dict(zip(OUT_FIELDS, got[bad[0]])), dict(zip(OUT_FIELDS, want[bad[0]])))
    # (the product reaches every value of every field)
    for k, n in zip(OUT_FIELDS, (3, 2, 2, 3, 2, 2, 2, 2, 2, 2, 2, 2, 4, 2)):
        assert len(np.unique(got[:, OUT_FIELDS.index(k)])) == n, k


def test_the_named_workloads_take_the_rows_of_the_design_table(plan_program):
    """4096 envs at 128 x 128 (4 tiles)."""
    named = [
        ('early window', row(4096, 4, 40, 3)),
        ('late window', row(4096, 4, 650, 3)),
        ('macro', row(4096, 4, 1848, 368)),
        ('macro without camera', row(4096, 4, 1848, 368, render_mode=0)),
        ('16 envs without camera', row(16, 4, 0, 0, render_mode=0)),
        ('gym facade', row(1, 4, 0, 0)),
        ('16 envs with camera', row(16, 4, 0, 0)),
    ]
    plans = {name: (r, dict(zip(OUT_FIELDS, p))) for (name, r), p in zip(named, plan_program([r for _, r in named]))}
    where = {name: placement(r, list(p.values())) for name, (r, p) in plans.items()}
    # (the one chain of a handful of envs is the form of their steps WITHOUT camera, and of ONE env's every step; a rendered step of 2 .. 64
    # envs takes the split like any batch)
    assert where == {'early window': '1', 'late window': "1'", 'macro': '2', 'macro without camera': '3b', '16 envs without camera': '4',
                     'gym facade': '4', '16 envs with camera': '1'}
    assert plans['gym facade'][1]['single_solve'] == CHAIN_N1 and plans['16 envs without camera'][1]['single_solve'] == WAVE_PER_ENV
    p = plans['early window'][1]
    assert p['coop_h'] and p['coop_vh_beside'] and p['heavy_render'] == WALKER and p['vh_render_on_aux'] and p['la_on_vh']
    p = plans['late window'][1]
    assert not p['coop_h'] and p['coop_vh_beside'] and p['heavy_render'] == RASTER_LIST and p['vh_render_on_main'] and not p['vh_render_on_aux']
    p = plans['macro'][1]
    assert p['heavy_render'] == GRID and not p['coop_h'] and not p['coop_vh_beside'] and not p['vh_render_on_main'] and not p['vh_render_on_aux']
    p = plans['macro without camera'][1]
    assert p['coop_vh_alone']                               # (a wave each for the 368 very heavy envs: the point of 3b)


def _forced(env_vars, N, ntiles, reading, **kw):
    """The PlanIn of a handle created under `env_vars` (the knobs read_settings() reads) whose counters hold `reading`."""
    h, vh = (int(x) for x in env_vars['RR_FORCE_HCOUNT'].split(',')) if 'RR_FORCE_HCOUNT' in env_vars else reading
    return row(N, ntiles, h, vh, split_heavy=int('RR_NO_SPLIT' not in env_vars), lookahead=int('RR_NO_LOOKAHEAD' not in env_vars),
               split_max_pct=int(env_vars.get('RR_SPLIT_MAX_PCT', 60)), **kw)


def test_the_forced_gpu_configurations_take_the_placements_their_labels_name(plan_program):
    """tests/test_gpu_round4.py forces placements through the library's knobs and proves them harmless; here: that each knob
    setting, at that test's batch size and tile count, IS the placement its label names (rendered steps; an entry that pins no
    reading is looked up with what such a batch holds: a handful of heavy envs)."""
    from tests import test_gpu_round4 as gpu4
    N, nt = 448, 4                                          # 128 x 128: four tiles
    for label, env_vars in gpu4.PLACEMENTS:
        names = re.match(r"([\d'b]+)(?: <-> ([\d'b]+))?", label).groups()
        readings = [(5, 1)] if names[1] is None else [(5, 1), (40, 1)]       # ('1 <-> 3': below and above RR_SPLIT_MAX_PCT = 2 % of 448)
        for want, reading in zip(names, readings):
            for mode in (1, 2):
                r = _forced(env_vars, N, nt, reading, render_mode=mode)
                p = dict(zip(OUT_FIELDS, plan_program([r])[0]))
                got = placement(r, list(p.values()))
                if 'long heavy list' in label:
                    assert got == "1'" and not p['coop_h'] and p['heavy_render'] != WALKER and p['vh_render_on_main'], (label, p)
                else:
                    assert got == want, (label, reading, got)
                if 'empty lists' in label or 'early window' in label:
                    assert p['coop_h'] and p['coop_vh_beside'] and p['heavy_render'] == WALKER, (label, p)
                if 'many very heavy' in label:
                    assert not p['coop_h'] and not p['coop_vh_beside'], (label, p)
    # no reading reaches k_raster_list + k_shade at this size: a list too long for the walker (h > 192) is more than a third of 448
    every = plan_program([row(N, nt, h, 0) for h in range(N + 1)])
    assert RASTER_LIST not in every[:, OUT_FIELDS.index('heavy_render')]
    # ... which test_raster_list_render_of_a_heavy_list_is_bitwise_the_inline_step forces at the smallest batch that has it
    r = _forced(gpu4.RASTER_LIST_FORM, 640, nt, None)
    p = dict(zip(OUT_FIELDS, plan_program([r])[0]))
    assert placement(r, list(p.values())) == "1'" and p['heavy_render'] == RASTER_LIST and p['coop_h'], p
    # placement 3b (test_steps_without_camera_side_by_side_...): 1100 envs at 32 x 32 (one tile), steps without camera
    for reading, vh_wave_each in (('400,100', 1), ('30,600', 0)):
        r = _forced({'RR_FORCE_HCOUNT': reading}, 1100, 1, None, render_mode=0)
        p = dict(zip(OUT_FIELDS, plan_program([r])[0]))
        assert placement(r, list(p.values())) == '3b' and p['coop_vh_alone'] == vh_wave_each, (reading, p)
