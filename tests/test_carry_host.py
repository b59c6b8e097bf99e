"""Tests of the C boundary of the carried objects (rr_set_attachments, include/realrobot.h) that need no GPU: the header, the binding,
the refusals that need no handle, the dispatch of the three posture queries and the sweep's refusal on the source, the shape of the
four kernel templates (`carry_only_violations`), the Python-side argument checks and `carry_pairs`.  The GPU side is tests/test_gpu_carry.py, the reference's own tests tests/test_numpy_carry.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rr_set_attachments', 'rr_get_attachments')
TEMPLATES = {'rr_posture.inc': 'k_posture_clearance', 'rr_signed.inc': 'k_signed_distance', 'rr_grad.inc': 'k_signed_gradient', 'rr_sweep.inc': 'k_swept_clearance'}
TABLE_KERNELS = ('k_attach_set', 'k_attach_capture')
CARRY_NAME = re.compile(r'\b(att|s_att|chain|cs_\w+|carry_stage_object)\b')


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _body(src, start, end):
    return src[src.index(start):src.index(end)]


def _code(text):
    """the text without its comments, line for line and column for column"""
    text = re.sub(r'/\*.*?\*/', lambda m: re.sub(r'[^\n]', ' ', m.group(0)), text, flags=re.S)
    return '\n'.join(l.split('//')[0] for l in text.splitlines())


def _blocks(code, opener):
    """the (start, end) spans of the brace blocks that `opener` opens, by counting braces"""
    spans = []
    for m in re.finditer(re.escape(opener) + r'\s*\{', code):
        depth, i = 1, m.end()
        while depth:
            depth += {'{': 1, '}': -1}.get(code[i], 0)
            i += 1
        spans.append((m.start(), i))
    return spans


def carry_only_violations(text):
    """What a kernel template <bool CARRY> says of carried objects outside the places for it.  The kernel is the one __global__ of the
    part, from `template <bool CARRY>` to the end.  Every code line of it that names att, s_att, chain, cs_* or carry_stage_object has
    to be the kernel's parameter list or lie inside an `if constexpr (CARRY) {...}` block; the one other form is the LDS array that
    only such blocks name, declared at function scope because they share it and sized by CARRY (`__shared__ T s_att[CARRY ? n : 1];`:
    an array no statement of the plain instantiation names takes no LDS there, which the kernel descriptors compared by
    tools/compare_kernel_asm.py show).  Returns the offending lines."""
    code = _code(text)
    assert code.count('__global__') == 1 and code.count('template <bool CARRY>') == 1
    start = code.index('template <bool CARRY>')
    assert start < code.index('__global__')
    params = (code.index(')', code.index('__launch_bounds__(', start)) + 1, code.index(') {', start) + 1)      # behind the launch bounds, up to the body's brace
    inside = _blocks(code, 'if constexpr (CARRY)') + [params]
    bad = []
    for m in CARRY_NAME.finditer(code, start):
        line = code[code.rfind('\n', 0, m.start()) + 1:code.find('\n', m.start())]
        if any(a <= m.start() < b for a, b in inside) or re.fullmatch(r'\s*__shared__ (int|float) s_att\[CARRY \? [\w *]+ : 1\];\s*', line):
            continue
        bad.append(line.strip())
    return bad


def test_header_declares_the_entry_points_and_keeps_the_abi_numbers():
    h = _read('include', 'realrobot.h')
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert re.search(r'#define\s+RR_NUM_KERNELS\s+9\b', h) and re.search(r'\bRR_F_COUNT\s*=\s*16\b', h)
    assert re.search(r'\bint\s+rr_set_attachments\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+int32_t\s*\*\s*link\s*(/\*.*?\*/)?\s*,\s*const\s+float\s*\*\s*rel_pose\s*(/\*.*?\*/)?\s*,'
                     r'\s*const\s+uint8_t\s*\*\s*env_mask\s*(/\*.*?\*/)?\s*\)\s*;', h, re.S)
    assert re.search(r'\bint\s+rr_get_attachments\s*\(\s*rr_env\s*\*\s*env\s*,\s*int32_t\s*\*\s*link_out\s*(/\*.*?\*/)?\s*,\s*float\s*\*\s*rel_pose_out\s*(/\*.*?\*/)?\s*\)\s*;', h)
    doc = h[h.index('Carried objects in the posture queries'):h.index('int rr_get_attachments(')]
    doc = re.sub(r'\s*\n \*\s*', ' ', doc)                     # (the comment's line breaks are not part of its words)
    for word in ('ATTACHED body', 'QUERY-SIDE SETTING', 'createConstraint', 'no step reads it', 'link[e][o] in [0, 17)', '-1: FREE', 'COM frame', 'RR_KIN_LINK_POSE',
                 'link_pose^-1 o object pose', 'R_o = R_b R_rel', 'p_o = p_b + R_b t_rel', 'RR_SG_PAIR_GRADIENT', 'the bits it has with the feature off', '16 + o',
                 'rr_closest_points is unaffected', 'rr_swept_clearance REFUSES', 'WHOLE', 'CAPTURE', 'T_link(q_present)^-1 o T_object(present)', 'turns the feature OFF',
                 'normalised on the host in float64', 'PERSISTENT', 'rr_reset', 'auto-reset', 'rr_write_state', 'rr_set_distance_pairs', 'DESTINATION env',
                 'checkpoints and snapshots do not carry it', 'NOTHING changed', 'rigid with the world', 'non-finite', 'norm zero', 'RR_EINVAL', 'all or nothing',
                 'N x 192 bytes', 'Out of scope'):
        assert word in doc, word
    v = _read('real_robots_amd', 'csrc', 'realrobot.hip')
    # what the kernel templates name is declared in front of them
    order = [v.index('#include "%s"' % f) for f in ('rr_dist.inc', 'rr_carry.inc', 'rr_posture.inc', 'rr_sweep.inc', 'rr_signed.inc', 'rr_grad.inc', 'rr_host.inc')]
    assert order == sorted(order)


def test_binding_lists_and_loads_the_symbols():
    L = nat.load_library()
    assert L.rr_abi_version() == 7
    for name in NEW:
        assert name in nat.SYMBOLS, name
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int32, name
    assert len(L.rr_set_attachments.argtypes) == 4 and len(L.rr_get_attachments.argtypes) == 3
    # the refusals that need no device: a null env -- RR_EINVAL with the entry point's name
    assert L.rr_set_attachments(None, None, None, None) == -1 and 'rr_set_attachments: null env' in L.rr_last_error().decode()
    assert L.rr_get_attachments(None, None, None) == -1 and 'rr_get_attachments: null env' in L.rr_last_error().decode()
    for name in ('attach_objects', 'detach_objects', 'attachments', 'carry_pairs', '_attach_args'):
        assert callable(getattr(BatchedREALRobotEnv, name))
    assert list(inspect.signature(BatchedREALRobotEnv.attach_objects).parameters)[1:] == ['links', 'rel_pose', 'env_mask']
    assert list(inspect.signature(BatchedREALRobotEnv.detach_objects).parameters)[1:] == ['env_mask']


def test_the_queries_dispatch_once_and_the_sweep_refuses():
    src = _read('real_robots_amd', 'csrc', 'rr_host.inc')
    ends = {'rr_posture_clearance': 'int rr_posture_buffer(', 'rr_signed_distance': 'int rr_signed_buffer(', 'rr_signed_gradient': 'int rr_signed_gradient_buffer('}
    for fn, kern in (('rr_posture_clearance', 'k_posture_clearance'), ('rr_signed_distance', 'k_signed_distance'), ('rr_signed_gradient', 'k_signed_gradient')):
        # one reading of the flag, in front of exactly two launches of the one kernel name, <true> first; the table once, in the <true> launch
        body = _body(src, 'int %s(' % fn, ends[fn])
        assert body.count('e->att_on') == 1 and body.count('hipLaunchKernelGGL(') == 2 == body.count('hipLaunchKernelGGL(%s<' % kern), fn
        at = body.index('if (e->att_on)')
        carry, plain = body.index('hipLaunchKernelGGL(%s<true>,' % kern), body.index('hipLaunchKernelGGL(%s<false>,' % kern)
        other = body.index('else', carry)
        assert at < carry < other < plain and body.count('e->att_table') == 1 and carry < body.index('e->att_table') < other, fn
        assert body[plain:body.index(';', plain)].rstrip().endswith('(const float *)nullptr)'), fn      # the plain launch: null for the added pointer
        assert body.index('ensure_query(') < at and plain < body.index('hipGetLastError')
    sweep = _body(src, 'int rr_swept_clearance(', 'int rr_sweep_reach(')
    assert sweep.count('e->att_on') == 1 and '_carry,' not in src and '_carry<' not in src
    assert sweep.count('hipLaunchKernelGGL(') == 1 == sweep.count('hipLaunchKernelGGL(k_swept_clearance<false>,') and 'e->att_table' not in sweep
    launch = sweep[sweep.index('hipLaunchKernelGGL('):]
    assert launch[:launch.index(';')].rstrip().endswith('(const float *)nullptr, (const SweepChain *)nullptr)')
    refuse = sweep.index('if (e->att_on)')
    first_effect = min(sweep.index(w) for w in ('ensure_query(', 'hipLaunchKernelGGL', 'st.in('))
    assert refuse < sweep.index('RR_EINVAL', refuse) < sweep.index('rr_set_attachments', refuse) < first_effect
    # rr_closest_points and the step know nothing of the table
    for fn, end in (('rr_closest_points', 'int rr_distance_buffer('), ('rr_step', 'int rr_render(')):
        body = _body(src, 'int %s(' % fn, end)
        assert 'att_' not in body, fn
    for f in ('rr_fork.inc', 'rr_prep.inc', 'rr_solve.inc', 'rr_collide.inc', 'rr_write.inc', 'rr_state.inc'):
        assert 'att' not in re.findall(r'\batt\w*', _read('real_robots_amd', 'csrc', f)), f
    # the four kernel templates: one __global__ each, and all they say of carried objects is the parameter list or under if constexpr (CARRY)
    for f, kern in TEMPLATES.items():
        text = _read('real_robots_amd', 'csrc', f)
        assert carry_only_violations(text) == [], f
        code = _code(text)
        assert re.search(r'template <bool CARRY>\s*__global__ void __launch_bounds__\(\w+\) %s\(' % kern, code), f
        assert len(_blocks(code, 'if constexpr (CARRY)')) >= 1 and '!CARRY' in code, f      # both kinds of statement exist, each under its guard
    # the setter validates before its first allocation, copy, launch or flag: a refusal changes nothing
    body = _body(src, 'int rr_set_attachments(', 'int rr_get_attachments(')
    first_effect = min(body.index(w) for w in ('ensure_attachments(', 'hipMemcpyAsync', 'hipLaunchKernelGGL', 'e->att_on =', 'e->att_link['))
    for msg in ('null env', 'is neither -1 (free) nor in [0, ', 'is rigid with the world', 'the rel pose is not finite', 'quaternion has norm zero'):
        assert body.index(msg) < first_effect, msg
    assert body.index('!link && !e->att_table') < body.index('ensure_attachments(')         # detaching a table that never was: nothing allocated
    assert 'la_valid' not in body and 'scratch' not in body and 'D.state' not in body
    # the carry code: no atomics; the pair functions and the staging are called, once per kernel, never written out a second time
    k = _code(_read('real_robots_amd', 'csrc', 'rr_carry.inc'))
    assert 'atomic' not in k and k.count('__device__ __forceinline__ int carry_stage_object(') == 1 and 'dist_pair(' not in k and 'sd_pair(' not in k
    assert '_carry(' not in k and k.count('__global__') == len(TABLE_KERNELS)
    calls = {f: _code(_read('real_robots_amd', 'csrc', f)) for f in TEMPLATES}
    for f, code in calls.items():
        kernel = code[code.index('template <bool CARRY>'):]
        assert 'atomic' not in kernel.lower() and kernel.count('carry_stage_object(') == 1, f
        assert kernel.count('dist_pair(') == (f in ('rr_posture.inc', 'rr_sweep.inc')) and kernel.count('sd_pair(') == (f in ('rr_signed.inc', 'rr_grad.inc')), f
    gate = _read('tools', 'check_scratch.py')
    for name in TABLE_KERNELS:
        assert name + '(' in k and "'%s'" % name in gate, name
    for name in TEMPLATES.values():                                                      # (the gate matches by substring: both instantiations)
        assert "'%s'" % name in gate and "'%s_carry'" % name not in gate, name


def test_python_side_arguments_need_no_device():
    N, n = 4, 3
    args = BatchedREALRobotEnv._attach_args
    links, rel = args(N, n, {'cube': 'base', 2: 10})
    assert rel is None and links.dtype == np.int32 and links.flags.c_contiguous and links.tolist() == [[8, -1, 10]] * N
    assert args(N, n, {})[0].tolist() == [[-1, -1, -1]] * N
    for t in (8, [8, -1, 4], np.array([[8], [-1], [4], [0]]), np.full((N, n), 16, np.int64)):
        links, _ = args(N, n, np.asarray(t))
        assert links.shape == (N, n) and links.dtype == np.int32
    links, rel = args(N, n, 8, [0, 0, 0.1, 0, 0, 0, 2.0])
    assert rel.shape == (N, n, 7) and rel.dtype == np.float32 and rel.flags.c_contiguous and (rel[..., 6] == 2.0).all()
    assert args(N, 2, {'tomato': 3})[0].shape == (N, 2)
    for bad in ({'mustard': 8}, {2: 8}):                                                 # an object a two-object handle does not have
        with pytest.raises(ValueError):
            args(N, 2, bad)
    for bad in ({'table': 8}, {'cube': 'gripper'}, {'cube': 17}, {'cube': -2}, {'cube': 1.5}, {3: 8}, {True: 8}, np.array([8.0]), np.array([17]), np.array([-2]),
                np.zeros((N + 1, n), np.int32), np.zeros((N, n + 1), np.int32)):
        with pytest.raises(ValueError):
            args(N, n, bad)
    for bad in (np.zeros((N, n, 6)), [np.nan] * 7, [np.inf, 0, 0, 0, 0, 0, 1]):
        with pytest.raises(ValueError):
            args(N, n, 8, bad)


def test_carry_pairs():
    shapes = BatchedREALRobotEnv.collision_shapes()
    name = {r['index']: r['name'] for r in shapes}
    idx = {r['name']: r['index'] for r in shapes}
    pairs = BatchedREALRobotEnv.carry_pairs(['cube'], exclude_links=('finger_01',))
    assert pairs.dtype == np.int32 and pairs.shape[1] == 2 and len(pairs) <= nat.DIST_MAX
    got = [(name[a], name[b]) for a, b in pairs.tolist()]
    robot = [r['name'] for r in shapes if 0 <= r['body'] < 16]
    assert len(robot) == 16
    want = [('cube', s) for s in ('table', 'shelf', 'robot_base')] + [('cube', 'tomato'), ('cube', 'mustard')] + [('cube', r) for r in robot if r != 'finger_01']
    want += [(r, s) for r in robot for s in ('table', 'shelf')] + [(r, o) for r in robot for o in ('tomato', 'mustard')]
    assert got == want and len(got) == 3 + 2 + 15 + 32 + 32
    # the robot's own pairs are pairs of the step's collision table, in its order
    from tests import numpy_collide as ncol
    table = [(a, b) for _, a, b in ncol.pair_table(3)]
    own = [tuple(p) for p in pairs[20:].tolist()]
    assert [p for p in table if p in set(own)] == own
    # an index for a name, two objects, a two-object env, both tips of the task's gripper excluded
    assert (BatchedREALRobotEnv.carry_pairs(0, exclude_links=[10]) == pairs).all()
    two = BatchedREALRobotEnv.carry_pairs(['cube', 'mustard'], exclude_links=('finger_01', 'finger_11'))
    got2 = [(name[a], name[b]) for a, b in two.tolist()]
    assert got2.count(('cube', 'mustard')) == 1 and ('mustard', 'cube') not in got2 and ('cube', 'finger_11') not in got2 and ('mustard', 'finger_01') not in got2
    assert len(two) == 2 * 3 + 3 + 2 * 14 + 32 + 16 and len(set(map(tuple, two.tolist()))) == len(two)
    small = BatchedREALRobotEnv.carry_pairs(['cube'], n_objects=1)
    assert idx['tomato'] not in small and idx['mustard'] not in small and len(small) == 3 + 16 + 32
    for bad in (dict(objects=['table']), dict(objects=[3]), dict(objects=['mustard'], n_objects=2), dict(objects=['cube'], exclude_links=['hand']),
                dict(objects=['cube'], exclude_links=[-1])):
        with pytest.raises(ValueError):
            BatchedREALRobotEnv.carry_pairs(**bad)
