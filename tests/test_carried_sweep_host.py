"""Tests of the C boundary of the swept clearance with carried objects (rr_carried_sweep, include/realrobot.h) that need no GPU: the
header, the binding, the refusal that needs no handle, the place and shape of the host function and of the kernel template on the
source, the scratch gate, the method's signature.  The GPU side is tests/test_gpu_carried_sweep.py, the restatement's own tests
tests/test_numpy_carried_sweep.py."""
import ctypes as C
import inspect
import os
import re

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests.test_carry_host import _blocks, _code, carry_only_violations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_point_and_documents_it():
    h = _read('include', 'realrobot.h')
    assert int(re.search(r'#define\s+RR_ABI_VERSION\s+(\d+)', h).group(1)) == nat.RR_ABI_VERSION == 7
    assert re.search(r'\bRR_SW_COUNT\s*=\s*4\b', h)                                      # the same four buffers: no new family
    assert re.search(r'\bint\s+rr_carried_sweep\s*\(\s*rr_env\s*\*\s*env\s*,\s*const\s+float\s*\*\s*segments\s*(/\*.*?\*/)?\s*,\s*int32_t\s+n_segments\s*,'
                     r'\s*int32_t\s+on_device\s*,\s*float\s+safety\s*,\s*float\s+tolerance\s*\)\s*;', h)
    assert h.index('int rr_get_attachments(') < h.index('int rr_carried_sweep(')
    doc = h[h.index('Swept clearance with carried objects'):h.index('int rr_carried_sweep(')]
    doc = re.sub(r'\s*\n \*\s*', ' ', doc)                     # (the comment's line breaks are not part of its words)
    for word in ('k_swept_clearance<true>', 'rr_swept_clearance', 'STREAM CONTRACT', 'rr_sweep_buffer', 'NO new buffer family', 'forwards', 'the same bytes', 'motion model',
                 'R_o = R_b R_rel', 'p_o = p_b + R_b t_rel', 'ancestors-or-self', 'chain[k][b]', 'rounded UP', 'all or nothing', 'rho = |t_rel + R_rel c_s|', 'MEASURED',
                 '1 + 2^-18', '1 + 2^-20', 'B_j = 0', 'exclusive-or', 'Guarantees', 'bit for bit', 'rr_posture_clearance', 'never attached', 'No atomics', 'clamped',
                 'RR_SW_MAX_STEPS', 'status in {0, 1, 3}', 'writes the four RR_SW_* buffers only', 'Errors', 'RR_EINVAL', 'RR_EDEVICE', 'Out of scope', 'keeps refusing',
                 'vector env', 'rr_posture_kinematics'):
        assert word in doc, word
    carry = h[h.index('Carried objects in the posture queries'):h.index('int rr_set_attachments(')]
    assert 'rr_carried_sweep' in carry


def test_binding_lists_and_loads_the_symbol():
    L = nat.load_library()
    assert 'rr_carried_sweep' in nat.SYMBOLS
    assert len(L.rr_carried_sweep.argtypes) == 6 and L.rr_carried_sweep.restype is C.c_int32
    assert L.rr_carried_sweep.argtypes == L.rr_swept_clearance.argtypes
    assert L.rr_carried_sweep(None, None, 1, 0, 0.0, 1e-3) == -1 and 'rr_carried_sweep: null env' in L.rr_last_error().decode()
    assert 'sweep' in nat.QUERY_FAMILIES and len(nat.QUERY_FAMILIES) == 10                # no new family
    sig = inspect.signature(BatchedREALRobotEnv.carried_sweep)
    assert list(sig.parameters)[1:] == ['segments', 'safety', 'tolerance', 'host']
    assert [sig.parameters[k].default for k in ('safety', 'tolerance', 'host')] == [0.0, 1e-3, False]
    assert sig.parameters == inspect.signature(BatchedREALRobotEnv.swept_clearance).parameters
    # the columns are cut in one place
    src = inspect.getsource(BatchedREALRobotEnv)
    assert src.count('pair_free_until=') == 1 and src.count('self._sweep_columns(') == 2
    assert 'carried_sweep' in BatchedREALRobotEnv.swept_clearance.__doc__ and 'carried_sweep' in BatchedREALRobotEnv.attach_objects.__doc__


def test_the_host_function_forwards_or_launches_once():
    v = _read('real_robots_amd', 'csrc', 'realrobot.hip')
    # the sweep's part holds the kernel template and what its CARRY instantiation names; rr_carry.inc's staging function is declared in front of it
    assert v.index('#include "rr_carry.inc"') < v.index('#include "rr_posture.inc"') < v.index('#include "rr_sweep.inc"') < v.index('#include "rr_host.inc"')
    assert 'rr_csweep' not in v and not os.path.exists(os.path.join(ROOT, 'real_robots_amd', 'csrc', 'rr_csweep.inc'))
    src = _read('real_robots_amd', 'csrc', 'rr_host.inc')
    assert src.index('int rr_sweep_reach(') < src.index('int rr_get_attachments(') < src.index('int rr_carried_sweep(')
    assert src.count('k_swept_clearance<true>,') == 1 and src.count('k_swept_clearance<false>,') == 1 and 'k_carried_sweep' not in src
    body = src[src.index('int rr_carried_sweep('):]
    body = body[:body.index('\n}\n')]
    assert body.count('hipLaunchKernelGGL(') == 1 and body.count('hipLaunchKernelGGL(k_swept_clearance<true>,') == 1
    assert body.count('e->att_on') == 1 and re.search(r'if \(!e->att_on\) return rr_swept_clearance\(e, segments, n_segments, on_device, safety, tolerance\);', body)
    forward, first_effect = body.index('if (!e->att_on)'), min(body.index(w) for w in ('ensure_query(', 'ensure_sweep_chain(', 'hipLaunchKernelGGL', 'st.in('))
    assert body.index('null env') < body.index('sweep_arguments(e, "rr_carried_sweep"') < forward < first_effect
    assert 'e->att_table' in body and 'e->sw_chain_dev' in body and 'e->sw_reach_dev' in body and 'la_valid' not in body and 'D.state' not in body
    # the reach table both instantiations read keeps its size; the chain table is the memory owner's
    sweep = _read('real_robots_amd', 'csrc', 'rr_sweep.inc')
    assert 'struct SweepReach { float r[NB][MAXSHAPES]; };' in sweep
    chain = src[src.index('static int ensure_sweep_chain('):src.index('int rr_carried_sweep(')]
    assert 'ensure_group(' in chain and 'mem_part(&e->sw_chain_dev' in chain and 'nextafterf' in chain and 'hipMalloc' not in chain
    # both entry points refuse through the one list, each under its own name
    assert src.count('static int sweep_arguments(') == 1 and src.count('sweep_arguments(e, "rr_swept_clearance"') == 1


def test_the_kernel_is_a_part_of_its_own_in_the_scratch_gate():
    """The carried sweep is the CARRY instantiation of the one kernel template in rr_sweep.inc (its name is kept from the time the
    kernel was a part of its own)."""
    k = _read('real_robots_amd', 'csrc', 'rr_sweep.inc')
    code = _code(k)
    assert code.count('__global__') == 1 and re.search(r'template <bool CARRY>\s*__global__ void __launch_bounds__\(SWEEP_THREADS\) k_swept_clearance\(', code)
    assert 'atomic' not in code.lower()
    assert code.count('dist_pair(') == 1 and code.count('carry_stage_object(') == 1
    # staging and the pair search are called, not written out for the carried objects: the one quat_to_m3 is the plain instantiation's staging
    plain = _blocks(code, 'if (!CARRY && tid >= 1 && tid < 1 + NOBJ)')
    assert code.count('quat_to_m3') == 1 and any(a < code.index('quat_to_m3') < b for a, b in plain) and 'gjk' not in code.lower()
    assert code.count('sw_joint_mask(') == 4                                             # its definition, the kernel's two, and the carrying body's
    assert 'SWEEP_THREADS' in code and 'RR_SW_MAX_STEPS + 1' in code and '#define CS_INFLATE (1.0f + 0x1p-18f)' in code
    assert 'min(max(__float_as_int(ar[ATT_BODY]), 0), NB)' in code
    assert code.index('sw_joint_mask(const int') < code.index('int cs_carried(') < code.index('template <bool CARRY>')
    gate = _read('tools', 'check_scratch.py')
    assert "'k_swept_clearance'" in gate and "'k_carried_sweep'" not in gate              # (the gate matches by substring: both instantiations)
    # the plain instantiation knows nothing of it: every word of the table, the chain and the cs_ functions in the kernel is under if constexpr (CARRY)
    assert carry_only_violations(k) == []
    assert '__shared__ float s_att[CARRY ? NOBJ * ATT_ROW : 1];' in code
