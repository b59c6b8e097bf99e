"""GPU tests (-m gpu) of the posture queries with carried objects (rr_set_attachments, include/realrobot.h): the three queries against
the float64 reference that moves the carried objects with their links (tests/numpy_carry.py), the capture, that a carried object
moves, bit identity of everything that is not carried against a twin handle that never attached, the gradient's masks, formula and
central differences, determinism and independence, no effect on the simulation, the life cycle of the table and the refusals.

Tolerances, the project's convention.  On the items that have a shape of an attached object the ceilings are four times the largest
|device - float64| the MI355X showed on the decided items of the fixture (the margin the sibling files give for the input sensitivity
of float32 GJK / EPA); the reference composes the rel poses READ BACK by attachments(), so both sides compose the device's own
float32 rel:
  MEASURED_D    m      signed distance and clearance (posture_clearance, signed_distance, signed_distance_gradient and the per-row records)
  MEASURED_G    m/rad  pair gradients against the float64 formula on the device's own record with the carried masks
  MEASURED_CAP  m, rad captured rel poses against float64 T_link^-1 o T_object of the same state
Conditions that are not measurements: a distance ceiling above 2e-6 m (about eight float32 roundings at 2 m; a wrong frame is wrong by
millimetres), a gradient ceiling above 1e-5 m/rad or a capture ceiling above 1e-6 m / 1e-6 rad is a finding, not a tolerance --
asserted below.  Items without an attached shape keep the siblings' ceilings, imported, and on them the bytes of the twin.  The
gradients are also held to the committed central differences (tests/golden/carry_gradient.npz) with its tol_g, four times the float64
formula's own disagreement with them."""
import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from tests import numpy_carry as nc
from tests import numpy_distance as nd
from tests import numpy_penetration as pen
from tests import numpy_posture as npo
from tests import numpy_signed_gradient as nsg
from tests.test_gpu_distance import TOL as TOL_DIST
from tests.test_gpu_posture_query import TOL as TOL_PC
from tests.test_gpu_signed_distance import TOL_SD
from tests.test_gpu_signed_gradient import TOL_F

pytestmark = pytest.mark.gpu

U = np.uint32
MEASURED_D = 1.42e-7          # m: the largest |device - float64| over the decided items with an attached shape on the MI355X (1.26e-7 over the fixture's 54
                              # items in each of the three queries and in the per-row records, 1.42e-7 over the 122 of the collision table at N = 2, K = 2)
MEASURED_G = 1.27e-7          # m/rad: the largest |pair gradient - float64 formula on the device's record| over the fixture's 54 attached items on the MI355X
MEASURED_CAP = 5.51e-8        # m and rad: captured rel poses against float64 on the MI355X (position 5.46e-8 m, rotation 5.51e-8 rad)
CEIL_D, CEIL_G, CEIL_CAP = 4 * MEASURED_D, 4 * MEASURED_G, 4 * MEASURED_CAP
MARGIN = np.float32(nsg.MARGIN)
PER_PAIR = ('pair_distance', 'pair_status', 'pair_iterations', 'pair_expansions')
PER_PAIR_PRESENT = PER_PAIR + ('pair_bound', 'pair_point_a', 'pair_point_b', 'pair_normal', 'pair_gradient')


def test_the_ceilings_are_tolerances_not_findings():
    assert CEIL_D <= 2e-6 and CEIL_G <= 1e-5 and CEIL_CAP <= 1e-6


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _copy(cols):
    return {k: np.array(v) for k, v in cols.items()}


def _flat(out):
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in out.items()}


def _same(x, y, keys=None, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    return all((_bits(pick(x[k])) == _bits(pick(y[k]))).all() for k in (keys or x))


def _report(where, fig, fails):
    print(where, {k: (float('%.3g' % v) if isinstance(v, float) else v) for k, v in fig.items()}, fails)


def _env(N, nobj=3):
    return BatchedREALRobotEnv(N, objects=nobj, width=64, height=64)


def _attach_fixture(env, sel=slice(None)):
    """the fixture's attachments on a handle of the envs `sel`: the captured ones from the present state, then env 4's given pose"""
    _, _, links, given = nc.inputs()
    links, given, cap = links[sel], given[sel], nc.CAPTURED[sel]
    env.attach_objects(links, env_mask=cap)
    if (cap == 0).any():
        env.attach_objects(links, given, env_mask=1 - cap)


def _queries(env, st, po, pairs):
    """the calls both handles of the fixture get: the three queries at the K postures, the gradient query at the present state, at the
    envs' own joints as a K = 1 posture, and per row with the row's posture written into the joints"""
    out = {}
    env.set_distance_pairs(pairs)
    out['pc'] = _copy(env.posture_clearance(po, host=True))
    out['sd'] = _copy(env.signed_distance(po, host=True))
    out['sg'] = _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True))
    out['present'] = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    out['own'] = _copy(env.signed_distance(np.ascontiguousarray(st[:, None, :11]), host=True))
    per = []
    for k in range(po.shape[1]):
        env.write_state(np.ascontiguousarray(npo.rows(st, po).reshape(len(st), po.shape[1], 61)[:, k]), joint_pos=True)
        per.append(_copy(env.signed_distance_gradient(margin=MARGIN, host=True)))
    env.write_state(st, joint_pos=True)
    out['per'] = {key: np.stack([p[key] for p in per], 1) for key in per[0]}                      # [N, K, ...]
    return out


_dev = {}


def _fixture():
    """(inputs, the carrying handle's results, the twin's, links and rel poses read back, the reference on the read-back poses): the
    device and the reference are asked once per process."""
    st, po, links, given = nc.inputs()
    if 'fix' not in _dev:
        a, t = _env(nc.N), _env(nc.N)
        a.state = st
        t.state = st
        _attach_fixture(a)
        got_links, rel = a.attachments()
        carry, twin = _queries(a, st, po, nc.seven_pairs()), _queries(t, st, po, nc.seven_pairs())
        a.close()
        t.close()
        _dev['fix'] = (carry, twin, got_links, rel, nc.reference(rel=rel.astype(np.float64)))
    return (st, po, links, given) + _dev['fix']


def _item_cols(out):
    """the per-pair records [R, Q, ...] under the names numpy_distance.compare / numpy_penetration.compare read"""
    return dict(distance=out['pair_distance'], lower=out['pair_bound'], bound=out['pair_bound'], point_a=out['pair_point_a'], point_b=out['pair_point_b'],
                normal=out['pair_normal'], status=out['pair_status'], expansions=out['pair_expansions'])


def test_against_float64():
    st, po, links, _, carry, _, got_links, rel, ref = _fixture()
    pairs = nc.seven_pairs()
    assert (got_links == links).all()
    att = nc.attached_items(links, pairs, nc.K)
    dec = ref['decided']
    fails = []
    # every pair's full record, from the per-row present-state queries: attached items with this file's ceiling, the others with the siblings'
    cols = _item_cols(_flat(carry['per']))
    for where, sel, tol_d, tol_sd in (('attached', att, CEIL_D, CEIL_D), ('others', ~att, TOL_DIST, TOL_SD)):
        sub = dict(ref, decided=dec & sel)
        fig, bad = pen.compare(cols, sub, pairs, tol_sd)
        _report('records, %s, overlapping' % where, fig, bad)
        fig2, bad2 = nd.compare(cols, dict(sub, decided=sub['decided'] & (ref['expect'] != 1)), tol_d, pairs)
        _report('records, %s, apart' % where, fig2, bad2)
        fails += ['%s: %s' % (where, b) for b in bad + bad2]
        if where == 'attached':
            assert fig['overlapping'] >= 10 and fig2['separated'] >= 10
    # the three queries' per-pair distances and statuses at the K postures
    sep, ov = dec & (ref['expect'] == 0), dec & (ref['expect'] == 1)
    for name in ('pc', 'sd', 'sg'):
        f = _flat(carry[name])
        d, s = f['pair_distance'].astype(np.float64), f['pair_status']
        want = np.maximum(ref['d'], 0.0) if name == 'pc' else ref['d']
        m = (sep | ov) if name != 'pc' else dec
        e_att, e_oth = np.abs(d - want)[m & att].max(), np.abs(d - want)[m & ~att].max()
        wrong = int((s[dec] != ref['expect'][dec]).sum())
        print('%s: |device - float64| on %d attached decided items %.3g (ceiling %.3g), on %d others %.3g; status mismatches %d'
              % (name, (m & att).sum(), e_att, CEIL_D, (m & ~att).sum(), e_oth, wrong))
        if not e_att <= CEIL_D:
            fails.append('%s: attached distance error %.3g > %.3g' % (name, e_att, CEIL_D))
        if not e_oth <= max(TOL_PC, TOL_SD, TOL_DIST):
            fails.append('%s: distance error of the others %.3g' % (name, e_oth))
        if wrong:
            fails.append('%s: %d status mismatches' % (name, wrong))
    # the reductions: the nearest pair of posture_clearance where the reference decides it, the deepest of the signed queries where it
    # is deepest by a millimetre; at least one such row per attachment pattern (tests/test_numpy_carry.py)
    jstar, rowdec = npo.nearest(ref)
    assert (rowdec.reshape(5, 3).sum(1) >= 1).all() and (_flat(carry['pc'])['pair'][rowdec] == jstar[rowdec]).all()
    fig, bad = npo.compare_nearest(_flat(carry['pc']), ref, max(CEIL_D, TOL_PC), pairs, jstar, rowdec)
    _report('nearest records', fig, bad)
    fails += bad
    srt = np.sort(ref['d'], 1)
    deep = srt[:, 1] - srt[:, 0] >= nd.DECIDE
    for name in ('sd', 'sg'):
        f = _flat(carry[name])
        assert (f['pair'][deep] == ref['d'].argmin(1)[deep]).all(), name
        assert (f['pair'] == npo.first_minimum(f['pair_distance'])).all() and (_bits(f['distance']) == _bits(f['pair_distance'][np.arange(15), f['pair']])).all()
    # reported ids: an object is 16 + o, attached or not
    f = _flat(carry['sd'])
    rows = (f['pair'] == 6)
    assert rows.any() and (f['body_a'][rows] == 18).all() and (f['body_b'][rows] == 16).all()
    assert not fails, fails


def test_capture():
    st, po, links, given, carry, twin, _, rel, _ = _fixture()
    want = nc.reference_rel()
    worst_p = worst_q = 0.0
    for e, o in zip(*np.nonzero(links >= 0)):
        q = rel[e, o, 3:].astype(np.float64)
        assert abs(np.linalg.norm(q) - 1.0) <= 4 * 2.0 ** -23
        ang = 2 * np.arcsin(min(1.0, np.linalg.norm(q * np.sign(q @ want[e, o, 3:]) - want[e, o, 3:])) / 2)
        worst_p, worst_q = max(worst_p, np.abs(rel[e, o, :3] - want[e, o, :3]).max()), max(worst_q, ang)
    print('rel poses read back against float64: position %.3g m, rotation %.3g rad (ceiling %.3g)' % (worst_p, worst_q, CEIL_CAP))
    free = links < 0
    assert (rel[free] == np.array([0, 0, 0, 0, 0, 0, 1], np.float32)).all()
    # a K = 1 query at the envs' own joints puts the captured objects back where the state has them
    cap = nc.CAPTURED.astype(bool)
    d = np.abs(carry['own']['pair_distance'][:, 0].astype(np.float64) - twin['present']['pair_distance'])[cap]
    print('K = 1 at the present joints against the feature-off present-state query: %.3g m' % d.max())
    assert (carry['own']['pair_status'][:, 0][cap] == twin['present']['pair_status'][cap]).all()
    assert worst_p <= CEIL_CAP and worst_q <= CEIL_CAP and d.max() <= CEIL_D


def test_it_moves():
    """(cube, table) of env 1 at a posture 0.35 rad away in joint 1: more than a centimetre from the answer with the cube left behind,
    and the reference's answer."""
    st, _, links, _, _, _, _, rel, _ = _fixture()
    mv, pairs = nc.moved_posture(), nc.two_pairs()
    assert abs(mv[1, 0, 1] - st[1, 1]) >= 0.3
    env = _env(nc.N)
    env.state = st
    env.set_distance_pairs(pairs)
    off = _copy(env.signed_distance(mv, host=True))
    _attach_fixture(env)
    assert (env.attachments()[1] == rel).all()                                               # (the capture is deterministic)
    on = _copy(env.signed_distance(mv, host=True))
    pc = _copy(env.posture_clearance(mv, host=True))
    env.close()
    ref_on = nc.reference(rel=rel.astype(np.float64), pairs=pairs, postures=mv)
    ref_off = nd.reference(npo.rows(st, mv), pairs)
    a, b = float(on['pair_distance'][1, 0, 0]), float(off['pair_distance'][1, 0, 0])
    print('(cube, table) of env 1: carried %.6f (float64 %.6f), left behind %.6f (float64 %.6f)' % (a, ref_on['d'][1, 0], b, ref_off['d'][1, 0]))
    assert abs(a - b) > 0.01 and ref_on['decided'][1, 0] and ref_off['decided'][1, 0]
    assert abs(a - ref_on['d'][1, 0]) <= CEIL_D and abs(b - ref_off['d'][1, 0]) <= TOL_DIST and abs(pc['pair_distance'][1, 0, 0] - max(ref_on['d'][1, 0], 0.0)) <= CEIL_D
    assert abs((a - b) - (ref_on['d'][1, 0] - ref_off['d'][1, 0])) <= CEIL_D + TOL_DIST
    # two pairs: waves 2 and 3 of a workgroup have none; env 0 and env 4's (cube, table) are the feature-off bytes
    assert (_bits(on['pair_distance'][0]) == _bits(off['pair_distance'][0])).all() and (_bits(on['pair_distance'][4, :, 0]) == _bits(off['pair_distance'][4, :, 0])).all()
    dec = ref_on['decided']
    assert np.abs(on['pair_distance'][:, 0].astype(np.float64) - ref_on['d'])[dec].max() <= CEIL_D and (on['pair_status'][:, 0][dec] == ref_on['expect'][dec]).all()


def test_what_is_not_carried_keeps_its_bits():
    st, po, links, _, carry, twin, _, _, _ = _fixture()
    pairs = nc.seven_pairs()
    att = nc.attached_items(links, pairs, nc.K).reshape(5, 3, 7)
    assert not att[0].any() and att[1:].any(2).all()
    for name in ('pc', 'sd', 'sg', 'present', 'own', 'per'):
        assert set(carry[name]) == set(twin[name])
        assert _same(carry[name], twin[name], sel=0), name                                   # env 0: every column of every buffer
    free = ~att
    for name in ('pc', 'sd', 'sg', 'per'):
        keys = [k for k in (PER_PAIR_PRESENT if name == 'per' else PER_PAIR) if k in carry[name]]
        assert len(keys) >= 3
        for k in keys:
            assert (_bits(carry[name][k])[free] == _bits(twin[name][k])[free]).all(), (name, k)
    for k in PER_PAIR_PRESENT:
        assert (_bits(carry['present'][k])[free[:, 0]] == _bits(twin['present'][k])[free[:, 0]]).all(), k
    # ... and the carried ones do not: most attached items differ from the twin's by more than a centimetre
    moved = np.abs(carry['sd']['pair_distance'] - twin['sd']['pair_distance'])[att]
    assert (moved > 0.01).sum() >= 30
    # separated pairs: posture_clearance and signed_distance report the same distance, byte for byte
    apart = (carry['pc']['pair_status'] == 0) & (carry['sd']['pair_status'] == 0)
    assert (apart & att).sum() >= 10 and (_bits(carry['pc']['pair_distance'])[apart] == _bits(carry['sd']['pair_distance'])[apart]).all()
    assert _same(carry['sd'], carry['sg'], keys=list(carry['sd']))                           # the gradient call writes the five RR_SD_* buffers as its sibling does


def test_gradient():
    st, po, links, _, carry, twin, _, rel, ref = _fixture()
    pairs = nc.seven_pairs()
    att = nc.attached_items(links, pairs, nc.K)
    mA, mB = nc.masks(links, pairs, nc.K)
    anc = nsg.ns.model()['anc']
    # masks at the present state: (cube, table) of env 1, the cube on link 8 (body 6) -- +0.0 bits outside the ancestors of that body,
    # non-zero wherever the float64 derivative is above the ceiling (joint 0 turns about the vertical, the table's normal: its
    # column is zero by geometry, not by the mask)
    present = carry['present']
    row = present['pair_gradient'][1, 1]
    g64 = nsg.formula(st[1, :11], present['pair_point_a'][1, 1], present['pair_point_b'][1, 1], present['pair_normal'][1, 1], mA[3, 1], mB[3, 1])
    on = anc[6] > 0
    assert on.sum() == 7 and not _bits(row[~on]).any() and (np.abs(g64) > CEIL_G).sum() >= 4 and (row[np.abs(g64) > CEIL_G] != 0).all()
    assert not _bits(twin['present']['pair_gradient'][1, 1]).any()                                           # (a free cube against the table: no columns)
    # the formula on the device's own record, every row and pair: the carried masks in float64
    per = _flat(carry['per'])
    g64 = nsg.formula(po.reshape(15, 1, 11), per['pair_point_a'], per['pair_point_b'], per['pair_normal'], mA, mB)
    live = (per['pair_status'] != 4)[..., None]
    ef = np.abs(per['pair_gradient'] - g64 * live).max(-1)
    print('pair gradients against the float64 formula on the device record: attached %.3g (ceiling %.3g), others %.3g (TOL_F %.3g); largest |g| %.3g'
          % (ef[att].max(), CEIL_G, ef[~att].max(), TOL_F, np.abs(per['pair_gradient'][att]).max()))
    # (cube, its own link): zero within the ceiling in every column, in the envs whose cube link 8 carries
    env = _env(nc.N)
    env.state = st
    _attach_fixture(env)
    env.set_distance_pairs(nc.own_link_pair())
    own = _copy(env.signed_distance_gradient(margin=MARGIN, host=True))
    own_k = _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True))
    env.close()
    print('(cube, its own link): largest |column| %.3g at the present state, %.3g at the postures' % (np.abs(own['pair_gradient'][[1, 3], 0]).max(), np.abs(own_k['gradient'][[1, 3]]).max()))
    print('(cube, its own link): the distance over the K postures differs from the present state\'s by %.3g m' % np.abs(own_k['pair_distance'][[1, 3]] - own['pair_distance'][[1, 3], None]).max())
    assert np.abs(own['pair_gradient'][[1, 3], 0]).max() <= CEIL_G and np.abs(own_k['gradient'][[1, 3]]).max() <= CEIL_G
    assert np.abs(own_k['pair_distance'][[1, 3]] - own['pair_distance'][[1, 3], None]).max() <= CEIL_D       # ... and the distance does not depend on the joints
    assert np.abs(own_k['gradient'][0]).max() > 0.01                                                          # (env 0's free cube: the link moves against it)
    # the central differences of the float64 reference with the carried objects moving
    g = nc.golden()
    cen, fwd, bwd = nsg.derivatives(g['d0'], g['dplus'], g['dminus'])
    ok = att & nsg.compared(np.nan_to_num(g['d0']), np.nan_to_num(fwd), np.nan_to_num(bwd))
    tol = float(g['tol_g'])
    ed = np.abs(per['pair_gradient'] - np.nan_to_num(cen)).max(-1)
    print('pair gradients against the central differences on %d compared items (%d overlapping): %.3g (tol_g %.3g)' % (ok.sum(), (ok & (g['d0'] < 0)).sum(), ed[ok].max(), tol))
    # the deepest pair's gradient of the posture query is that pair's row, and the cost sums are float64 sums of the device's own terms
    sg = _flat(carry['sg'])
    assert (_bits(sg['gradient']) == _bits(per['pair_gradient'][np.arange(15), sg['pair']])).all()
    d, gg = per['pair_distance'].astype(np.float64), per['pair_gradient'].astype(np.float64)
    c = np.maximum(np.float64(MARGIN) - d, 0.0)
    tol_sum = lambda terms, axis: (terms.shape[axis] + 4) * 2.0 ** -24 * np.abs(terms).sum(axis) + 1e-30
    eC, eG = np.abs(sg['cost'] - nsg.cost(d, np.float64(MARGIN))), np.abs(sg['cost_gradient'] - nsg.cost_gradient(d, gg, np.float64(MARGIN)))
    print('cost error / bound %.3g, cost gradient error / bound %.3g, largest cost %.3g' % ((eC / tol_sum(0.5 * c * c, -1)).max(), (eG / tol_sum(c[..., None] * gg, -2)).max(), sg['cost'].max()))
    assert (c[att] > 0).sum() >= 10 and sg['cost'].max() > 1e-4
    assert (eC <= tol_sum(0.5 * c * c, -1)).all() and (eG <= tol_sum(c[..., None] * gg, -2)).all()
    assert _same(_flat(carry['sg']), per, keys=('gradient', 'cost', 'cost_gradient'))                         # the posture form carries the per-row form's bits
    assert ef[att].max() <= CEIL_G and ef[~att].max() <= TOL_F and np.abs(per['pair_gradient'][att]).max() > 0.3
    assert ok.sum() >= 40 and ed[ok].max() <= tol


def test_determinism_and_independence():
    st, po, links, given, carry, _, _, rel, _ = _fixture()
    pairs = nc.seven_pairs()
    env = _env(nc.N)
    env.state = st
    _attach_fixture(env)
    env.set_distance_pairs(pairs)
    for _ in range(2):                                                                       # another handle, two calls: the same bytes
        assert _same(carry['sg'], _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True)))
        assert _same(carry['pc'], _copy(env.posture_clearance(po, host=True)))
    # a row's place among the K: the postures in reverse order
    rev = _copy(env.signed_distance_gradient(np.ascontiguousarray(po[:, ::-1]), margin=MARGIN, host=True))
    assert _same(carry['sg'], {k: v[:, ::-1] for k, v in rev.items()})
    # K and the neighbours' attachments: only env 1 attached, K = 1 -- env 1's row keeps its bytes
    env.detach_objects(np.array([0, 0, 1, 1, 1], np.uint8))
    assert env.attachments()[0].tolist() == [[-1] * 3, [8, -1, -1]] + [[-1] * 3] * 3
    one = _copy(env.signed_distance_gradient(np.ascontiguousarray(po[:, 2:3]), margin=MARGIN, host=True))
    assert _same({k: v[1, 2] for k, v in carry['sg'].items()}, {k: v[1, 0] for k, v in one.items()})
    env.close()
    # N = 2 (envs 1 and 2 of the fixture), K = 32: the first three rows are the fixture's, and every row of 32 is written
    small = _env(2)
    small.state = st[1:3]
    _attach_fixture(small, slice(1, 3))
    assert (small.attachments()[1] == rel[1:3]).all()
    small.set_distance_pairs(pairs)
    wide = np.ascontiguousarray(np.concatenate([po[1:3]] + [po[1:3, ::-1]] * 9 + [po[1:3, :2]], 1))
    assert wide.shape == (2, 32, 11)
    out = _copy(small.signed_distance_gradient(wide, margin=MARGIN, host=True))
    assert out['gradient'].shape == (2, 32, 11)
    assert _same({k: v[1:3] for k, v in carry['sg'].items()}, {k: v[:, :3] for k, v in out.items()})
    assert _same({k: v[:, 30:32] for k, v in out.items()}, {k: v[:, :2] for k, v in out.items()})
    pc = _copy(small.posture_clearance(wide, host=True))
    assert _same({k: v[1:3] for k, v in carry['pc'].items()}, {k: v[:, :3] for k, v in pc.items()})
    # the step's 92 collision pairs, N = 2, K = 2: against float64 on the decided items with an attached shape
    small.set_distance_pairs('collision')
    table = nd.collision_pairs(3)
    two = np.ascontiguousarray(po[1:3, :2])
    big = _copy(small.signed_distance_gradient(two, margin=MARGIN, host=True))
    small.close()
    ref = nd.reference(nc.carried_rows(st[1:3], two, links[1:3], rel[1:3].astype(np.float64)), table)
    att = nc.attached_items(links[1:3], table, 2)
    m = ref['decided'] & att
    err = np.abs(big['pair_distance'].reshape(4, 92).astype(np.float64) - ref['d'])
    print('collision table: %d decided items with an attached shape, |device - float64| %.3g (ceiling %.3g); %d others %.3g'
          % (m.sum(), err[m].max(), CEIL_D, (ref['decided'] & ~att).sum(), err[ref['decided'] & ~att].max()))
    assert m.sum() >= 60 and err[m].max() <= CEIL_D and err[ref['decided'] & ~att].max() <= max(TOL_DIST, TOL_SD)
    assert (big['pair_status'].reshape(4, 92)[ref['decided']] == ref['expect'][ref['decided']]).all()


def test_no_effect_on_the_simulation():
    """N = 8: steps with attachments set and the three queries between them give the bytes of steps without; so do steps with
    attachments alone."""
    from real_robots_amd.distributed import synthetic_actions
    a, b, c = _env(8), _env(8), _env(8)
    po = np.ascontiguousarray(nd.states(24, 121)[:, :11].reshape(8, 3, 11))
    for e in (a, b, c):
        e.reset()
    a.set_distance_pairs(npo.robot_pairs())
    fields = (nat.F_STATE, nat.F_PREP, nat.F_ERRFLAGS, nat.F_TOUCH, nat.F_CONTACT_COUNT)
    for t in range(12):
        cmd = synthetic_actions(list(range(8)), t)
        for e in (a, b, c):
            e.step(cmd)
        if t == 2:
            a.attach_objects({'cube': 'base', 'mustard': 'finger_11'})
            c.attach_objects({'cube': 'base'})
        if t >= 2:
            before = [a.host(f).tobytes() for f in fields]
            a.posture_clearance(po, host=True)
            a.signed_distance(po if t % 2 else None, host=(t % 3 == 0))
            a.signed_distance_gradient(None if t % 2 else po, margin=MARGIN)
            if t == 6:
                a.attach_objects({'tomato': 4}, env_mask=np.arange(8) % 2 == 0)
            assert before == [a.host(f).tobytes() for f in fields], t
        for f in fields:
            assert a.host(f).tobytes() == b.host(f).tobytes() == c.host(f).tobytes(), (t, f)
    assert (a.posture_buffer('distance', host=True) != 0).any() and (a.attachments()[0] >= 0).any()
    for e in (a, b, c):
        e.close()


def test_life_cycle_and_refusals():
    st, po, links, given, carry, twin, _, rel, _ = _fixture()
    pairs = nc.seven_pairs()
    env = _env(nc.N)
    L = env.L
    # before anything is attached: all free, detaching is fine, the sweep works
    l0, r0 = env.attachments()
    assert (l0 == -1).all() and (r0 == np.array([0, 0, 0, 0, 0, 0, 1], np.float32)).all()
    env.detach_objects()
    env.detach_objects(np.ones(nc.N, np.uint8))
    env.state = st
    env.set_distance_pairs(pairs)
    seg = np.ascontiguousarray(np.stack([np.repeat(st[:, None, :11], 3, 1), po], 2))
    sweep0 = _copy(env.swept_clearance(seg, host=True))
    _attach_fixture(env)
    table = env.attachments()
    assert (table[0] == links).all() and (table[1] == rel).all()

    def unchanged():
        now = env.attachments()
        return (now[0] == table[0]).all() and (_bits(now[1]) == _bits(table[1])).all()
    # the table survives a reset, a state write, a step, a pair table and a fork of other envs; fork leaves the destination's row
    env.reset(np.array([0, 1, 0, 0, 0], np.uint8))
    env.write_state(st, obj_pose=True, joint_pos=True)
    env.step(np.zeros((nc.N, 9), np.float32))
    env.set_distance_pairs(nc.two_pairs())
    env.set_distance_pairs(pairs)
    assert unchanged()
    env.fork(np.array([3, -1, 1, -1, 0], np.int32))
    assert unchanged()
    env.state = st
    assert _same(carry['sg'], _copy(env.signed_distance_gradient(po, margin=MARGIN, host=True)))
    # the refusals: RR_EINVAL, the message names env and object, nothing changes
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    bad_link, world_link, masked_bad = links.copy(), links.copy(), links.copy()
    bad_link[2, 1], world_link[3, 2], masked_bad[0, 0] = 17, 0, 99
    nan_rel, zero_q = given.copy(), given.copy()
    nan_rel[4, 2, 1], zero_q[1, 0, 3:] = np.nan, 0.0
    cases = [((i32(bad_link), None, None), ('env 2, object 1', 'link 17')), ((i32(world_link), None, None), ('env 3, object 2', 'rigid with the world')),
             ((i32(links), f32(nan_rel), None), ('env 4, object 2', 'not finite')), ((i32(links), f32(zero_q), None), ('env 1, object 0', 'norm zero')),
             ((i32(-2 * np.ones_like(links)), None, None), ('env 0, object 0', 'link -2')), ((None, f32(given), None), ('rel_pose without link',))]
    for (lk, rp, mk), words in cases:
        rc = L.rr_set_attachments(env.h, lk.ctypes.data if lk is not None else None, rp.ctypes.data if rp is not None else None, mk)
        msg = L.rr_last_error().decode()
        assert rc == -1 and 'rr_set_attachments' in msg and all(w in msg for w in words), msg
        assert unchanged()
    mask = np.array([0, 1, 1, 1, 1], np.uint8)                                               # a bad row outside the mask is not looked at
    masked_bad = i32(masked_bad)
    assert L.rr_set_attachments(env.h, masked_bad.ctypes.data, None, mask.ctypes.data) == 0
    nan_free, lk, given_mask = given.copy(), i32(links), np.ascontiguousarray(1 - nc.CAPTURED)
    nan_free[4, 0] = np.nan                                                                  # ... nor the rel pose of a free object
    env.attach_objects(links, given, env_mask=given_mask)
    assert L.rr_set_attachments(env.h, lk.ctypes.data, nan_free.ctypes.data, given_mask.ctypes.data) == 0
    assert (env.attachments()[0] == links).all()
    with pytest.raises(nat.NativeError, match='rigid with the world'):
        env.attach_objects({'cube': 0})
    # the sweep refuses while attachments are on, and writes nothing
    sw_before = [env.sweep_buffer(i, host=True).tobytes() for i in range(len(nat.SW_FIELDS))]
    assert L.rr_swept_clearance(env.h, seg.ctypes.data, 3, 0, 0.0, 1e-3) == -1
    msg = L.rr_last_error().decode()
    assert 'rr_swept_clearance' in msg and 'attach' in msg
    assert sw_before == [env.sweep_buffer(i, host=True).tobytes() for i in range(len(nat.SW_FIELDS))]
    with pytest.raises(nat.NativeError, match='attached'):
        env.swept_clearance(seg)
    # a masked detach frees only the masked envs, and the feature stays on
    env.detach_objects(np.array([0, 0, 1, 0, 0], np.uint8))
    now = env.attachments()[0]
    assert (now[2] == -1).all() and (np.delete(now, 2, 0) == np.delete(links, 2, 0)).all()
    part = _copy(env.signed_distance(po, host=True))
    assert _same(part, twin['sd'], sel=2) and _same(part, carry['sd'], sel=[0, 1, 3, 4])
    assert L.rr_swept_clearance(env.h, seg.ctypes.data, 3, 0, 0.0, 1e-3) == -1
    # the unmasked detach: every buffer equals the never-attached twin's, byte for byte, and the sweep works again
    env.detach_objects()
    assert (env.attachments()[0] == -1).all()
    off = _queries(env, st, po, pairs)
    for name in off:
        assert _same(off[name], twin[name]), name
    assert _same(sweep0, _copy(env.swept_clearance(seg, host=True)))
    # ... and attaching again gives the carried answers again
    _attach_fixture(env)
    assert _same(carry['pc'], _copy(env.posture_clearance(po, host=True)))
    env.close()
