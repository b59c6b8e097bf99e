"""GPU tests (-m gpu): the device's preparation record and contact solve against the float64 numpy step (tests/numpy_step.py).

Every other GPU test of the step compares the kernels with the oracle (oracle/rr_oracle.c) or with another kernel form; a slip
those share -- a sign in a row, the frame of an inertia, a missing gyroscopic or Coriolis term, a material combiner -- would pass
them all.  Here the reference is computed independently: the Lagrangian bias by complex step, complex-step contact Jacobians,
dense rows over generalised velocities, materials combined from each env's own dynamics rows.
"""
import numpy as np
import pytest

from real_robots_amd import _native as nat
from real_robots_amd.batched import BatchedREALRobotEnv
from real_robots_amd.distributed import synthetic_actions
from tests import numpy_step as ns
from tests.test_gpu_contacts_fuzz import state_bounds, SENS_FACTOR, SENS_RUNS
from tests.test_gpu_object_dynamics import PATHS, _drive
from tests.test_gpu_round6 import (_make, _rich_states, S_BR, S_BP, S_BAX, S_MINV, S_QDS, S_OR, S_OIINV, S_OVS, S_OWS, S_OP,
                                   S_TOTAL)

pytestmark = pytest.mark.gpu

PREP_PATHS = {'scalar': {'RR_PREP_SCALAR': '1', 'RR_NO_LOOKAHEAD': '1'}, 'p16': {'RR_NO_LOOKAHEAD': '1'}, 'lookahead': {}}


def random_dynamics(n, seed):
    """Per-env dynamics rows [n, 3, 8]: mass x 0.2-5, anisotropic inertia (each axis x 0.5-2 on top of the mass ratio), friction,
    restitution, rolling and spinning friction drawn around the model's."""
    rng = np.random.default_rng(seed)
    d = np.broadcast_to(ns.default_dynamics(), (n, 3, 8)).copy()
    k = np.exp(rng.uniform(np.log(0.2), np.log(5.0), (n, 3)))
    d[..., 0] *= k
    d[..., 1:4] *= k[..., None] * rng.uniform(0.5, 2.0, (n, 3, 3))
    d[..., 4] = rng.uniform(0.1, 1.2, (n, 3))
    d[..., 5] = rng.uniform(0.0, 0.8, (n, 3))
    d[..., 6:8] = rng.uniform(0.0, 0.05, (n, 3, 2))
    return d.astype(np.float32)


def edge_states(N, seed):
    """_rich_states with edges: qd = 0 exactly, objects exactly at rest, |w| ~ 50 rad/s, quaternions with w ~ 0 and w = +-1,
    near-singular postures (elbow straight, wrist axes aligned), objects past the out-of-bounds rule, joints at 40 rad/s."""
    st = _rich_states(N, seed)
    rng = np.random.default_rng(seed)
    ob = st[:, 22:61].reshape(N, 3, 13)
    for i in range(N):
        e = i % 8
        if e == 0:
            st[i, 11:22] = 0.0
        elif e == 1:
            ob[i, :, 7:13] = 0.0
        elif e == 2:
            w = rng.normal(size=(3, 3))
            ob[i, :, 10:13] = 50.0 * w / np.linalg.norm(w, axis=1, keepdims=True)
        elif e == 3:
            v = rng.normal(size=(3, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            ob[i, :, 3:6], ob[i, :, 6] = v * np.sqrt(1 - 1e-8), 1e-4
        elif e == 4:
            ob[i, :, 3:7] = [[0, 0, 0, 1], [0, 0, 0, -1], [0, 0, 0, 1]]
        elif e == 5:
            st[i, 3], st[i, 5] = 0.0, 1e-7
        elif e == 6:
            ob[i, 0, :3] = [-0.1, 0.0, 0.05]
            ob[i, 1, :3] = [0.2, 0.1, 0.25]
        else:
            st[i, 11:22] = rng.uniform(-40, 40, 11)
    st[:, 22:61] = ob.reshape(N, 39)
    return st.astype(np.float32)


def prep_ratios(rec, st, dyn):
    """Worst ratio of |device - numpy| to the float32 ceiling of every field of RR_F_PREP."""
    N = len(st)
    ref = ns.prep(st.astype(np.float64), dyn.astype(np.float64))
    rec = rec.astype(np.float64)
    qd = np.abs(st[:, 11:22].astype(np.float64)).max(1, keepdims=True)
    ob = st[:, 22:61].astype(np.float64).reshape(N, 3, 13)
    ob[ref['oob']] = 0.0
    vn = np.linalg.norm(ob[..., 7:10], axis=-1)[..., None]
    wn = np.linalg.norm(ob[..., 10:13], axis=-1)[..., None]
    Minv = ref['Minv']
    # (qd*: the issue's 2e-4 + 2e-6 |qd| is linear in |qd|, but the velocity terms of the bias are quadratic: at 40 rad/s on every
    # joint dt M^-1 b reaches 90 rad/s and the first run found float32 errors of 1.2e-5 of it, the scalar kernel 4x over the linear
    # ceiling.  A term of float32 epsilon x the mass matrix's condition (~1e3 here) times |dt M^-1 b| covers that rounding.)
    bterm = np.abs(ns.DT * np.einsum('nij,nj->ni', Minv, ref['bias'])).max(1, keepdims=True)
    scale_m = np.sqrt(np.einsum('nii,njj->nij', Minv, Minv))
    Iinv = ref['oIinv'].reshape(N, 3, 9)
    out = {
        'frames R': np.abs(rec[:, S_BR:S_BP] - ref['R'].reshape(N, 99)) / 2e-6,
        'frames p': np.abs(rec[:, S_BP:S_BAX] - ref['p'].reshape(N, 33)) / 2e-6,
        'joint axes': np.abs(rec[:, S_BAX:S_MINV] - ref['axis'].reshape(N, 33)) / 2e-6,
        'M^-1': np.abs(rec[:, S_MINV:S_QDS].reshape(N, 11, 11) - Minv) / (1e-4 * scale_m),
        'qd*': np.abs(rec[:, S_QDS:S_OR] - ref['qds']) / (2e-4 + 2e-6 * qd + 5e-5 * bterm),
        'object R': np.abs(rec[:, S_OR:S_OIINV] - ref['oR'].reshape(N, 27)) / 2e-6,
        'object I^-1': np.abs(rec[:, S_OIINV:S_OVS].reshape(N, 3, 9) - Iinv) / (1e-5 * np.abs(Iinv).max(-1, keepdims=True)),
        'v*': np.abs(rec[:, S_OVS:S_OWS].reshape(N, 3, 3) - ref['ovs']) / (1e-6 * (1 + vn)),
        'w*': np.abs(rec[:, S_OWS:S_OP].reshape(N, 3, 3) - ref['ows']) / (1e-6 * (1 + wn)),
        'collision position': np.abs(rec[:, S_OP:S_TOTAL].reshape(N, 3, 3) - ref['opos']) / 2e-6,
    }
    q = out['qd*']
    n, j = np.unravel_index(int(np.argmax(q)), q.shape)
    print("  worst qd*: env %d (edge %d) joint %d: device %.6f numpy %.6f; max|qd| %.1f, |dt M^-1 b| %.1f" % (
        n, n % 8, j, rec[n, S_QDS + j], ref['qds'][n, j], qd[n, 0], bterm[n, 0]))
    return {k: float(v.max()) for k, v in out.items()}


@pytest.mark.parametrize('N', [1, 5, 17, 4096])
def test_prep_record_matches_the_numpy_preparation(monkeypatch, N):
    """RR_F_PREP field by field against numpy under the three preparation paths: the thread-per-env kernels, the 16-lane kernel,
    and the look-ahead (the record then describes the state the step left).  Ceilings from float32 arithmetic, not measured."""
    st = edge_states(N, 3)
    dyn = random_dynamics(N, 5)
    for path, envv in PREP_PATHS.items():
        env = _make(monkeypatch, envv, N, objects=3, width=64, height=64)
        env.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(dyn))
        env.state = st
        env.step(None)
        rec, used = env.host(nat.F_PREP), (st if path != 'lookahead' else env.state)
        assert (env.host(nat.F_ERRFLAGS) == 0).all()
        env.close()
        r = prep_ratios(rec, used, dyn)
        print("N=%d %s: worst |device - numpy| / ceiling: %s" % (N, path, ', '.join('%s %.3f' % kv for kv in r.items())))
        assert max(r.values()) < 1.0, (path, r)


def _perturbed_spread(st0, cmd, cd, prev, dyn, iters, ref, rng):
    """The numpy step's own spread when every entry of the float32 start state moves by one unit in the last place."""
    sj = so = sv = 0.0
    for _ in range(SENS_RUNS):
        up = rng.random(st0.shape) < 0.5
        stp = np.where(up, np.nextafter(st0, np.float32(np.inf)), np.nextafter(st0, np.float32(-np.inf)))
        d = np.abs(ns.step(stp.astype(np.float64), cmd, cd, dyn=dyn, prev=prev, solver_iters=iters)['state'] - ref)
        dobj = d[22:61].reshape(3, 13)
        sj, so, sv = max(sj, float(d[:22].max())), max(so, float(dobj[:, :7].max())), max(sv, float(dobj[:, 7:].max()))
    return sj, so, sv


def _dev(a, b):
    d = np.abs(np.asarray(a, np.float64) - b)
    dobj = d[22:61].reshape(3, 13)
    return float(d[:22].max()), float(dobj[:, :7].max()), float(dobj[:, 7:].max())


@pytest.mark.parametrize('path', list(PATHS) + ['iters1'])
def test_contact_step_matches_the_numpy_step(monkeypatch, path):
    """One step of the contact solve from each checked env's device state and contact history, against the numpy step on the
    device's own new contact list, in a 96-env batch with per-env dynamics driven like the per-env dynamics tests."""
    N = 96
    iters = 1 if path == 'iters1' else 50
    env = _make(monkeypatch, PATHS.get(path, {}), N, objects=3, width=64, height=64, solver_iters=iters)
    dyn = random_dynamics(N, 9)
    env.set_object_dynamics(**BatchedREALRobotEnv._dynamics_dict(dyn))
    dyn64 = dyn.astype(np.float64)
    _drive([env], 160, seed=3)
    rng = np.random.default_rng(1)
    occurred, seen_cls, pairs, limit_active, worst, checked = set(), set(), set(), 0, [0.0, 0.0, 0.0], 0
    controls = []
    cls_name = lambda b: 'object' if b >= 16 else 'robot' if b >= 0 else 'static'
    lim = ns.model()['body_limits']
    limited = [j for j in range(11) if lim[j][0] < lim[j][1]]
    for t in range(160, 300):
        cmd = (synthetic_actions(range(N), t, seed=3) * 1.6).astype(np.float32)
        if t % 35 != 0:
            env.step(cmd)
            continue
        st0 = env.state
        caches = [env.contacts(i) for i in range(N)]
        env.step(cmd)
        st1, cls = env.state, env.host(nat.F_ENV_CLASS)
        occurred |= set(int(c) for c in cls)
        new = [env.contacts(i) for i in range(N)]
        picks = []
        for c in (0, 1, 2):                       # every class, most contacts first
            members = [i for i in range(N) if cls[i] == c]
            picks += sorted(members, key=lambda i: -len(new[i]))[:3]
        # envs with an object x object contact, and envs with a robot contact and a limited joint within 0.01 rad of a limit
        picks += [i for i in range(N) if ((new[i][:, 0] >= 16) & (new[i][:, 1] >= 16)).any()][:3]
        picks += [i for i in range(N) if ((new[i][:, 0] >= 0) & (new[i][:, 0] < 16)).any()
                  and min(min(abs(st0[i][j] - lim[j][0]), abs(st0[i][j] - lim[j][1])) for j in limited) < 0.01][:3]
        for i in sorted(set(picks)):
            cd = env.contacts(i)
            res = ns.step(st0[i].astype(np.float64), cmd[i].astype(np.float64), cd, dyn=dyn64[i], prev=caches[i], solver_iters=iters)
            ref = res['state']
            assert np.array_equal(cd[:, 11], res['mat'][:, 0].astype(np.float32)), "mu of env %d" % i
            fmax = float(cd[:, 10].max()) if len(cd) else 0.0
            b = state_bounds(fmax)
            d = _dev(st1[i], ref)
            if any(x > y for x, y in zip(d, b)):
                s = _perturbed_spread(st0[i], cmd[i].astype(np.float64), cd, caches[i], dyn64[i], iters, ref, rng)
                b = tuple(max(x, SENS_FACTOR * y) for x, y in zip(b, s))
            assert all(x <= y for x, y in zip(d, b)), (path, i, int(cls[i]), fmax, d, b)
            worst = [max(w, x / y) for w, x, y in zip(worst, d, state_bounds(fmax))]
            seen_cls.add(int(cls[i]))
            checked += 1
            pairs |= {(cls_name(int(c[0])), cls_name(int(c[1]))) for c, l in zip(cd, res['lambda_n']) if l > 0}
            limit_active += sum(1 for r, l in zip(res['rows'], res['lam']) if r[0] == 'limit' and l > 0)
            controls.append((i, st0[i], cmd[i], cd, caches[i], st1[i], b))
    print("%s: %d checks; worst deviation / flat bound: joints %.3f, object pose %.3f, object velocity %.3f; pairs %s; %d active limit rows"
          % (path, checked, worst[0], worst[1], worst[2], sorted(pairs), limit_active))
    assert seen_cls == occurred and len(occurred) >= 2, (seen_cls, occurred)
    if path in ('default', 'scalar_prep', 'no_split'):
        assert occurred == {0, 1, 2}
    assert {('robot', 'object'), ('object', 'static')} <= pairs, pairs
    if path != 'iters1':               # (one sweep per step drives another trajectory: no pile, no limit contact at these steps)
        assert ('object', 'object') in pairs and limit_active > 0, (pairs, limit_active)
    # negative controls on the checked cases: each slip must push some case far outside its bound
    def control(**kw):
        worst_c = 0.0
        for i, s0, c, cd, prev, s1, b in controls:
            dn = dyn64[(i + 1) % N] if kw.get('neighbour') else dyn64[i]
            r = ns.step(s0.astype(np.float64), c.astype(np.float64), cd, dyn=dn, prev=prev, solver_iters=iters, drop=kw.get('drop', ()))
            worst_c = max(worst_c, max(x / y for x, y in zip(_dev(s1, r['state']), b)))
        return worst_c
    ratios = {'coriolis': control(drop=('coriolis',)), 'neighbour dynamics': control(neighbour=True)}
    if path == 'iters1':
        ratios['reversed normals'] = control(drop=('reverse_normals',))
    print("%s: negative controls, worst deviation / bound: %s" % (path, ratios))
    assert min(ratios.values()) > 10.0, ratios
    env.close()
