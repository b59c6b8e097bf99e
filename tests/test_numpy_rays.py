"""CPU tests (-m "not gpu") of the float64 ray-cast reference (tests/numpy_rays.py) itself: a brute-force march along the segments,
the coverage of the aimed ray set, the cap on undecided rays for the inputs the GPU test uses, and the negative controls."""
import numpy as np
import pytest

from tests import numpy_rays as nr

STEP = 1e-4          # m between the samples of the march


@pytest.fixture(scope='module')
def cases():
    out = {}
    for N, nobj in nr.CASES:
        st, links, segs = nr.case(N, nobj)
        out[N] = (st, links, segs, nobj, nr.cast(st, links, segs, nobj))
    return out


def test_brute_force_march_brackets_the_hit(cases):
    """About 200 decided rays of at most 1 m: inside(x) on samples 1e-4 m apart (and at the end point).  A hull that holds the
    origin is out of the race.  The first sample inside a hull is at most one sample behind the reference's hit, that hull is the
    reference's winner, and a segment without such a sample is a miss of the reference."""
    st, links, segs, nobj, ref = cases[131]
    n_checked = n_hits = 0
    worst = 0.0
    for n in range(4):
        for r in range(64):
            L = ref['length'][n, r]
            if not ref['decided'][n, r] or L > 1.0 or L == 0:
                continue
            t = np.append(np.arange(0.0, L, STEP), L) / L
            x = ref['start'][n, r] + t[:, None] * (ref['end'][n, r] - ref['start'][n, r])
            ins = nr.inside_any(x, st[n], nobj)
            ins[:, ins[0]] = False                                   # hulls that hold the origin
            first = np.flatnonzero(ins.any(1))
            n_checked += 1
            if len(first) == 0:
                assert ref['shape'][n, r] == -1, (n, r, ref['shape'][n, r], ref['distance'][n, r])
                continue
            i = first[0]
            n_hits += 1
            assert ref['shape'][n, r] >= 0 and ins[i, ref['shape'][n, r]], (n, r, np.flatnonzero(ins[i]), ref['shape'][n, r])
            d = ref['distance'][n, r]
            assert t[i - 1] * L - 1e-9 <= d <= t[i] * L + 1e-9, (n, r, d, t[i - 1] * L, t[i] * L)
            worst = max(worst, t[i] * L - d)
    print("march: %d rays, %d hits, hit at most %.2e m in front of its first inside sample" % (n_checked, n_hits, worst))
    assert n_checked >= 180 and n_hits >= 60


def test_every_shape_wins_an_aimed_ray(cases):
    st, links, segs, nobj, ref = cases[131]
    sel = ref['decided'] & (ref['shape'] >= 0)
    wins = np.bincount(ref['shape'][sel], minlength=22)
    print("wins per shape:", wins)
    assert len(wins) == 22 and (wins > 0).all()
    # the handle with one object: shapes of objects 1 and 2 do not exist
    ref3 = cases[3][4]
    assert not np.isin(ref3['shape'], (20, 21)).any()
    # the special rays: 1 mm short of the table top is a miss, 1 mm beyond hits the table, the tie goes to the lower plane (+x)
    assert (ref['shape'][:, 22][ref['decided'][:, 22]] != 0).all() and ((ref['shape'][:, 23] == 0) | (ref['distance'][:, 23] < 0.6)).all()
    tie = ref['decided'][:, 24] & (ref['shape'][:, 24] == 1)
    assert tie.sum() > 100 and (ref['normal'][tie, 24] == [1, 0, 0]).all() and (ref['fraction'][tie, 24] == 0.5).all()
    # zero-length rays are misses with nothing to decide
    zero = ref['length'] == 0
    assert zero.any() and (ref['shape'][zero] == -1).all() and ref['decided'][zero].all()
    # rays that start inside their own link's hull do not hit it
    ids = nr.shape_ids()
    for r in range(26, 36):
        own = ids[:, 2] == links[r]
        assert not np.isin(ref['shape'][:, r], np.flatnonzero(own)).any(), r


def test_undecided_rays_stay_under_the_cap(cases):
    """A condition on the inputs, not a tolerance: at most 5 % of the rays of every case the GPU test runs are undecided."""
    for N, nobj in nr.CASES:
        st, links, segs, _, ref = cases[N]
        fr = [1 - ref['decided'].mean()]
        for R in (1, 5):
            l, s = nr.table_rays(R, nr.SEED + 200)
            fr.append(1 - nr.cast(st, l, s, nobj)['decided'].mean())
        print("N = %d: undecided %.4f (64 per-env rays), %.4f (table of 1), %.4f (table of 5)" % (N, *fr))
        assert max(fr) < nr.UNDECIDED_CAP, (N, fr)


def test_compare_accepts_the_reference_and_rejects_every_variant(cases):
    for N, nobj in nr.CASES:
        st, links, segs, _, ref = cases[N]
        fig, fails = nr.compare(*nr.as_device(ref), ref)
        assert not fails, fails
        if N < 100:
            continue
        for v in nr.VARIANTS:
            fig, fails = nr.compare(*nr.as_device(nr.cast(st, links, segs, nobj, variant=v)), ref)
            print(v, fails[:2])
            assert fails, v
