#!/usr/bin/env python3
"""Generates tests/golden/signed_gradient.npz: the float64 reference that tests/test_numpy_signed_gradient.py and
tests/test_gpu_signed_gradient.py hold rr_signed_gradient to -- FINITE DIFFERENCES of tests/numpy_distance.reference (qhull on the
Minkowski difference: no GJK, no Jacobian) over the eleven joints, at H = 1e-3 rad, for

  case R   tests/numpy_posture.case_r_inputs: N = 4, K = 4, the 80 robot pairs of the collision table (keys r_*, rows e * K + k);
  case 5   tests/numpy_distance.case(5): the present state of 5 envs, seven pairs (keys p_*).

Per case: d0 [R, Q], dplus / dminus [R, Q, 11] (the distance with joint k moved by +-H), from which the tests form central, forward
and backward differences (numpy_signed_gradient.derivatives) and the items they compare (numpy_signed_gradient.compared: decided and
max_k |forward - backward| <= SMOOTH, both read off the reference alone).

The float64 formula's own agreement: the header's expression, on witness points from the supporting vertex sets
(numpy_signed_gradient.witness), against the central differences on every item of both cases; its largest error over the compared
items, times four, is TOL_G -- what the device may differ from the differences by (it adds float32 witness and frame rounding only,
about 1e-6 m on levers of at most about 1 m).  *_formula [R, Q, 11] and *_unique [R, Q] keep the restatement's values.

The cost: r_cost_fd [16, 11], central differences of the float64 hinge cost (margin 0.05 m) of case R's rows over all 80 pairs, and
r_cost_rows [16]: the rows on which no pair lies within 1e-3 m of the margin and every pair inside the margin is smooth.

Run here (CPU only, a few minutes):  python tests/golden/make_signed_gradient.py
"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import numpy_distance as nd               # noqa: E402
from tests import numpy_posture as npo               # noqa: E402
from tests import numpy_signed_gradient as nsg       # noqa: E402
from tests import numpy_step as ns                   # noqa: E402


def _one(job):
    rows, pairs, k, sg = job
    s = np.asarray(rows, dtype=np.float64).copy()
    if k >= 0:
        s[:, k] += sg * nsg.H
    return nd.reference(s, pairs)['d']


def differences(pool, rows, pairs):
    jobs = [(rows, pairs, -1, 0.0)] + [(rows, pairs, k, sg) for k in range(ns.NB) for sg in (1.0, -1.0)]
    out = pool.map(_one, jobs, chunksize=1)
    return out[0], np.stack(out[1::2], -1), np.stack(out[2::2], -1)


def quantile(x, q):
    return float(np.quantile(x, q)) if len(x) else 0.0


def main():
    st, po, pairs_r = npo.case_r_inputs()
    rows_r = npo.rows(st, po)
    st5, pairs_5, _ = nd.case(5)
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        r = differences(pool, rows_r, pairs_r)
        p = differences(pool, st5, pairs_5)
    out, err, cmp_, over = {}, [], [], 0
    for tag, rows, pairs, (d0, dp, dm) in (('r', rows_r, pairs_r, r), ('p', st5, pairs_5, p)):
        cen, fwd, bwd = nsg.derivatives(d0, dp, dm)
        items = [(i, j) for i in range(d0.shape[0]) for j in range(d0.shape[1])]
        W = nsg.witnesses(rows, pairs, items)
        g = nsg.formula_items(rows, pairs, items, W).reshape(cen.shape)
        ok = nsg.compared(d0, fwd, bwd)
        dec = np.abs(d0) >= nd.DECIDE
        e = np.abs(g - cen).max(-1)
        print('case %s: %d items, %d decided, %d compared (%.1f %%), overlapping %d of which compared %d, non-unique witnesses %d'
              % (tag, d0.size, dec.sum(), ok.sum(), 100.0 * ok.sum() / dec.sum(), (dec & (d0 < 0)).sum(), (ok & (d0 < 0)).sum(),
                 (~W['unique']).sum()))
        print('   formula vs central: 99 %% quantile %.3g, max %.3g over the decided; max %.3g over the compared; max over compared overlapping %.3g'
              % (quantile(e[dec], 0.99), e[dec].max(), e[ok].max(), e[ok & (d0 < 0)].max() if (ok & (d0 < 0)).any() else 0.0))
        print('   max_k |fwd - bwd|: 99 %% quantile %.3g; largest |ds/dq| %.3g; |W.s - d0| max %.3g'
              % (quantile(np.abs(fwd - bwd).max(-1)[dec], 0.99), np.abs(cen).max(), np.abs(W['s'].reshape(d0.shape) - d0).max()))
        err.append(e[ok].max())
        cmp_.append(ok)
        over += int((ok & (d0 < 0)).sum())
        out.update({tag + '_d0': d0, tag + '_dplus': dp, tag + '_dminus': dm, tag + '_formula': g, tag + '_unique': W['unique'].reshape(d0.shape)})
    d0, dp, dm = r
    c = (nsg.cost(np.moveaxis(dp, -1, 1)) - nsg.cost(np.moveaxis(dm, -1, 1))) / (2 * nsg.H)
    active = d0 < nsg.MARGIN
    rows_ok = (np.abs(d0 - nsg.MARGIN) >= nsg.NEAR_MARGIN).all(1) & (cmp_[0] | ~active).all(1)
    print('cost: %d of %d rows compared; largest |dC/dq| %.3g' % (rows_ok.sum(), len(rows_ok), np.abs(c).max()))
    tol_g = 4.0 * max(err)
    print('TOL_G = 4 x %.4g = %.4g m/rad' % (max(err), tol_g))
    out.update(r_cost_fd=c, r_cost_rows=rows_ok, tol_g=np.float64(tol_g), formula_error=np.float64(max(err)), h=np.float64(nsg.H),
               smooth=np.float64(nsg.SMOOTH), margin=np.float64(nsg.MARGIN))
    np.savez_compressed(nsg.FIXTURE, **out)
    print('wrote %s (%d bytes)' % (nsg.FIXTURE, os.path.getsize(nsg.FIXTURE)))


if __name__ == '__main__':
    main()
