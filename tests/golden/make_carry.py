"""Writes tests/golden/carry_gradient.npz: the float64 signed distances of tests/numpy_carry.py's fixture at the K postures and with
every joint moved by +-H, THE CARRIED OBJECTS MOVING WITH THEIR LINKS, on the items that have a shape of an attached object (NaN
elsewhere) -- the central differences the carried gradients are held to -- and tol_g, four times the largest disagreement of the
float64 formula (numpy_signed_gradient.formula with numpy_carry.masks, on float64 witnesses) with those differences over the compared
items.  About 1 250 qhull evaluations, 5 s: too much for a test, so the result is committed; tests/test_numpy_carry.py recomputes one
item and the formula's disagreement.

    python -m tests.golden.make_carry
"""
import os

import numpy as np

from tests import numpy_carry as nc
from tests import numpy_signed_gradient as nsg

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'carry_gradient.npz')


def formula_error(d0, dp, dm):
    """(compared [R, Q], the float64 formula's |g - central| per compared item [I], the items [(row, pair)])"""
    st, po, links, _ = nc.inputs()
    pairs = nc.seven_pairs()
    att = nc.attached_items(links, pairs, nc.K)
    cen, fwd, bwd = nsg.derivatives(d0, dp, dm)
    ok = att & nsg.compared(np.nan_to_num(d0), np.nan_to_num(fwd), np.nan_to_num(bwd))
    items = [(int(r), int(j)) for r, j in zip(*np.nonzero(ok))]
    rows = nc.carried_rows(st, po, links, nc.reference_rel())
    W = nsg.witnesses(rows, pairs, items)
    mA, mB = nc.masks(links, pairs, nc.K)
    r, j = np.array([i[0] for i in items]), np.array([i[1] for i in items])
    g = nsg.formula(rows[r, :11], W['a'], W['b'], W['n'], mA[r, j], mB[r, j])
    return ok, np.abs(g - cen[r, j]).max(-1), items


def main():
    st, po, links, _ = nc.inputs()
    pairs = nc.seven_pairs()
    att = nc.attached_items(links, pairs, nc.K)
    items = [(int(r), int(j)) for r, j in zip(*np.nonzero(att))]
    d0, dp, dm = nc.differences(st, po, links, nc.reference_rel(), pairs, items)
    ok, err, _ = formula_error(d0, dp, dm)
    print('%d items with an attached shape, %d compared (%d overlapping); the float64 formula against the differences: %.3g m/rad'
          % (att.sum(), ok.sum(), (ok & (d0 < 0)).sum(), err.max()))
    np.savez_compressed(OUT, seed=nc.SEED, d0=d0, dplus=dp, dminus=dm, tol_g=4 * err.max())


if __name__ == '__main__':
    main()
