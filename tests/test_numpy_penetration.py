"""CPU tests of the float64 penetration reference (tests/numpy_penetration.py) that the GPU tests of rr_signed_distance rely on: a
known depth, the defining property of depth and direction on the seeded items, that the seeded items stay at half the kernel's caps
or below, and that every negative control moves the depth by far more than any tolerance the device may get."""
import numpy as np
import pytest

from tests import numpy_distance as nd
from tests import numpy_penetration as pen

# where a control applies: first_64_vertices_only changes a hull only when a shape of an overlapping item has more than 64 extreme
# vertices -- in case 5 it moves the depth by 0.09 mm only (measured: 0.65 mm in case 1, 1.4 mm in case R)
APPLIES = {c: (('1', 'R') if c == 'first_64_vertices_only' else pen.CASES) for c in pen.CONTROLS}


def _box(lo, hi):
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)


def test_axis_aligned_boxes():
    """Overlaps of 0.3, 0.2 and 0.05 along x, y, z: the depth is 0.05 along z, and A (the upper box) leaves upwards."""
    A, B = _box((0.7, 0.8, 0.95), (1.7, 1.8, 1.95)), _box((0, 0, 0), (1, 1, 1))
    depth, n = pen.nearest_facet(A, B)
    assert abs(depth - 0.05) < 1e-12 and np.allclose(n, (0, 0, 1), atol=1e-12)
    assert abs(nd.signed_distance(A, B)[0] + 0.05) < 1e-12
    assert abs(pen.width(A, B, (0, 0, 1)) - 0.05) < 1e-12 and abs(pen.width(A, B, (1, 0, 0)) - 0.3) < 1e-12 and abs(pen.width(A, B, (0, -1, 0)) - 1.8) < 1e-12
    assert abs(pen.face_normals_only(A, B) - 0.05) < 1e-12            # boxes: the nearest facet is a face of a box
    d, m, trips, faces = pen.expansion(A, B)
    assert abs(d - 0.05) < 1e-12 and np.allclose(m, (0, 0, 1), atol=1e-12) and trips <= 8 and faces <= 16


@pytest.mark.parametrize('name', pen.CASES)
def test_depth_and_direction_separate(name):
    """A moved by (depth + 1e-9) n* is apart, by (depth - 1e-6) n* still overlaps; the width along n* is the depth."""
    ref, pairs = pen.case(name)
    rows, cols = pen.overlapping(ref)
    assert len(rows) == {'1': 9, '5': 4, 'R': 40}[name]
    for e, j in zip(rows, cols):
        A, B = pen.hulls(ref, pairs, e, j)
        depth, n = pen.nearest_facet(A, B)
        assert abs(depth + ref['d'][e, j]) < 1e-12 and abs(np.linalg.norm(n) - 1) < 1e-12
        assert abs(pen.width(A, B, n) - depth) < 1e-12
        assert nd.signed_distance(A + (depth + 1e-9) * n, B)[0] > 0
        assert nd.signed_distance(A + (depth - 1e-6) * n, B)[0] <= 0


@pytest.mark.parametrize('name', pen.CASES)
def test_expansion_reaches_the_depth_at_half_the_caps(name):
    """The float64 expansion reaches the exact depth on every decided overlapping item within 16 trips and 38 faces (measured: 13 / 32
    in case 1, 16 / 38 in case 5, 10 / 26 in case R): the kernel's caps are 32 trips and 64 faces."""
    ref, pairs = pen.case(name)
    worst = [0, 0]
    for e, j in zip(*pen.overlapping(ref)):
        A, B = pen.hulls(ref, pairs, e, j)
        d, n, trips, faces = pen.expansion(A, B)
        assert abs(d + ref['d'][e, j]) < 1e-9 and abs(pen.width(A, B, n) - d) < 1e-12, (e, j)
        worst = [max(worst[0], trips), max(worst[1], faces)]
    print('case %s: expansion trips <= %d, faces <= %d' % (name, *worst))
    assert worst[0] <= 16 and worst[1] <= 38 and worst[0] <= pen.TRIP_CAP // 2 and worst[1] <= pen.FACE_CAP


def test_all_vertex_classes_overlap():
    seen = set()
    for name in pen.CASES:
        ref, pairs = pen.case(name)
        for e, j in zip(*pen.overlapping(ref)):
            seen |= {nd.vertex_class(int(pairs[j][0])), nd.vertex_class(int(pairs[j][1]))}
    assert seen == set(nd.CLASSES)


@pytest.mark.parametrize('control', pen.CONTROLS)
def test_negative_controls_move_the_depth(control):
    """Each deliberately wrong restatement, and the face-normals-only search, moves the depth of some decided overlapping item by at
    least 0.4 mm in every case where it applies (measured for face_normals_only: 1.4 mm, 0.45 mm and 3.9 mm)."""
    errs = {name: pen.control_error(name, control) for name in APPLIES[control]}
    print(control, {k: float('%.3g' % v) for k, v in errs.items()})
    assert min(errs.values()) >= 0.4e-3, errs
    if control == 'face_normals_only':            # an upper bound of the depth, never below it
        for name in pen.CASES:
            ref, _ = pen.case(name)
            rows, cols = pen.overlapping(ref)
            assert (pen.control_depths(name, control) + ref['d'][rows, cols] >= -1e-12).all()
