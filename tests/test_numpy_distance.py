"""CPU tests (-m "not gpu") of the float64 reference of the closest-point queries (tests/numpy_distance.py): analytic box-box
distances, the symmetry of a swap, the conditions on the seeded inputs of the GPU test (enough decided items, every pair class
decided somewhere), and that every negative control has teeth."""
import numpy as np
import pytest

from tests import numpy_distance as nd

BOX = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)


def _rot(axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def test_analytic_box_box_distances():
    A = BOX * [0.5, 0.5, 0.5]
    # face - face: unit cubes 0.3 apart along x, shifted sideways (the closest vector is unique although the points are not)
    d, v = nd.signed_distance(A, A + [1.3, 0.2, -0.1])
    assert abs(d - 0.3) < 1e-12 and np.abs(v - [-0.3, 0, 0]).max() < 1e-12
    # edge - edge, crossed: an edge along y of a cube turned by 45 degrees about y against an edge along z of one turned about z
    Ae = A @ _rot([0, 1, 0], np.pi / 4).T                            # edges along y at x = +- sqrt(0.5), z = 0
    Bc = A @ _rot([0, 0, 1], np.pi / 4).T                            # edges along z at x = +- sqrt(0.5), y = 0
    d, v = nd.signed_distance(Ae, Bc + [2 * np.sqrt(0.5) + 0.1, 0, 0])
    assert abs(d - 0.1) < 1e-12 and np.abs(v - [-0.1, 0, 0]).max() < 1e-12          # crossed edges (y against z) 0.1 apart
    # vertex - face: a cube standing on its corner (body diagonal along z) above A's top face
    Rc = _rot([1, -1, 0], np.arccos(1 / np.sqrt(3)))
    C = A @ Rc.T
    assert abs(C[:, 2].min() + np.sqrt(0.75)) < 1e-12
    d, v = nd.signed_distance(C + [0.1, -0.2, 0.5 + 0.4 + np.sqrt(0.75)], A)
    assert abs(d - 0.4) < 1e-12 and np.abs(v - [0, 0, 0.4]).max() < 1e-12
    # vertex - vertex, and overlap: minus the penetration depth, no vector
    d, v = nd.signed_distance(A, A + [1.3, 1.4, 2.2])
    assert abs(d - np.linalg.norm([0.3, 0.4, 1.2])) < 1e-12 and np.abs(v + [0.3, 0.4, 1.2]).max() < 1e-12
    d, v = nd.signed_distance(A, A + [0.9, 0.2, 0.3])
    assert abs(d + 0.1) < 1e-12 and not v.any()


def test_swapping_a_and_b_keeps_the_distance_and_negates_the_vector():
    rng = np.random.default_rng(3)
    for _ in range(5):
        A = BOX * rng.uniform(0.1, 0.4, 3) @ _rot(rng.normal(size=3), rng.uniform(0, 3)).T
        B = rng.normal(size=(30, 3)) * 0.2 + rng.normal(size=3)
        d1, v1 = nd.signed_distance(A, B)
        d2, v2 = nd.signed_distance(B, A)
        assert abs(d1 - d2) < 1e-12 and np.abs(v1 + v2).max() < 1e-12 and (d1 <= 0 or abs(np.linalg.norm(v1) - d1) < 1e-12)


def test_extreme_points_keep_the_hull():
    """The reduction of a vertex set to its extreme points changes no distance (the coplanar statics lose most of their vertices)."""
    from tests import numpy_collide as ncol
    n = nd.names()
    T, C = ncol.shapes()[n['table']]['V'], ncol.shapes()[n['cube']]['V'] + [0.1, 0.2, 0.9]
    assert len(nd.local_vertices(n['table'])) < len(T)
    d1, v1 = nd.signed_distance(C, T)
    d2, v2 = nd.signed_distance(C, nd.local_vertices(n['table']))
    assert abs(d1 - d2) < 1e-12 and np.abs(v1 - v2).max() < 1e-12


def test_the_seeded_cases_are_decided_and_cover_every_pair_class():
    """A condition on the inputs of tests/test_gpu_distance.py, shown by the reference alone."""
    seen = set()
    for N, _, pairs in nd.cases():
        ref = nd.case(N)[2]
        assert ref['decided'].mean() >= 0.9, (N, ref['decided'].mean())
        for j, (a, b) in enumerate(pairs.tolist()):
            if ref['decided'][:, j].any():
                seen |= {nd.vertex_class(a), nd.vertex_class(b)}
    assert seen == set(nd.CLASSES), seen
    assert {nd.vertex_class(s) for s in nd.seven_pairs().ravel().tolist()} == set(nd.CLASSES)
    st, pairs, ref = nd.case(1)
    byname = {tuple(p): j for j, p in enumerate(pairs.tolist())}
    n = nd.names()
    assert abs(ref['d'][0, byname[n['cube'], n['table']]] - 0.005) < 1e-5          # the cube 5 mm above the table, faces parallel
    assert ref['d'][0, byname[n['cube'], n['tomato']]] <= -1e-3                      # overlapping objects, >= 1 mm deep
    st, pairs, ref = nd.case(5)
    assert ref['d'][1, 0] < 0.08 and ref['d'][2, 6] <= -1e-3                         # env 1: the cube between the fingers (pair 0: skin_00, cube); env 2: tomato and cube overlap
    cull = nd.case(1, max_distance=0.05)[2]
    assert (cull['decided'] & cull['culled']).sum() >= 10 and (cull['decided'] & ~cull['culled']).sum() >= 10


@pytest.mark.parametrize('variant', nd.VARIANTS)
def test_negative_controls_have_teeth(variant):
    """Every variant differs from the reference on decided items: by at least 1 mm in the distance or 0.1 rad in the direction."""
    ref, var = nd.case(5)[2], nd.case(5, variant=variant)[2]
    m = ref['decided'] & (ref['d'] > 0)
    dd = np.abs(np.maximum(var['d'], 0) - ref['d'])[m]
    cos = (var['v'] * ref['v']).sum(-1)[m] / np.maximum(np.linalg.norm(var['v'], axis=-1) * np.linalg.norm(ref['v'], axis=-1), 1e-300)[m]
    ang = np.arccos(np.clip(cos, -1, 1))
    print(variant, 'max distance change %.3g m, max angle %.3g rad, control error %.3g m' % (dd.max(), ang.max(), nd.control_error(ref, var)))
    assert dd.max() >= 1e-3 or ang.max() >= 0.1
    assert nd.control_error(ref, var) >= 1e-3
