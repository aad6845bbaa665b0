"""Marching tetrahedra oracle (oracle/tetmesh_ref.py) against the reference's own utils/tetmesh.py
(tests/golden/tetmesh_reference.npz, tools/gen_tetmesh_golden.py): every output array bit for bit."""
import os

import numpy as np
import pytest

from oracle import tetmesh_ref as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tetmesh_reference.npz")
CASES = ("doc", "qhull", "inside", "outside", "zeros")


def golden_case(name):
    z = np.load(GOLD)
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


def assert_same(got, g):
    (ends, end_sdf), end_scales, faces, ids = got
    for a, b, what in ((ends, g["endpoints"], "endpoints"), (end_sdf, g["endpoint_sdf"], "endpoint sdf"),
                       (end_scales, g["endpoint_scales"], "endpoint scales"), (faces, g["faces"], "faces"),
                       (ids, g["ids"], "ids")):
        a = np.asarray(a)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_reference(name):
    g = golden_case(name)
    out = TR.marching_tetrahedra(g["vertices"][None], g["tets"].astype(np.int64), g["sdf"][None], g["scales"][None, :, None])
    assert_same([o[0] for o in out], g)


def test_golden_covers_the_cases():
    g = {n: golden_case(n) for n in CASES}
    assert len(g["doc"]["ids"]) == 4 and len(g["qhull"]["faces"]) > 1000
    assert len(g["inside"]["ids"]) == 0 and len(g["outside"]["ids"]) == 0
    assert (g["zeros"]["sdf"] == 0).any() and np.isnan(g["zeros"]["sdf"]).any() and len(g["zeros"]["faces"]) > 0


def test_bisection_and_filter():
    lp = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    rp = np.array([[1, 0, 0], [2, 0, 0], [4, 0, 0]], np.float32)
    ls = np.array([[1], [-1], [1]], np.float32)
    rs = -ls
    TR.bisection_step(lp, rp, ls, rs, np.array([0.5, 0.0, -0.5], np.float32))
    assert lp[:, 0].tolist() == [0.5, 0, 0] and rp[:, 0].tolist() == [1, 1, 2]   # mid == 0 moves the right end
    v, f = TR.filter_mesh(np.arange(12, dtype=np.float32).reshape(4, 3), np.array([[0, 1, 2], [1, 2, 3]]),
                          np.array([True, False, True, True]))
    assert v.shape == (3, 3) and f.tolist() == []
    v, f = TR.filter_mesh(np.arange(12, dtype=np.float32).reshape(4, 3), np.array([[0, 2, 3], [1, 2, 3]]),
                          np.array([True, False, True, True]))
    assert f.tolist() == [[0, 1, 2]]
