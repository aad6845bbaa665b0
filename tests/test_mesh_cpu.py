"""Mesh-extraction glue on the CPU (ed3dgs_amd/mesh.py): PLY round trip, box corners of get_tetra_points, the outlier
rule against a scipy cKDTree float64 restatement, bisection and the trimesh-style filter against oracle/tetmesh_ref.py."""
import numpy as np
import torch
from scipy.spatial import cKDTree

from ed3dgs_amd import mesh as M
from ed3dgs_amd import ply
from oracle import tetmesh_ref as TR


def test_ply_round_trip(tmp_path):
    g = np.random.default_rng(0)
    v = g.normal(size=(57, 3)).astype(np.float32)
    f = g.integers(0, 57, (91, 3)).astype(np.int64)
    p = str(tmp_path / "recon.ply")
    M.write_mesh_ply(p, v, f)
    v2, f2 = ply.read_mesh(p)
    assert v2.dtype == np.float32 and f2.dtype == np.int64
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    M.write_mesh_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    v3, f3 = ply.read_mesh(p)
    assert v3.shape == (0, 3) and f3.shape == (0, 3)
    assert open(p, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\n")


def test_tetra_points_layout():
    g = torch.Generator().manual_seed(1)
    K = 6
    xyz, scale = torch.randn(K, 3, generator=g), torch.rand(K, 3, generator=g) + 0.1
    rot = torch.randn(K, 4, generator=g)
    keep = torch.tensor([True, False, True, True, True, False])
    pts, ps = M.get_tetra_points(rot, xyz, scale, keep=keep)
    k = int(keep.sum())
    assert pts.shape == (9 * k, 3) and ps.shape == (9 * k, 1)
    assert torch.equal(pts[8 * k:], xyz[keep])                       # centres after all corners
    R = M.build_rotation(rot[keep]).double()
    for i in range(k):                                              # Gaussian-major corners, x the slowest bit
        want = (R[i] @ (torch.from_numpy(M.BOX_CORNERS).T * 3 * scale[keep][i].double()[:, None])).T + xyz[keep][i].double()
        assert torch.allclose(pts[8 * i:8 * i + 8].double(), want, atol=1e-5)
        assert torch.all(ps[8 * i:8 * i + 8, 0] == (3 * scale[keep][i]).max())
    assert M.BOX_CORNERS[:2].tolist() == [[-1, -1, -1], [-1, -1, 1]] and M.BOX_CORNERS[4].tolist() == [1, -1, -1]


def kdtree_keep(x, k=20):
    d, _ = cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k)
    avg = d.mean(1)
    thr = avg.mean() + avg.std(ddof=1)
    return (avg > 0) & (avg < thr), avg, thr


def test_outlier_rule_against_kdtree():
    """statistical_outlier_mask on cKDTree averages (k = 20 with the point itself) is the same rule as a direct numpy
    restatement.  The k-NN side runs in tests/test_mesh_gpu.py."""
    x = np.random.default_rng(3).normal(size=(3000, 3))
    want, avg, thr = kdtree_keep(x)
    got = M.statistical_outlier_mask(torch.from_numpy(avg)).numpy()
    assert np.array_equal(got, want) and 0 < (~want).sum() < len(x)


def test_bisection_and_filter_match_oracle():
    g = np.random.default_rng(5)
    E = 400
    ends = g.normal(size=(E, 2, 3)).astype(np.float32)
    esdf = g.choice([-1.0, 0.5, 0.0], size=(E, 2, 1)).astype(np.float32)
    evals = [g.choice([-0.25, 0.0, 0.25], E).astype(np.float32) for _ in range(8)]
    calls = []

    def ev(p):
        calls.append(p.clone())
        return torch.from_numpy(evals[len(calls) - 1])

    pts = M.bisect_edges(torch.from_numpy(ends), torch.from_numpy(esdf), ev)
    lp, rp, ls, rs = ends[:, 0].copy(), ends[:, 1].copy(), esdf[:, 0].copy(), esdf[:, 1].copy()
    for i in range(8):
        assert np.array_equal(calls[i].numpy(), (lp + rp) / np.float32(2))
        TR.bisection_step(lp, rp, ls, rs, evals[i])
    assert np.array_equal(pts.numpy(), (lp + rp) / np.float32(2))
    faces = g.integers(0, E, (700, 3))
    keep = g.random(E) < 0.8
    v, f = M.filter_mesh(pts, torch.from_numpy(faces), torch.from_numpy(keep))
    v2, f2 = TR.filter_mesh(pts.numpy(), faces, keep)
    assert np.array_equal(v.numpy(), v2) and np.array_equal(f.numpy(), f2)


def test_cull_alpha_glue():
    """:38-62 on hand-made probes: normalisation, grid_sample validity, min and the -100 default."""
    pts = torch.zeros(3, 3)
    mask = torch.zeros(1, 4, 6)
    mask[0, :, :3] = 1
    coord = torch.tensor([[0.5, 1.5], [4.5, 1.5], [1.0, 2.0]])
    alpha = torch.tensor([0.2, 0.1, 0.9])
    out = M.cull_alpha_from_probes(pts, [(alpha, coord.clone(), mask, 6, 4)])
    assert out[1] == -100 and out[0] == torch.tensor(0.5) - torch.tensor(0.2) and out[2] == torch.tensor(0.5) - torch.tensor(0.9)
