"""Mesh extraction on the GPU: marching tetrahedra in HIP (csrc/tetmesh.hip) against the reference's own outputs
(tests/golden/tetmesh_reference.npz) and the numpy oracle; the view cache (ed3dgs_integrate_view_prepare / _probe)
against gaussian_renderer.integrate; the whole pipeline against the same glue driven by integrate per view per pass and
the oracle's marching tetrahedra.  All comparisons bit for bit."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tetmesh_ref as TR
from test_tetmesh_cpu import CASES, assert_same, golden_case

pytestmark = pytest.mark.gpu
ITER, NDE = 20000, 30


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected without a GPU")


def hip_mt(v, t, s, sc):
    from ed3dgs_amd.tetmesh import marching_tetrahedra
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = marching_tetrahedra(d(v)[None], d(t), d(s)[None], d(sc)[None])
    (e, es), esc, f, i = (x[0] for x in out)
    return (e.cpu().numpy(), es.cpu().numpy()), esc.cpu().numpy(), f.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
@pytest.mark.parametrize("name", CASES)
def test_hip_marching_tetrahedra_equals_reference(name, dtype):
    _need_gpu()
    g = golden_case(name)
    assert_same(hip_mt(g["vertices"], g["tets"].astype(dtype), g["sdf"], g["scales"][:, None]), g)


def grid(n, dev):
    """(n+1)^3 lattice vertices, 6 n^3 Freudenthal tets (each cube split along its main diagonal), built on the device."""
    r = torch.arange(n + 1, device=dev)
    X, Y, Z = torch.meshgrid(r, r, r, indexing="ij")
    verts = torch.stack([X, Y, Z], -1).reshape(-1, 3).float()
    c = torch.arange(n, device=dev)
    I, J, K = (a.reshape(-1) for a in torch.meshgrid(c, c, c, indexing="ij"))
    idx = lambda i, j, k: (i * (n + 1) + j) * (n + 1) + k
    steps = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    tets = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        cur = [I, J, K]
        vs = [idx(*cur)]
        for ax in p:
            cur = [cur[q] + steps[ax][q] for q in range(3)]
            vs.append(idx(*cur))
        tets.append(torch.stack(vs, 1))
    return verts, torch.stack(tets, 1).reshape(-1, 4)


def test_hip_marching_tetrahedra_large_grid_equals_oracle():
    _need_gpu()
    n = 120
    verts, tets = grid(n, "cuda")
    assert tets.shape[0] >= 10_000_000
    c = n / 2.0
    sdf = ((0.35 * n) ** 2 - ((verts - c) ** 2).sum(1)).contiguous()          # integer lattice: exact zeros occur
    assert (sdf == 0).any()
    sc = torch.rand(verts.shape[0], generator=torch.Generator().manual_seed(0)).cuda()
    got = hip_mt(verts.cpu().numpy(), tets.cpu().numpy(), sdf.cpu().numpy(), sc.cpu().numpy())
    want = TR.marching_tetrahedra(verts.cpu().numpy()[None], tets.cpu().numpy(), sdf.cpu().numpy()[None], sc.cpu().numpy()[None])
    g = dict(zip(("endpoints", "endpoint_sdf", "endpoint_scales", "faces", "ids"),
                 (want[0][0][0], want[0][0][1], want[1][0], want[2][0], want[3][0])))
    assert len(g["faces"]) > 100000
    assert_same(got, g)
    # every tet valid: a checkerboard sdf puts two corners of each Freudenthal tet inside
    m = 20
    v2, t2 = grid(m, "cuda")
    chk = ((v2.sum(1).long() % 2) * 2 - 1).float()
    sc2 = torch.ones(v2.shape[0], device="cuda")
    got = hip_mt(v2.cpu().numpy(), t2.int().cpu().numpy(), chk.cpu().numpy(), sc2.cpu().numpy())
    assert len(got[2]) == 2 * t2.shape[0]
    want = TR.marching_tetrahedra(v2.cpu().numpy()[None], t2.cpu().numpy(), chk.cpu().numpy()[None], sc2.cpu().numpy()[None])
    assert_same(got, dict(zip(("endpoints", "endpoint_sdf", "endpoint_scales", "faces", "ids"),
                              (want[0][0][0], want[0][0][1], want[1][0], want[2][0], want[3][0]))))


def test_hip_marching_tetrahedra_empty_and_bad_index():
    _need_gpu()
    v = np.zeros((4, 3), np.float32)
    (e, es), esc, f, i = hip_mt(v, np.array([[0, 1, 2, 3]]), -np.ones(4, np.float32), np.ones(4, np.float32))
    assert e.shape == (0, 2, 3) and es.shape == (0, 2, 1) and esc.shape == (0, 2, 1) and f.shape == (0, 3) and i.shape == (0, 2)
    with pytest.raises(RuntimeError, match="outside"):
        hip_mt(v, np.array([[0, 1, 2, 4]]), np.ones(4, np.float32), np.ones(4, np.float32))


# ---- the view cache and the pipeline ----

def _model(P, seed=0):
    from ed3dgs_amd import synthetic as S
    from ed3dgs_amd.model import SynthGaussianModel, default_hyper
    return SynthGaussianModel(S.make_scene(P, seed=seed), args=default_hyper(), device="cuda")


def _pipe(cov3d):
    return SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=cov3d, debug=False)


@pytest.mark.parametrize("cov3d", [False, True], ids=["scale-rot", "cov3D-python"])
def test_view_cache_equals_integrate(cov3d):
    _need_gpu()
    from ed3dgs_amd import mesh as M
    from ed3dgs_amd import synthetic as S
    from gaussian_renderer import integrate
    model = _model(3000)
    views = [c.with_time(0.25) for c in S.make_cameras(3, 160, 112, seed=4, device="cuda")]
    bg = torch.ones(3, device="cuda")
    pipe = _pipe(cov3d)
    cached = M.prepare_views(views, model, pipe, bg, 0.0, ITER, NDE, NDE)
    g = torch.Generator().manual_seed(9)
    sets = [(torch.rand(4000, 3, generator=g) * 2.4 - 1.2).cuda(), (torch.rand(2500, 3, generator=g) * 3 - 1.5).cuda()]
    for pts in sets:
        for view, cv in zip(views, cached):
            ref = integrate(pts, view, model, pipe, bg, 0.0, ITER, num_down_emb_c=NDE, num_down_emb_f=NDE)
            alpha, color, coord, sdf = cv.probe(pts)
            for a, b, what in ((alpha, ref["alpha_integrated"], "alpha"), (color, ref["color_integrated"], "color"),
                               (coord, ref["point_coordinate"], "coordinate"), (sdf, ref["point_sdf"], "sdf"),
                               (cv.render[:8], ref["render"][:8], "render[0:8]")):
                assert torch.equal(a, b), what
            assert (alpha < 1).any()
    assert cached[0].nbytes > 0


def _reference_shaped(views, model, pipe, bg, masks):
    from ed3dgs_amd import mesh as M
    from gaussian_renderer import integrate

    def evaluate(points):
        probes = []
        for cam_id, view in enumerate(views):
            ret = integrate(points, view, model, pipe, bg, 0.0, ITER, num_down_emb_c=NDE, num_down_emb_f=NDE)
            mask = ret["render"][7][None]
            if masks is not None:
                mask = mask * masks[cam_id]
            probes.append((ret["alpha_integrated"], ret["point_coordinate"], mask.type(torch.float32), view.image_width,
                           view.image_height))
        return M.cull_alpha_from_probes(points, probes)
    return evaluate


def oracle_marching(vertices, tets, sdf, scales):
    n = lambda t: t.detach().cpu().numpy()
    out = TR.marching_tetrahedra(n(vertices), n(tets), n(sdf), n(scales))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return [tuple((t(v[0]), t(v[1])) for v in out[0]), tuple(t(a) for a in out[1]), tuple(t(a) for a in out[2]),
            tuple(t(a) for a in out[3])]


@pytest.mark.parametrize("with_masks", [False, True], ids=["no-masks", "masks"])
def test_pipeline_equals_reference_shaped(with_masks, tmp_path):
    _need_gpu()
    from ed3dgs_amd import mesh as M
    from ed3dgs_amd import ply
    from ed3dgs_amd import synthetic as S
    model = _model(3000, seed=1)
    views = [c.with_time(0.0) for c in S.make_cameras(4, 128, 96, seed=2, device="cuda")]
    bg = torch.zeros(3, device="cuda")
    pipe = _pipe(False)
    masks = None
    if with_masks:
        yy, xx = torch.meshgrid(torch.arange(96.), torch.arange(128.), indexing="ij")
        masks = [((xx - 64 - 5 * k) ** 2 + (yy - 48) ** 2 < 40 ** 2).float()[None].cuda() for k in range(4)]
    kw = dict(num_down_emb_c=NDE, num_down_emb_f=NDE, masks=masks)
    v, f = M.marching_tetrahedra_with_binary_search("", "test", ITER, views, model, pipe, bg, 0.0, str(tmp_path / "a"), 0, ITER, **kw)
    v2, f2 = M.marching_tetrahedra_with_binary_search("", "test", ITER, views, model, pipe, bg, 0.0, str(tmp_path / "b"), 0, ITER,
                                                      evaluate=_reference_shaped(views, model, pipe, bg, masks),
                                                      marching=oracle_marching, **kw)
    assert len(f) > 100, len(f)
    assert torch.equal(v.cpu(), v2.cpu()) and torch.equal(f.cpu(), f2.cpu())
    rv, rf = ply.read_mesh(str(tmp_path / "a" / "recon.ply"))
    assert np.array_equal(rv, v.cpu().numpy()) and np.array_equal(rf, f.cpu().numpy())


def test_outlier_filter_against_kdtree():
    _need_gpu()
    from ed3dgs_amd import mesh as M
    from test_mesh_cpu import kdtree_keep
    x = np.random.default_rng(7).normal(size=(20000, 3)).astype(np.float32)
    want, avg_k, thr = kdtree_keep(x)
    avg = M.outlier_average_distance(torch.from_numpy(x).cuda())
    got = M.statistical_outlier_mask(avg).cpu().numpy()
    diff = np.nonzero(got != want)[0]
    near = np.abs(avg_k[diff] - thr) <= 1e-6 * thr
    print("outlier filter: %d differing keep decisions, all within 1e-6 of the threshold: %s" % (len(diff), bool(near.all())))
    assert near.all()
    assert np.abs(avg.cpu().numpy() - avg_k).max() <= 1e-12 * avg_k.max()


def test_sphere_geometry():
    """Flat Gaussians tangent to the unit sphere (discs of 0.02 x 0.02 x 0.003, normal along the radius), deformation
    outputs zeroed, 8 views: at least 95 % of the mesh vertices lie within 0.05 of the sphere."""
    _need_gpu()
    from ed3dgs_amd import mesh as M
    from ed3dgs_amd import synthetic as S
    P = 20000
    model = _model(P, seed=3)
    i = torch.arange(P, dtype=torch.float64) + 0.5
    phi, th = torch.acos(1 - 2 * i / P), np.pi * (1 + 5 ** 0.5) * i
    n = torch.stack([torch.cos(th) * torch.sin(phi), torch.sin(th) * torch.sin(phi), torch.cos(phi)], 1)
    q = torch.stack([1 + n[:, 2], -n[:, 1], n[:, 0], torch.zeros(P, dtype=torch.float64)], 1)   # rotates z onto n
    with torch.no_grad():
        model._xyz.copy_(n.float().cuda())
        model._rotation.copy_((q / q.norm(dim=1, keepdim=True)).float().cuda())
        model._scaling.copy_(torch.log(torch.tensor([0.02, 0.02, 0.003])).expand(P, 3).cuda())
        model._opacity.fill_(4.0)
    model._deformation = lambda xyz, s, r, o, t, cam, pc, _n, shs, **kw: (xyz, s, r, o, shs, None)
    views = [c.with_time(0.0) for c in S.make_cameras(8, 256, 192, seed=5, device="cuda")]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        v, f = M.marching_tetrahedra_with_binary_search("", "sphere", ITER, views, model, _pipe(False),
                                                        torch.zeros(3, device="cuda"), 0.0, d, 0, ITER,
                                                        num_down_emb_c=NDE, num_down_emb_f=NDE)
    r = v.norm(dim=1)
    frac = float(((r - 1).abs() <= 0.05).float().mean())
    print("sphere: %d vertices, %d faces, fraction within 0.05 of the sphere %.4f, median |r - 1| %.4f"
          % (len(v), len(f), frac, float((r - 1).abs().median())))
    assert len(f) > 1000 and frac >= 0.95
