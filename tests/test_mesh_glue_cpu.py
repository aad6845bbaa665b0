"""ed3dgs_amd.mesh's pipeline glue against the REFERENCE's own mesh_extract_tetrahedra.py / utils/mesh_extraction_utils.py
(tests/golden/mesh_glue_reference.npz, tools/gen_mesh_glue_golden.py).  Both run with the stand-ins of
tests/support/mesh_probe.py (analytic integrate, recording deformation, the same outlier choice) on the CPU; this side
uses the view-cache glue (prepare -> view_mask -> evaluate_cull_alpha) and oracle/tetmesh_ref.py's marching tetrahedra.
Bit for bit: the deformation call, the tetra points and scales, the cells, the points of all 9 evaluations, the
vertices and faces before the filter, both masks, and the final mesh."""
import os
import sys

import numpy as np
import torch

from ed3dgs_amd import mesh as M
from ed3dgs_amd import ply
from oracle import tetmesh_ref as TR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "support"))
import mesh_probe as MP  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_glue_reference.npz")


def oracle_marching(vertices, tets, sdf, scales):
    out = TR.marching_tetrahedra(vertices.numpy(), tets.numpy(), sdf.numpy(), scales.numpy())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return [tuple((t(v[0]), t(v[1])) for v in out[0]), tuple(t(a) for a in out[1]), tuple(t(a) for a in out[2]),
            tuple(t(a) for a in out[3])]


def run_glue(tmp_path, monkeypatch):
    rec = MP.Recorder()
    got = {}
    gaussians, views = MP.Gaussians(), MP.make_views()

    def prepare(vs):
        return [M.CachedView(MP.AnalyticView(v, rec, i == 0), v.image_width, v.image_height,
                             M.view_mask(MP.analytic(torch.zeros(0, 3), v)[2][7], v, None)) for i, v in enumerate(vs)]

    tri = M.triangulate

    def triangulate(points):
        got["tetra_points"] = points.numpy().copy()
        cells = tri(points)
        got["cells"] = cells.numpy().copy()
        return cells

    filt = M.filter_mesh

    def filter_mesh(points, faces, keep):
        got["trimesh_vertices"], got["trimesh_faces"], got["vertex_mask"] = points.numpy().copy(), faces.numpy().copy(), keep.numpy().copy()
        got["face_mask"] = keep[faces].all(dim=1).numpy()
        return filt(points, faces, keep)

    orig_tp = M.get_tetra_points

    def get_tetra_points(*a, **k):
        pts, sc = orig_tp(*a, **k)
        got["tetra_scales"] = sc.numpy().copy()
        return pts, sc

    monkeypatch.setattr(M, "triangulate", triangulate)
    monkeypatch.setattr(M, "filter_mesh", filter_mesh)
    monkeypatch.setattr(M, "get_tetra_points", get_tetra_points)
    keep = torch.zeros(MP.K_GAUSSIANS, dtype=torch.bool)
    keep[torch.from_numpy(MP.keep_indices(MP.K_GAUSSIANS))] = True
    v, f = M.marching_tetrahedra_with_binary_search("model", "test", MP.LOADED_ITER, views, gaussians, None, torch.zeros(3),
                                                    0.0, str(tmp_path), MP.TIMESTEP, MP.LOADED_ITER,
                                                    num_down_emb_c=MP.MIN_EMB, num_down_emb_f=MP.MIN_EMB, keep=keep,
                                                    prepare=prepare, marching=oracle_marching)
    return got, rec, gaussians, v, f


def test_glue_equals_reference(tmp_path, monkeypatch):
    g = np.load(GOLD)
    got, rec, gaussians, v, f = run_glue(tmp_path, monkeypatch)
    c = gaussians._deformation.calls
    assert len(c) == 1
    assert [c[0]["time"], -1 if c[0]["cam_no"] is None else c[0]["cam_no"], c[0]["iter"], c[0]["num_down_emb_c"],
            c[0]["num_down_emb_f"], c[0]["n"]] == g["deform_call"].tolist()
    assert g["outlier_args"].tolist() == [20, 1.0]
    for k in ("tetra_points", "tetra_scales", "cells", "trimesh_vertices", "trimesh_faces", "vertex_mask", "face_mask"):
        a, b = np.asarray(got[k]), g[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(a.astype(b.dtype), b) and (a.dtype.kind == b.dtype.kind), k
        if a.dtype.kind == "f":
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert len(rec.eval_points) == 9
    for i, p in enumerate(rec.eval_points):
        assert p.dtype == g["eval_points_%d" % i].dtype and np.array_equal(p.view(np.uint8), g["eval_points_%d" % i].view(np.uint8)), i
    # both filters bite, and the final mesh is their net effect
    assert 0 < g["vertex_mask"].sum() < len(g["vertex_mask"]) and 0 < g["face_mask"].sum() < len(g["face_mask"])
    ev, ef = TR.filter_mesh(g["trimesh_vertices"], g["trimesh_faces"], g["vertex_mask"])
    assert np.array_equal(v.numpy(), ev) and np.array_equal(f.numpy(), ef)
    rv, rf = ply.read_mesh(str(tmp_path / "recon.ply"))
    assert np.array_equal(rv, ev) and np.array_equal(rf, ef)


def test_glue_fixture_exercises_the_masks():
    """The gt_alpha_mask (float64) view and the disc masks must decide some points, or the fixture pins nothing there."""
    views = MP.make_views()
    assert views[1].gt_alpha_mask.dtype == torch.float64 and (views[1].gt_alpha_mask < 1).any()
    m = M.view_mask(MP.analytic(torch.zeros(0, 3), views[1])[2][7], views[1], None)
    assert m.dtype == torch.float32 and len(torch.unique(m)) == 3   # 0, 0.875, 0.875 * 0.25
