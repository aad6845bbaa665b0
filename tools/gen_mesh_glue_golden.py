"""tools/gen_mesh_glue_golden.py -- tests/golden/mesh_glue_reference.npz from the REFERENCE's own mesh-extraction glue.

Runs mesh_extract_tetrahedra.py:marching_tetrahedra_with_binary_search and utils/mesh_extraction_utils.py:get_tetra_points
(container only: needs /root/reference) on the CPU, with its real utils/tetmesh.py and utils/general_utils.py, and
recording stand-ins for its native or heavy neighbours: `cv2`, `trimesh` (creation.box, Trimesh, update_vertices /
update_faces / export), `open3d` (the statistical outlier filter returns tests/support/mesh_probe.keep_indices),
`tetranerf` (cpp.triangulate = scipy Delaunay), `scene`, `arguments` and `gaussian_renderer` (integrate = the analytic
stand-in of tests/support/mesh_probe.py).  Records the tetra points and their scales, the cells, the points of every
evaluation (the first pass and the 8 midpoint sets), the vertices and faces handed to Trimesh, the two masks and the
deformation call.  tests/test_mesh_glue_cpu.py runs ed3dgs_amd.mesh the same way and compares bit for bit.  Only data is
written."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import gen_raster_golden as G  # noqa: E402
import mesh_probe as MP  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mesh_glue_reference.npz")
REC = {}


def stub_modules(recorder):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class Trimesh:
        def __init__(self, vertices=None, faces=None, process=True):
            REC["trimesh_vertices"], REC["trimesh_faces"] = np.array(vertices), np.array(faces)
            REC["trimesh_process"] = np.array(process)

        def update_vertices(self, mask):
            REC["vertex_mask"] = np.array(mask)

        def update_faces(self, mask):
            REC["face_mask"] = np.array(mask)

        def export(self, path):
            REC["export_name"] = np.array(os.path.basename(path))

    box = lambda: types.SimpleNamespace(vertices=np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)]))
    mod("trimesh", Trimesh=Trimesh, creation=types.SimpleNamespace(box=box))

    class PointCloud:
        points = None

        def remove_statistical_outlier(self, nb_neighbors, std_ratio):
            REC["outlier_args"] = np.array([nb_neighbors, std_ratio])
            return None, MP.keep_indices(len(self.points))

    mod("open3d", geometry=types.SimpleNamespace(PointCloud=PointCloud), utility=types.SimpleNamespace(Vector3dVector=np.asarray))

    def triangulate(points):
        REC["tetra_points_in"] = points.numpy().copy()
        cells = Delaunay(points.double().numpy()).simplices.astype(np.int32)
        REC["cells"] = cells.astype(np.int64)
        return torch.from_numpy(cells)

    mod("tetranerf"); mod("tetranerf.utils")
    mod("tetranerf.utils.extension", cpp=types.SimpleNamespace(triangulate=triangulate))
    mod("cv2")
    mod("scene", Scene=object)
    mod("arguments", ModelParams=object, PipelineParams=object, get_combined_args=None, ModelHiddenParams=object,
        OptimizationParams=object)
    mod("gaussian_renderer", render=None, integrate=recorder.integrate, GaussianModel=object)
    mod("utils.extra_utils", o3d_knn=None)


def main():
    G.load_reference_utils()                       # utils.general_utils (build_rotation) with the device-dropping torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    rec = MP.Recorder()
    stub_modules(rec)
    G._load("utils.tetmesh", "utils/tetmesh.py")
    meu = G._load("utils.mesh_extraction_utils", "utils/mesh_extraction_utils.py")
    spec = importlib.util.spec_from_file_location("ref_mesh_extract", os.path.join(G.REF, "mesh_extract_tetrahedra.py"))
    mx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mx)
    mx.torch = G._TorchCpu()
    mx.hyperparam = types.SimpleNamespace(min_embeddings=MP.MIN_EMB)
    mx.tqdm = lambda it, **k: it

    gaussians, views = MP.Gaussians(), MP.make_views()
    rec.first_view = views[0]
    orig = meu.get_tetra_points

    def get_tetra_points(**kw):
        pts, sc = orig(**kw)
        REC["tetra_points"], REC["tetra_scales"] = pts.numpy().copy(), sc.numpy().copy()
        return pts, sc
    mx.get_tetra_points = get_tetra_points
    with tempfile.TemporaryDirectory() as d:
        mx.marching_tetrahedra_with_binary_search("model", "test", MP.LOADED_ITER, views, gaussians, None,
                                                  torch.zeros(3), 0.0, d, MP.TIMESTEP, MP.LOADED_ITER)
    assert len(rec.eval_points) == 9 and len(gaussians._deformation.calls) == 1
    c = gaussians._deformation.calls[0]
    REC["deform_call"] = np.array([c["time"], -1 if c["cam_no"] is None else c["cam_no"], c["iter"], c["num_down_emb_c"],
                                   c["num_down_emb_f"], c["n"]], np.float64)
    for i, p in enumerate(rec.eval_points):
        REC["eval_points_%d" % i] = p
    assert np.array_equal(REC["tetra_points_in"], REC["tetra_points"])
    np.savez_compressed(OUT, **REC)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(REC["trimesh_vertices"]), "vertices,", len(REC["trimesh_faces"]),
          "faces,", int(REC["vertex_mask"].sum()), "kept")


if __name__ == "__main__":
    main()
