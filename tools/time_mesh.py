"""tools/time_mesh.py -- one timestep of tetrahedral mesh extraction, timed per phase (GPU; separate from bench.py).

Workload (defaults): 200k synthetic Gaussians, 16 views at 1100 x 1604, one timestep.  Phases of
ed3dgs_amd.mesh.marching_tetrahedra_with_binary_search: deformation, tetra points + outlier filter, qhull (CPU), the
view prepares, the 9 x V probes (with their cull-alpha glue), marching tetrahedra (HIP), the bisection glue and the
filter + PLY write; plus the bytes one cached view keeps.  In the same process the reference-shaped path
(gaussian_renderer.integrate per view per pass, the numpy oracle's marching tetrahedra) runs, alternating with the
cached path `--rounds` times (the first round of each path includes process warm-up; the medians over rounds are
reported); the meshes must be identical.  The reference-shaped marching tetrahedra is a torch restatement of the
oracle's on the GPU (`torch.unique` over all valid tets' edges, as utils/tetmesh.py does).  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "e-d3dgs_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ITER, NDE = 20000, 30
EDGES = torch.tensor([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])

def torch_marching(vertices, tets, sdf, scales):
    """utils/tetmesh.py's algorithm in torch on the device (one batch entry): unique over every edge of the valid tets."""
    from oracle.tetmesh_ref import TRIANGLES as TT
    dev = vertices.device
    v, s, sc, t = vertices[0], sdf[0], scales[0].reshape(-1), tets.long()
    occ = s > 0
    o4 = occ[t]
    n = o4.sum(1)
    valid = (n > 0) & (n < 4)
    e = t[valid][:, EDGES.to(dev)].reshape(-1, 2)
    e = torch.stack([e.min(1).values, e.max(1).values], 1)
    uniq, inv = torch.unique(e, dim=0, return_inverse=True)
    cross = occ[uniq].sum(1) == 1
    mapping = torch.full((uniq.shape[0],), -1, dtype=torch.long, device=dev)
    mapping[cross] = torch.arange(int(cross.sum()), device=dev)
    idx = mapping[inv].reshape(-1, 6)
    ids = uniq[cross]
    case = (o4[valid] * torch.tensor([1, 2, 4, 8], device=dev)).sum(1)
    ntri = torch.where(n[valid] == 2, 2, 1)
    tab = torch.from_numpy(TT).to(dev)
    faces = torch.cat([torch.gather(idx[ntri == 1], 1, tab[case[ntri == 1]][:, :3]).reshape(-1, 3),
                       torch.gather(idx[ntri == 2], 1, tab[case[ntri == 2]][:, :6]).reshape(-1, 3)], 0)
    flat = ids.reshape(-1)
    return [((v[flat].reshape(-1, 2, 3), s[flat].reshape(-1, 2, 1)),), (sc[flat].reshape(-1, 2, 1),), (faces,), (ids,)]


def model_and_views(P, n_views, W, H):
    from types import SimpleNamespace

    from ed3dgs_amd import synthetic as S
    from ed3dgs_amd.model import SynthGaussianModel, default_hyper
    model = SynthGaussianModel(S.make_scene(P, seed=0), args=default_hyper(), device="cuda")
    views = [c.with_time(0.0) for c in S.make_cameras(n_views, W, H, seed=1, device="cuda")]
    return model, views, SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)


def reference_shaped_evaluator(views, model, pipe, bg):
    """gaussian_renderer.integrate per view per pass (each call deforms, bins and runs the per-pixel pass again)."""
    from ed3dgs_amd import mesh as M
    from gaussian_renderer import integrate

    def evaluate(points):
        probes = []
        for view in views:
            ret = integrate(points, view, model, pipe, bg, 0.0, ITER, num_down_emb_c=NDE, num_down_emb_f=NDE)
            probes.append((ret["alpha_integrated"], ret["point_coordinate"], ret["render"][7][None].type(torch.float32),
                           view.image_width, view.image_height))
        return M.cull_alpha_from_probes(points, probes)
    return evaluate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200000)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--W", type=int, default=1100)
    ap.add_argument("--H", type=int, default=1604)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-reference", action="store_true")
    a = ap.parse_args()
    from ed3dgs_amd import mesh as M
    model, views, pipe = model_and_views(a.P, a.views, a.W, a.H)
    bg = torch.zeros(3, device="cuda")
    kw = dict(num_down_emb_c=NDE, num_down_emb_f=NDE)
    res = dict(P=a.P, views=a.views, W=a.W, H=a.H, cached=[], reference=[])
    ref_mesh = None
    with tempfile.TemporaryDirectory() as d:
        for _ in range(a.rounds):
            tm = {}
            t0 = time.perf_counter()
            v, f = M.marching_tetrahedra_with_binary_search("", "t", ITER, views, model, pipe, bg, 0.0, d, 0, ITER, timings=tm, **kw)
            tm["total"] = time.perf_counter() - t0
            tm.update(V=len(v), F=len(f))
            res["cached"].append(tm)
            print("cached", json.dumps(tm), file=sys.stderr, flush=True)
            if a.skip_reference:
                continue
            tr = {}
            t0 = time.perf_counter()
            v2, f2 = M.marching_tetrahedra_with_binary_search("", "t", ITER, views, model, pipe, bg, 0.0, d, 0, ITER, timings=tr,
                                                              evaluate=reference_shaped_evaluator(views, model, pipe, bg),
                                                              marching=torch_marching, **kw)
            tr["total"] = time.perf_counter() - t0
            res["reference"].append(tr)
            print("reference", json.dumps(tr), file=sys.stderr, flush=True)
            assert torch.equal(v.cpu(), v2.cpu()) and torch.equal(f.cpu(), f2.cpu()), "meshes differ"
            res["identical"] = True
    for path in ("cached", "reference"):
        if res[path]:
            res[path + "_median"] = {k: float(np.median([r[k] for r in res[path]])) for k in res[path][0]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
