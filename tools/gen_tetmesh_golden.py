"""tools/gen_tetmesh_golden.py -- tests/golden/tetmesh_reference.npz from the REFERENCE's own utils/tetmesh.py.

The reference's marching tetrahedra (adapted from kaolin) imports only torch, so this script (container only: needs
/root/reference) loads the file by path and runs `marching_tetrahedra` on the CPU -- where mesh_extract_tetrahedra.py:96-97
runs it too -- over five cases, and stores inputs and outputs:
  doc      -- the docstring's single tet (two vertices inside);
  qhull    -- scipy Delaunay cells of 2000 random points, sphere sdf;
  inside   -- every vertex inside (no valid tet, E = 0);
  outside  -- every vertex outside (E = 0);
  zeros    -- an sdf quantised to {-1, -0.5, 0, 0.5, 1} with NaNs: 0 and NaN count as outside.
tests/test_tetmesh_cpu.py compares oracle/tetmesh_ref.py with it, tests/test_mesh_gpu.py the HIP kernel; bit for bit.
Only data is written."""
import importlib.util
import os

import numpy as np
import torch
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "tetmesh_reference.npz")


def load_reference_tetmesh():
    spec = importlib.util.spec_from_file_location("ref_tetmesh", os.path.join(REF, "utils", "tetmesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(11)
    out = {}
    out["doc"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 1, 2, 3]], np.int64),
                  np.array([-1, -1, 0.5, 0.5], np.float32), np.array([0.1, 0.2, 0.3, 0.4], np.float32))
    pts = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    cells = Delaunay(pts.astype(np.float64)).simplices.astype(np.int64)
    out["qhull"] = (pts, cells, (0.6 - np.linalg.norm(pts, axis=1)).astype(np.float32),
                    rng.uniform(0.01, 0.1, 2000).astype(np.float32))
    small = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    scells = Delaunay(small.astype(np.float64)).simplices.astype(np.int64)
    sscale = rng.uniform(0.01, 0.1, 300).astype(np.float32)
    out["inside"] = (small, scells, rng.uniform(0.1, 1, 300).astype(np.float32), sscale)
    out["outside"] = (small, scells, -rng.uniform(0.0, 1, 300).astype(np.float32), sscale)
    q = (np.round(2 * (0.5 - np.linalg.norm(small, axis=1)) * 2) / 2).clip(-1, 1).astype(np.float32)
    q[rng.choice(300, 6, replace=False)] = np.nan
    out["zeros"] = (small, scells, q, sscale)
    return out


def main():
    ref = load_reference_tetmesh()
    data = {}
    for name, (v, t, s, sc) in cases().items():
        verts, scales, faces, ids = ref.marching_tetrahedra(torch.from_numpy(v)[None], torch.from_numpy(t),
                                                            torch.from_numpy(s)[None], torch.from_numpy(sc)[:, None][None])
        data.update({f"{name}/vertices": v, f"{name}/tets": t.astype(np.int32), f"{name}/sdf": s, f"{name}/scales": sc,
                     f"{name}/endpoints": verts[0][0].numpy(), f"{name}/endpoint_sdf": verts[0][1].numpy(),
                     f"{name}/endpoint_scales": scales[0].numpy(), f"{name}/faces": faces[0].numpy(),
                     f"{name}/ids": ids[0].numpy()})
        print(name, "tets", len(t), "E", len(ids[0]), "F", len(faces[0]), faces[0].dtype, ids[0].dtype)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
