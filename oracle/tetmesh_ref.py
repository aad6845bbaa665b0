"""Marching tetrahedra and the mesh-extraction glue in numpy: the test oracle of e-d3dgs_amd/csrc/tetmesh.hip and
ed3dgs_amd/mesh.py (utils/tetmesh.py, mesh_extract_tetrahedra.py:93-139).  Test use only; no torch, no GPU.

marching_tetrahedra(vertices [B,N,3], tets [T,4], sdf [B,N], scales [B,N(,1)]) -> list of
((endpoints [E,2,3], endpoint sdf [E,2,1]), endpoint scales [E,2,1], faces [F,3] int64, edge ids [E,2] int64) per batch
entry, as the reference's zip(*...) returns them.  A vertex is inside when sdf > 0; a tet is valid when 1-3 of its
vertices are inside; output vertex k is the k-th crossing edge in lexicographic (min, max) order; faces are the
one-triangle tets in tet order, then the two-triangle tets in tet order.  The order is the unchunked one (the reference
emits faces chunk by chunk above 32 Mi tets)."""
import numpy as np

# corner pairs of the six edges, and per case (sum of inside_i << i) the edges the triangles join
EDGE_CORNERS = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], np.int64)
TRIANGLES = np.array([
    [-1, -1, -1, -1, -1, -1], [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4],
    [3, 1, 5, -1, -1, -1], [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1],
    [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1], [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1],
    [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1], [-1, -1, -1, -1, -1, -1]], np.int64)


def _one(vertices, tets, sdf, scales):
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    sdf = np.asarray(sdf, np.float32).reshape(-1)
    scales = np.asarray(scales, np.float32).reshape(-1)
    tets = np.asarray(tets).astype(np.int64).reshape(-1, 4)
    N = sdf.shape[0]
    with np.errstate(invalid="ignore"):
        inside = sdf > 0
    occ = inside[tets]                                             # [T,4]
    n_in = occ.sum(1)
    case = (occ * np.array([1, 2, 4, 8])).sum(1)
    valid = (n_in > 0) & (n_in < 4)
    a, b = tets[:, EDGE_CORNERS[:, 0]], tets[:, EDGE_CORNERS[:, 1]]
    cross = (occ[:, EDGE_CORNERS[:, 0]] != occ[:, EDGE_CORNERS[:, 1]]) & valid[:, None]   # [T,6]
    lo, hi = np.minimum(a, b)[cross], np.maximum(a, b)[cross]
    key = lo * max(N, 1) + hi                                      # lexicographic (lo, hi) as one integer
    ukey, inv = np.unique(key, return_inverse=True)
    ids = np.stack([ukey // max(N, 1), ukey % max(N, 1)], 1).astype(np.int64).reshape(-1, 2)
    vid = np.full(cross.shape, -1, np.int64)
    vid[cross] = inv.reshape(-1)
    faces = []
    for ntri in (1, 2):
        sel = np.nonzero(valid & (np.where(n_in == 2, 2, 1) == ntri))[0]
        corners = TRIANGLES[case[sel], :3 * ntri]
        faces.append(np.take_along_axis(vid[sel], corners, 1).reshape(-1, 3))
    faces = np.concatenate(faces, 0).astype(np.int64)
    flat = ids.reshape(-1)
    return ((vertices[flat].reshape(-1, 2, 3), sdf[flat].reshape(-1, 2, 1)), scales[flat].reshape(-1, 2, 1), faces, ids)


def marching_tetrahedra(vertices, tets, sdf, scales):
    return list(zip(*[_one(vertices[i], tets, sdf[i], scales[i]) for i in range(len(vertices))]))


# ---- the glue of mesh_extract_tetrahedra.py:132-139 after marching tetrahedra ----

def bisection_step(left_points, right_points, left_sdf, right_sdf, mid_sdf):
    """One step of :117-127 in place: mid == 0 moves the right end.  *_sdf are [E,1], mid_sdf [E]."""
    mid_points = (left_points + right_points) / np.float32(2)
    mid = mid_sdf.reshape(-1, 1)
    low = ((mid < 0) & (left_sdf < 0)) | ((mid > 0) & (left_sdf > 0))
    left_sdf[low] = mid[low]
    right_sdf[~low] = mid[~low]
    lf = low.reshape(-1)
    left_points[lf] = mid_points[lf]
    right_points[~lf] = mid_points[~lf]


def filter_mesh(points, faces, keep):
    """trimesh's update_vertices(keep) then update_faces(all three corners kept), net: kept vertices renumbered by prefix
    count, faces with a dropped corner removed."""
    keep = np.asarray(keep, bool)
    remap = np.cumsum(keep) - 1
    fk = keep[faces].all(1)
    return points[keep], remap[faces[fk]].astype(np.int64)
