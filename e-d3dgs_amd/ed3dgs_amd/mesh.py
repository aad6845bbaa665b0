"""Tetrahedral mesh extraction: mesh_extract_tetrahedra.py:37-139 and utils/mesh_extraction_utils.py:9-62 on the parts the
project has -- the integrate probe with a per-view cache (csrc/integrate.hip), exact k-NN (csrc/knn.hip) and marching
tetrahedra in HIP (csrc/tetmesh.hip).  Plain torch plumbing; one timestep per call.

get_tetra_points        -- 8 box corners per kept Gaussian, then the centres; per-point scale max(3 scale).  The
                           statistical outlier filter restates Open3D's remove_statistical_outlier(20, 1.0).
triangulate             -- scipy.spatial.Delaunay (qhull, CPU) in place of the CGAL/CUDA tetra_triangulation.
prepare_views           -- deform once per distinct view time, prepare every view once (IntegrateView).
evaluate_cull_alpha     -- evaluage_cull_alpha (:38-62) against prepared views.
marching_tetrahedra_with_binary_search -- :64-139, returns (vertices, faces) and writes recon.ply.
"""
import math
import os

import numpy as np
import torch

from . import knn as _knn

# trimesh.creation.box() vertex order (x the slowest bit), times 2: the corners of [-1, 1]^3.  Restated, not pinned
# (trimesh is not a dependency); the order only permutes the triangulation's input, not the mesh.
BOX_CORNERS = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])


def build_rotation(r):
    """utils/general_utils.py:81-101 (normalised quaternion -> rotation matrix), same expression order."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def outlier_average_distance(xyz, nb_neighbors=20):
    """Per point, the mean Euclidean distance (float64) to its nearest points INCLUDING itself, as Open3D's statistical
    outlier removal computes it: over nb_neighbors = 20 points, or over all of them in a cloud of fewer points (Open3D
    averages over the neighbours its search finds)."""
    if nb_neighbors != 20:
        raise ValueError("the k-NN kernel serves k = 20 (19 others + the point itself)")
    x = xyz.detach().float().contiguous()
    x64 = x.double()
    P = x.shape[0]
    if P <= nb_neighbors:   # every point is a neighbour of every point (the k-NN kernel needs K + 1 points)
        d = torch.linalg.vector_norm(x64[None, :, :] - x64[:, None, :], dim=-1)
        return d.sum(1) / P
    _, idx = _knn.knn_neighbours(x, 20)
    idx = idx[:, :nb_neighbors - 1]
    d = torch.linalg.vector_norm(x64[idx] - x64[:, None, :], dim=-1)   # [P, 19]
    return d.sum(1) / nb_neighbors                                      # + the point's own distance 0


def statistical_outlier_mask(avg, std_ratio=1.0):
    """Keep mask of Open3D's remove_statistical_outlier from the per-point averages.  As its source does: the sums run over
    the points with avg > 0, but both divisors count every point whose search found a neighbour (here: every point,
    the point itself is always found), the std with Bessel's correction; kept when 0 < avg < mean + std_ratio * std."""
    n = avg.shape[0]
    if n == 0:
        return avg > 0
    pos = avg > 0
    a = torch.where(pos, avg, torch.zeros_like(avg))
    mean = a.sum() / n
    sq = torch.where(pos, (avg - mean) ** 2, torch.zeros_like(avg)).sum()
    std = torch.sqrt(sq / (n - 1)) if n > 1 else torch.full_like(mean, float("nan"))   # Open3D divides by 0 here too
    return pos & (avg < mean + std_ratio * std)


@torch.no_grad()
def get_tetra_points(rotation_not_activated, xyz, scale_after_3D_filter, keep=None):
    """utils/mesh_extraction_utils.py:9-62: (points [9K,3], points_scale [9K,1]) of the K Gaussians the outlier filter
    keeps.  `keep` overrides the filter (a boolean mask; tests on the CPU, where the k-NN kernel does not run)."""
    rots = build_rotation(rotation_not_activated)
    scale = scale_after_3D_filter * 3.
    if keep is None:
        keep = statistical_outlier_mask(outlier_average_distance(xyz))
    xyz, scale, rots = xyz[keep], scale[keep], rots[keep]
    corners = torch.from_numpy(BOX_CORNERS.T.copy()).float().to(xyz.device).unsqueeze(0).repeat(xyz.shape[0], 1, 1)
    corners = corners * scale.unsqueeze(-1)
    vertices = torch.bmm(rots, corners).squeeze(-1) + xyz.unsqueeze(-1)
    vertices = vertices.permute(0, 2, 1).reshape(-1, 3).contiguous()
    vertices = torch.cat([vertices, xyz], dim=0)
    scale = scale.max(dim=-1, keepdim=True)[0]
    vertices_scale = torch.cat([scale.repeat(1, 8).reshape(-1, 1), scale], dim=0)
    return vertices, vertices_scale


def triangulate(points):
    """Delaunay cells [T,4] int64 on the points' device (qhull on the CPU).  Coplanar or duplicate points may end up in no
    cell; they then take no part in the mesh."""
    from scipy.spatial import Delaunay

    p = points.detach().cpu().double().numpy()
    cells = Delaunay(p).simplices.astype(np.int64)
    return torch.from_numpy(cells).to(points.device)


# ---- the per-view cache ----

class CachedView:
    """A prepared view (diff_gaussian_rasterization._C.IntegrateView, or anything with its `probe`, `out_color` and
    `nbytes`) with its size and cull mask."""

    def __init__(self, iv, width, height, mask):
        self.iv, self.width, self.height, self.mask = iv, width, height, mask

    @property
    def render(self):
        return self.iv.out_color

    @property
    def nbytes(self):
        return self.iv.nbytes + self.mask.numel() * self.mask.element_size()

    def probe(self, points):
        return self.iv.probe(points)


def _activated(pc, pipe, deformed, scaling_modifier):
    """What gaussian_renderer.integrate hands the rasterizer after the deformation (gaussian_renderer/__init__.py:601-653)."""
    means3D_final, scales_deformed, rotations_deformed, opacity_deformed, shs_final = deformed
    scales_final = rotations_final = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
        _, opacity_final = pc.apply_scaling_n_opacity_with_3D_filter(opacity=opacity_deformed, scales=scales_deformed)
    else:
        scales_final, opacity_final = pc.apply_scaling_n_opacity_with_3D_filter(opacity=opacity_deformed, scales=scales_deformed)
        rotations_final = pc.rotation_activation(rotations_deformed)
    return means3D_final, shs_final, opacity_final, scales_final, rotations_final, cov3D_precomp


def _deform(pc, time, loaded_iter, num_down_emb_c, num_down_emb_f):
    out = pc._deformation(pc.get_xyz, pc._scaling, pc._rotation, pc._opacity, float(time), None, pc, None, pc.get_features,
                          iter=loaded_iter, num_down_emb_c=num_down_emb_c, num_down_emb_f=num_down_emb_f)
    return out[:5]


def view_mask(render7, view, extra):
    mask = render7[None]
    gt = getattr(view, "gt_alpha_mask", None)
    if gt is not None:
        # the reference's mask is a float64 numpy array: the product is float64, cast back by .type(float32)
        mask = mask.double() * torch.as_tensor(gt).to(mask.device).double()
    if extra is not None:
        mask = mask * extra.to(mask.device)
    return mask.type(torch.float32).contiguous()


@torch.no_grad()
def prepare_views(views, pc, pipe, background, kernel_size, loaded_iter, num_down_emb_c, num_down_emb_f, masks=None,
                  scaling_modifier=1.0):
    """Deform once per distinct view time (integrate deforms at view.time with cam_no = None: every view of a timestep
    sees the same Gaussians), then prepare every view once.  kernel_size is unused by integrate (it passes 0.0)."""
    from diff_gaussian_rasterization import _C

    from gaussian_renderer import _eval_sh

    deformed = {}
    out = []
    for cam_id, view in enumerate(views):
        t = float(view.time)
        if t not in deformed:
            deformed[t] = _activated(pc, pipe, _deform(pc, t, loaded_iter, num_down_emb_c, num_down_emb_f), scaling_modifier)
        means3D, shs, opacity, scales, rotations, cov3D = deformed[t]
        dev = means3D.device
        colors = None
        if pipe.convert_SHs_python:
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - view.camera_center.to(dev).repeat(pc.get_features.shape[0], 1)
            colors = torch.clamp_min(_eval_sh()(pc.active_sh_degree, shs_view, dir_pp / dir_pp.norm(dim=1, keepdim=True)) + 0.5, 0.0)
            shs = None
        empty = torch.empty(0, device=dev)
        W, H = int(view.image_width), int(view.image_height)
        iv = _C.IntegrateView(background.to(dev), means3D, empty if colors is None else colors, opacity,
                              empty if scales is None else scales, empty if rotations is None else rotations,
                              scaling_modifier, empty if cov3D is None else cov3D, view.world_view_transform.to(dev),
                              view.full_proj_transform.to(dev), math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5), H, W,
                              empty if shs is None else shs, int(pc.active_sh_degree), view.camera_center.to(dev), False,
                              bool(pipe.debug))
        out.append(CachedView(iv, W, H, view_mask(iv.out_color[7], view, None if masks is None else masks[cam_id])))
    return out


def cull_alpha_from_probes(points, probes):
    """:38-62 given, per view, (alpha_integrated, point_coordinate, mask [1,H,W], W, H)."""
    final_sdf = torch.ones((points.shape[0]), dtype=torch.float32, device=points.device)
    weight = torch.zeros((points.shape[0]), dtype=torch.int32, device=points.device)
    for alpha_integrated, point_coordinate, mask, W, H in probes:
        point_coordinate[:, 0] = (point_coordinate[:, 0] * 2 + 1) / (W - 1) - 1
        point_coordinate[:, 1] = (point_coordinate[:, 1] * 2 + 1) / (H - 1) - 1
        prob = torch.nn.functional.grid_sample(mask[None], point_coordinate[None, None], padding_mode='zeros',
                                               align_corners=False)[0, 0, 0]
        valid = prob > 0.5
        final_sdf = torch.where(valid, torch.min(alpha_integrated, final_sdf), final_sdf)
        weight = torch.where(valid, weight + 1, weight)
    return torch.where(weight > 0, 0.5 - final_sdf, -100)


@torch.no_grad()
def evaluate_cull_alpha(points, cached_views, masks=None):
    """evaluage_cull_alpha (mesh_extract_tetrahedra.py:38-62) against prepared views.  `masks` (per-view [1,H,W] or None)
    multiplies the view masks fixed at prepare time."""
    def probes():
        for cam_id, cv in enumerate(cached_views):
            alpha, _, coord, _ = cv.probe(points)
            mask = cv.mask if masks is None else (cv.mask * masks[cam_id].to(cv.mask.device)).float()
            yield alpha, coord, mask, cv.width, cv.height
    return cull_alpha_from_probes(points, probes())


def bisect_edges(end_points, end_sdf, evaluate, n_binary_steps=8):
    """:106-127: returns the final midpoints [E,3]."""
    left_points, right_points = end_points[:, 0, :].clone(), end_points[:, 1, :].clone()
    left_sdf, right_sdf = end_sdf[:, 0, :].clone(), end_sdf[:, 1, :].clone()
    points = (left_points + right_points) / 2.
    for _ in range(n_binary_steps):
        mid_points = (left_points + right_points) / 2
        mid_sdf = evaluate(mid_points).unsqueeze(-1)
        ind_low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
        left_sdf[ind_low] = mid_sdf[ind_low]
        right_sdf[~ind_low] = mid_sdf[~ind_low]
        left_points[ind_low.flatten()] = mid_points[ind_low.flatten()]
        right_points[~ind_low.flatten()] = mid_points[~ind_low.flatten()]
        points = (left_points + right_points) / 2
    return points


def filter_mesh(points, faces, keep):
    """Net effect of trimesh's update_vertices(keep) + update_faces(all corners kept): kept vertices renumbered by prefix
    count, faces with a dropped corner removed."""
    remap = torch.cumsum(keep.long(), 0) - 1
    fk = keep[faces].all(dim=1)
    return points[keep], remap[faces[fk]]


def write_mesh_ply(path, vertices, faces):
    """Binary little-endian PLY: vertex (float x, y, z), face (list uchar int vertex_indices)."""
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    body = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    body["n"] = 3
    body["i"] = f
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.astype("<f4").tobytes())
        fh.write(body.tobytes())


@torch.no_grad()
def marching_tetrahedra_with_binary_search(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size,
                                           meshes_path, timestep, loaded_iter, *, num_down_emb_c, num_down_emb_f,
                                           masks=None, evaluate=None, marching=None, keep=None, prepare=None,
                                           timings=None):
    """mesh_extract_tetrahedra.py:64-139 for one timestep: returns (vertices [V,3] float32, faces [F,3] int64) and writes
    meshes_path/recon.ply.  `evaluate(points) -> sdf` and `marching` (utils/tetmesh.py's signature) default to the view
    cache and the HIP kernel; `prepare(views) -> [CachedView]` replaces prepare_views (stand-in probes); `keep`
    overrides the outlier filter; `timings`, a dict, receives per-phase seconds."""
    import time as _time

    def tick(key, t0):
        if timings is not None:
            torch.cuda.synchronize() if torch.cuda.is_available() else None
            timings[key] = timings.get(key, 0.0) + _time.perf_counter() - t0
        return _time.perf_counter()

    if marching is None:
        from .tetmesh import marching_tetrahedra as marching
    t0 = _time.perf_counter()
    pc = gaussians
    means3D_final, scales_deformed, rotations_deformed, opacity_deformed, _ = _deform(pc, timestep, loaded_iter,
                                                                                      num_down_emb_c, num_down_emb_f)
    scales_final, _ = pc.apply_scaling_n_opacity_with_3D_filter(opacity=opacity_deformed, scales=scales_deformed)
    t0 = tick("deformation", t0)
    points, points_scale = get_tetra_points(rotations_deformed, means3D_final, scales_final, keep=keep)
    t0 = tick("tetra_points", t0)
    cells = triangulate(points)
    t0 = tick("triangulate", t0)
    if evaluate is None:
        if prepare is None:
            cached = prepare_views(views, pc, pipeline, background, kernel_size, loaded_iter, num_down_emb_c, num_down_emb_f,
                                   masks=masks)
        else:
            cached = prepare(views)
        if timings is not None:
            timings["bytes_per_view"] = max((cv.nbytes for cv in cached), default=0)
        t0 = tick("prepare", t0)

        def evaluate(p):
            return evaluate_cull_alpha(p, cached)
    sdf = evaluate(points)
    t0 = tick("probe", t0)
    verts_list, scale_list, faces_list, _ = marching(points[None], cells, sdf[None], points_scale[None])
    end_points, end_sdf = (x.to(points.device) for x in verts_list[0])
    end_scales = scale_list[0].to(points.device)
    faces = faces_list[0].to(points.device)
    t0 = tick("marching_tetrahedra", t0)
    left, right = end_points[:, 0, :], end_points[:, 1, :]
    distance = torch.norm(left - right, dim=-1)
    scale = end_scales[:, 0, 0] + end_scales[:, 1, 0]

    def timed_eval(p):
        t = _time.perf_counter()
        r = evaluate(p)
        tick("probe", t)
        return r

    t1 = _time.perf_counter()
    points = bisect_edges(end_points, end_sdf, timed_eval)
    if timings is not None:
        tick("bisection_total", t1)
    t0 = _time.perf_counter()
    vertices, faces = filter_mesh(points, faces, distance <= scale)
    os.makedirs(meshes_path, exist_ok=True)
    write_mesh_ply(os.path.join(meshes_path, "recon.ply"), vertices.cpu().numpy(), faces.cpu().numpy())
    tick("filter_ply", t0)
    return vertices, faces
