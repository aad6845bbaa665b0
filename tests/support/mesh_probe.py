"""Stand-ins around the mesh-extraction glue (mesh_extract_tetrahedra.py + utils/mesh_extraction_utils.py, and this repo's
ed3dgs_amd/mesh.py): a small Gaussian model whose deformation network is a recording affine map, cameras with fixed
sizes, and an ANALYTIC integrate -- alpha = s / (s + |p - o|) per view (0.5 on a sphere of radius s around o), a linear
pixel coordinate, points "behind" a plane left unwritten (alpha 1, coordinate (0, 0), as the real probe leaves culled
points) and a fixed disc as render[7].  Only + - * / sqrt and comparisons: the same bits wherever it runs.  Used by
tools/gen_mesh_glue_golden.py on the REFERENCE's glue and by tests/test_mesh_glue_cpu.py on this repo's.  CPU only."""
import types

import numpy as np
import torch

K_GAUSSIANS, TIMESTEP, LOADED_ITER, MIN_EMB = 64, 3, 14000, 7
VIEWS = ((40, 30, (0.05, -0.02, 0.0), 0.55, 24.0, 11.0), (36, 32, (-0.03, 0.04, 0.02), 0.6, 20.0, 12.0),
         (44, 28, (0.0, 0.0, -0.04), 0.5, 26.0, 9.0))   # W, H, sphere centre o, radius s, pixels per unit, disc radius


class Deformation:
    """Records its arguments; returns an affine function of the inputs and the time."""

    def __init__(self):
        self.calls = []

    def __call__(self, means3D, scales, rotations, opacity, time, cam_no, pc, _unused, shs, iter=None, num_down_emb_c=None,
                 num_down_emb_f=None):
        t = float(time.reshape(-1)[0]) if torch.is_tensor(time) else float(time)
        self.calls.append(dict(time=t, cam_no=cam_no, iter=iter, num_down_emb_c=num_down_emb_c, num_down_emb_f=num_down_emb_f,
                               n=int(means3D.shape[0])))
        f = torch.tensor(t, dtype=torch.float32)
        return (means3D + f * 0.0078125, scales + 0.25, rotations * 1.5 + f * 0.03125, opacity - 0.5, shs, None)


class Gaussians:
    def __init__(self):
        g = torch.Generator().manual_seed(21)
        u = torch.randn(K_GAUSSIANS, 3, generator=g)
        self._xyz = u / torch.sqrt((u * u).sum(1, keepdim=True)) * 0.55 + torch.randn(K_GAUSSIANS, 3, generator=g) * 0.03
        self._scaling = torch.randn(K_GAUSSIANS, 3, generator=g) * 0.3 - 3.2
        self._rotation = torch.randn(K_GAUSSIANS, 4, generator=g)
        self._opacity = torch.randn(K_GAUSSIANS, 1, generator=g)
        self._features = torch.randn(K_GAUSSIANS, 16, 3, generator=g)
        self.filter_3D = torch.rand(K_GAUSSIANS, 1, generator=g) * 0.01
        self._deformation = Deformation()

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return self._features

    def apply_scaling_n_opacity_with_3D_filter(self, opacity, scales):
        s = torch.exp(scales)
        sq = s * s + self.filter_3D * self.filter_3D
        return torch.sqrt(sq), torch.sigmoid(opacity)


def make_views():
    out = []
    for i, (W, H, o, s, k, r) in enumerate(VIEWS):
        v = types.SimpleNamespace(image_width=W, image_height=H, time=TIMESTEP, origin=torch.tensor(o, dtype=torch.float32),
                                  radius=float(s), ppu=float(k), disc=float(r), gt_alpha_mask=None)
        if i == 1:   # the reference's masks come from numpy: float64
            yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            v.gt_alpha_mask = torch.from_numpy(np.where(xx < W * 0.8, 1.0, 0.25)[None])
        out.append(v)
    return out


def analytic(points, view):
    """(alpha_integrated [PN], point_coordinate [PN,2], render [9,H,W]) of `view`."""
    o = view.origin
    dx, dy, dz = points[:, 0] - o[0], points[:, 1] - o[1], points[:, 2] - o[2]
    d = torch.sqrt(dx * dx + dy * dy + dz * dz)
    s = torch.tensor(view.radius, dtype=torch.float32)
    written = dz < 0.7
    alpha = torch.where(written, s / (s + d), torch.ones_like(d))
    u = dx * view.ppu + view.image_width * 0.5
    v = dy * view.ppu + view.image_height * 0.5
    coord = torch.where(written[:, None], torch.stack([u, v], 1), torch.zeros(points.shape[0], 2))
    H, W = view.image_height, view.image_width
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ex, ey = xx - W * 0.5, yy - H * 0.5
    render = torch.zeros(9, H, W)
    render[7] = (ex * ex + ey * ey < view.disc * view.disc).float() * 0.875
    return alpha, coord, render


class Recorder:
    def __init__(self):
        self.eval_points = []

    def integrate(self, points, view, gaussians, pipeline, background, kernel_size, loaded_iter=None, num_down_emb_c=None,
                  num_down_emb_f=None):
        """gaussian_renderer.integrate stand-in for the reference's glue."""
        if view is self.first_view:
            self.eval_points.append(points.clone().numpy())
        alpha, coord, render = analytic(points, view)
        return {"alpha_integrated": alpha, "point_coordinate": coord, "render": render, "point_sdf": None,
                "color_integrated": None}


class AnalyticView:
    """A prepared view for ed3dgs_amd.mesh (what diff_gaussian_rasterization._C.IntegrateView offers)."""

    def __init__(self, view, recorder, first):
        self.view, self.rec, self.first = view, recorder, first
        self.out_color = analytic(torch.zeros(0, 3), view)[2]
        self.nbytes = 0

    def probe(self, points):
        if self.first:
            self.rec.eval_points.append(points.clone().numpy())
        alpha, coord, _ = analytic(points, self.view)
        return alpha, torch.zeros(points.shape[0], 3), coord, torch.full((points.shape[0],), -1000.0)


def keep_indices(n):
    """The stand-in statistical outlier filter's choice (indices into the Gaussians)."""
    return np.array([i for i in range(n) if i % 7 != 3], np.int64)
