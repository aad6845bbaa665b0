"""bench.py --dump-outputs: what the last timed step computed goes to DIR/<name>.npy in float32 / float64, within the byte
budget, and arrays too large for their share are sampled at the same elements every time (two builds compare output for
output)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _kept():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    pkg = {"render": r(3, 64, 80), "mask": r(1, 64, 80), "radii": torch.arange(500, dtype=torch.int32),
           "visibility_filter": torch.ones(500, dtype=torch.bool), "extras": None, "tiny64": r(7).double(),
           "viewspace_points": torch.zeros(500, 3), "expected_coord": torch.zeros(3, 64, 80), "median_coord": torch.zeros(3, 64, 80),
           "tongue_mask": torch.zeros(1, 64, 80)}
    grads = [r(500, 3), None, r(500, 3, 15), r(500, 4), r(500, 1), r(500, 1, 3), r(500, 32),   # the seven per-Gaussian tensors
             torch.zeros(30, 1), r(2, 4), r(2)]                     # deformation, named_parameters() order: offsets, lin.weight, lin.bias
    return dict(pkg=pkg, grads=grads, viewspace_grad=r(500, 3))


class _Deformation(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 2)
        self.offsets = torch.nn.Parameter(torch.zeros(30, 1))


class _Model:
    _deformation = _Deformation()
    tongue_class = torch.zeros(500, 1)


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40_000)
    kept = _kept()
    names = bench.dump_outputs(kept, _Model(), str(tmp_path / "a"))
    again = bench.dump_outputs(_kept(), _Model(), str(tmp_path / "b"))
    assert names == again
    assert {"out_render", "out_radii", "out_tiny64", "grad_xyz", "grad_rotation", "grad_viewspace_points"} <= set(names)
    assert "out_extras" not in names and "grad_scaling" not in names          # None: nothing to write
    # zero by construction, not written: the gradient carrier, coordinate images not asked for, the tongue image of a scene without
    # tongue Gaussians, parameters the step does not read (the per-camera offsets under cam_no=None; the whole network and the
    # embeddings when nothing deforms)
    assert {"grad_deformation.lin.weight", "grad_deformation.lin.bias", "grad_embedding"} <= set(names)
    assert not {"out_viewspace_points", "out_expected_coord", "out_median_coord", "out_tongue_mask", "grad_deformation.offsets"} & set(names)
    static = bench.dump_outputs(_kept(), _Model(), str(tmp_path / "c"), deform=False)
    assert not [n for n in static if n.startswith("grad_deformation.")] and "grad_embedding" not in static and "grad_xyz" in static
    for d in ("a", "c"):
        assert all(np.load(tmp_path / d / (n + ".npy")).any() for n in os.listdir(tmp_path / d) for n in [n[:-4]])
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 40_000
    assert np.load(tmp_path / "a" / "out_tiny64.npy").dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "out_radii.npy"), np.arange(500, dtype=np.float32))
    # the sampled render holds elements of the render, in flat order
    s = np.load(tmp_path / "a" / "out_render.npy")
    full = kept["pkg"]["render"].numpy().reshape(-1)
    assert 0 < s.size < full.size and np.isin(s, full).all()


def test_steps_must_be_positive():
    import bench
    assert bench.parse_args(["--steps", "3"]).steps == 3
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
