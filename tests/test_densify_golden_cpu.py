"""SURVEY 8(f) rank 2, pinned by the reference itself: `ed3dgs_amd.densify_stats` against tests/golden/densify_reference.npz, which
tools/gen_densify_golden.py wrote by running the REFERENCE's own `GaussianModel.add_densification_stats` (scene/gaussian_model.py
:516-518, train.py:404-407) and `GaussianModel.densify` (= densify_and_clone + densify_and_split, :452-514, including
densification_postfix / prune_points and their optimizer surgery) on a synthetic 1 200-Gaussian model on the CPU.  The split's normal
samples come from a generator seeded with the iteration number on both sides (densify_tensors' convention; the reference draws
from the device RNG), so the comparison is bit for bit: accumulators, and every post-densify tensor (1 200 -> ~2 000 rows) -- except
the last bits of the split's NEW positions and scales.  Those alone pass through MKL's vector math (the sqrt of build_rotation, the
exp / log of the scales) and its bmm, whose roundings follow the kernels MKL picks for the host CPU: on an AMD EPYC host, where MKL
ignores MKL_CBWR, they differ from the fixture's in the last bit or two (so would the reference's own code), so those rows are held
to a few float32 ulps of their magnitude."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-d3dgs_amd"))
GOLD = os.path.join(ROOT, "tests", "golden", "densify_reference.npz")


def _load():
    z = np.load(GOLD)
    P, views, iteration = (int(x) for x in z["params"])
    max_grad, extent, percent_dense = (float(x) for x in z["thresholds"])
    return z, P, views, iteration, max_grad, extent, percent_dense


def _stats(z, P, views):
    from ed3dgs_amd import densify_stats as DS
    st = DS.DensificationStats(P, "cpu")
    for i in range(views):
        grad, radii = torch.from_numpy(z["view%d_grad" % i]), torch.from_numpy(z["view%d_radii" % i])
        st.add(grad, radii > 0, radii)
    return st


def test_accumulators_equal_the_references():
    z, P, views, *_ = _load()
    st = _stats(z, P, views)
    assert np.array_equal(st.xyz_gradient_accum.numpy(), z["accum"])
    assert np.array_equal(st.denom.numpy(), z["denom"])
    assert np.array_equal(st.max_radii2D.numpy(), z["max_radii2D"])
    assert (z["denom"] == 0).any() and (z["denom"] > 1).any()          # never-visible rows and several visits both occur


def test_densify_tensors_equal_the_references_post_densify_model():
    from ed3dgs_amd import densify_stats as DS
    z, P, views, iteration, max_grad, extent, percent_dense = _load()
    st = _stats(z, P, views)
    names = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation", "embedding", "tongue_class")
    t = {k: torch.from_numpy(z["in_" + k]) for k in names}
    out = DS.densify_tensors(t, st, max_grad, extent, iteration, percent_dense=percent_dense)
    cm, sm, _ = DS.decide(st, torch.exp(t["scaling"]), torch.sigmoid(t["opacity"]), max_grad, 0.005, extent, None, percent_dense=percent_dense)
    n_ref = z["out_xyz"].shape[0]
    n_new = 2 * int(sm.sum())                                           # the split's new rows: the last ones
    assert n_ref > P and n_new > 0                                      # the round cloned and split
    for k in names:
        assert tuple(out[k].shape) == z["out_" + k].shape, k
        got, ref = out[k].numpy(), z["out_" + k]
        if k not in ("xyz", "scaling"):
            assert np.array_equal(got, ref), k                          # bit for bit
            continue
        assert np.array_equal(got[:-n_new], ref[:-n_new]), k            # kept and cloned rows: bit for bit
        # the split's new positions R (s * n) + x and scales log(s / 1.6): the host CPU's MKL roundings, a few ulps of the magnitude
        mag = np.maximum(np.abs(ref[-n_new:]), np.float32(1.0 if k == "xyz" else 0.0))
        err = np.abs(got[-n_new:].astype(np.float64) - ref[-n_new:])
        assert (err <= 4 * np.spacing(mag)).all(), (k, float(err.max()))
    # the masks decide() reports are the ones behind those tensors: clones appended after the originals, splits after them, the split
    # originals removed
    assert n_ref == P + int(cm.sum()) + 2 * int(sm.sum()) - int(sm.sum())
    kept = (~sm).nonzero().reshape(-1)
    assert np.array_equal(out["xyz"][: kept.numel()].numpy(), t["xyz"][kept].numpy())
