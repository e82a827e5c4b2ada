"""The references of the TSDF tests (tests/tsdf_refs.py) against closed forms, without a GPU: the cap on the share of
voxels the GPU test does not hold to the reference, the integration rule on a fronto-parallel plane, and the reference
mesher on a sphere (closed, consistently oriented, normals outwards)."""
import numpy as np
import pytest

import tsdf_refs as TR


@pytest.fixture(scope="module")
def scene():
    return TR.scene()


@pytest.mark.parametrize("name", list(TR.integration_cases()))
def test_fragile_share_is_capped(scene, name):
    (_, w64, _), _, fragile = TR.case_refs(scene, **TR.integration_cases()[name])
    live = w64 > 0
    share = float((fragile & live).sum()) / float(live.sum())
    print(f"TSDF refs {name}: {int(live.sum())} voxels with weight, fragile share {share:.4f}")
    assert live.sum() > 500 and share <= 0.05
    assert (w64 == 0).sum() > 500  # (untouched voxels exist: the exact-initial-state check has something to hold)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fronto_parallel_plane_closed_form(dtype):
    W, H, d0, trunc, vs = 32, 24, 2.0, 0.25, 0.0625
    origin, dims = (-0.25, -0.1875, 1.5), (8, 8, 16)
    depths = np.full((1, H, W), d0, np.float32)
    tsdf, w, _, _ = TR.integrate(dtype, origin, vs, dims, trunc, depths, np.eye(4, dtype=np.float32)[None], 0.5, 0.4)
    z = (origin[2] + vs * np.arange(16))[:, None, None] * np.ones((16, 8, 8))
    band = np.abs(d0 - z) <= trunc  # (every voxel of this volume projects inside the image)
    assert np.array_equal(w, band.astype(dtype))
    assert np.array_equal(tsdf, np.where(band, (d0 - z) / trunc, 1.0).astype(dtype))  # dyadic numbers: exact in both
    half, _, _, _ = TR.integrate(dtype, origin, vs, dims, trunc, np.concatenate([depths, depths + 0.125]),
                                 np.stack([np.eye(4, dtype=np.float32)] * 2), 0.5, 0.4, weights=[1, 3])
    both = band & (np.abs(d0 + 0.125 - z) <= trunc)
    assert np.array_equal(half[both], (((d0 - z) / trunc + 3 * (d0 + 0.125 - z) / trunc) / 4)[both].astype(dtype))


@pytest.mark.parametrize("name", ["sphere", "one_brick"])
def test_reference_mesh_of_a_sphere_is_closed_and_faces_outwards(name):
    tsdf, weight, closed = TR.mesh_cases()[name]
    v, f, _ = TR.mesh(np.float64, tsdf, weight, TR.MESH_ORIGIN, TR.MESH_VOXEL)
    manifold, euler, vol = TR.closed_surface_figures(v, f)
    assert closed and len(f) > 100 and manifold and euler == 2
    r = 0.8 if name == "sphere" else 0.31
    assert 0.9 * 4 / 3 * np.pi * r ** 3 < vol < 4 / 3 * np.pi * r ** 3  # (inscribed: a little less than the ball)
    # the sets the GPU test compares are well defined: fp32 and fp64 sort the vertices the same way
    v32, f32, _ = TR.mesh(np.float32, tsdf, weight, TR.MESH_ORIGIN, TR.MESH_VOXEL)
    (u64, c64, t64), (u32, c32, t32) = TR.canonical(v, f), TR.canonical(v32.astype(np.float64), f32)
    assert u64.shape == u32.shape and np.array_equal(c64, c32) and np.array_equal(t64, t32)
    assert np.abs(u64 - u32).max() < 1e-6
