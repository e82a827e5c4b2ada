"""Mesh extraction (csrc/tsdf.hip) against the float64 restatements of tests/tsdf_refs.py.
Integration: on every voxel whose decisions no fp32 rounding can flip (tsdf_refs' `fragile` mask, capped at 5 % by
tests/test_tsdf_refs_cpu.py) the weight is the reference's exactly, tsdf and rgb pass helpers.assert_elem_close (K = 8
times the float32 reference's own error), and a voxel the reference never updates keeps its initial state bit for bit --
which is what an over-eager update or a culling bug would break.  Batches: 6 views at once and as 2 + 3 + 1, the same bits.
Extraction: vertex and triangle SETS equal the reference's (tsdf_refs.canonical), every vertex used, indices in range, two
runs the same bits; closed cases are 2-manifolds of Euler characteristic 2 with positive volume.  Then the refusals (no
GPU needed: they come before any device work) and one walk through meshing.fuse_views."""
import math

import numpy as np
import pytest
import torch

import tsdf_refs as TR
from helpers import assert_elem_close

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    return TR.scene()


def _fused(scene, device, V, color, weights=None, depth_trunc=math.inf, splits=None):
    from meshing import TSDFVolume

    vol = TSDFVolume(scene["origin"], scene["voxel_size"], scene["dims"], scene["trunc"], color=color, device=device)
    dev = lambda a: torch.from_numpy(a).to(device)
    s = 0
    for n in splits or [V]:
        vol.integrate(dev(scene["depths"][s:s + n]), dev(scene["views"][s:s + n]), scene["tanfovx"], scene["tanfovy"],
                      colors=dev(scene["colors"][s:s + n]) if color else None,
                      weights=None if weights is None else weights[s:s + n], depth_trunc=depth_trunc)
        s += n
    return vol


@gpu
@pytest.mark.parametrize("name", list(TR.integration_cases()))
def test_integration_against_float64(device, scene, name):
    kw = TR.integration_cases()[name]
    (t64, w64, c64), (t32, w32, c32), fragile = TR.case_refs(scene, **kw)
    t, w, c = (None if p is None else p.cpu().numpy() for p in _fused(scene, device, **kw).dense())
    keep, T = ~fragile, torch.from_numpy
    assert np.array_equal(w[keep], w64[keep].astype(np.float32)), "weights"
    ratio = assert_elem_close(T(t[keep]), T(t64[keep]), T(t32[keep]), what="tsdf")
    idle = keep & (w64 == 0)
    assert idle.sum() > 500 and np.all(t[idle] == 1.0) and np.all(w[idle] == 0.0)
    if kw["color"]:
        ratio = max(ratio, assert_elem_close(T(c[:, keep]), T(c64[:, keep]), T(c32[:, keep]), what="rgb"))
        assert np.all(c[:, idle] == 0.0)
    print(f"TSDF integrate {name}: {int((keep & (w64 > 0)).sum())} voxels held, worst error / unit {ratio:.3g} of 8")


@gpu
def test_batches_give_the_same_bits(device, scene):
    kw = dict(V=6, color=True, weights=[1, 2, 1, 2, 2, 1])
    a, b = _fused(scene, device, **kw), _fused(scene, device, splits=[2, 3, 1], **kw)
    for p, q in ((a.tsdf, b.tsdf), (a.weight, b.weight), (a.rgb, b.rgb)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    assert float(a.weight.max()) > 3


@gpu
@pytest.mark.parametrize("name", list(TR.mesh_cases()))
def test_extraction_against_float64(device, name):
    from meshing import TSDFVolume

    tsdf, weight, closed = TR.mesh_cases()[name]
    Z, Y, X = tsdf.shape
    iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    lin = lambda x, y, z: np.stack([0.5 + 0.1 * x, 0.4 - 0.1 * y + 0.05 * z, 0.3 + 0.1 * z])  # colours linear in position
    rgb = lin(*(TR.MESH_ORIGIN[a] + TR.MESH_VOXEL * i for a, i in enumerate((ix, iy, iz)))).astype(np.float32)
    vol = TSDFVolume(TR.MESH_ORIGIN, TR.MESH_VOXEL, (X, Y, Z), 3 * TR.MESH_VOXEL, device=device)
    vol.from_dense(torch.from_numpy(tsdf), torch.from_numpy(weight), torch.from_numpy(rgb))
    assert all(torch.equal(p.cpu(), torch.from_numpy(q)) for p, q in zip(vol.dense(), (tsdf, weight, rgb)))
    runs = [vol.extract() for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*runs)), "two runs differ"
    v, f, c = (t.cpu().numpy() for t in runs[0])
    assert v.dtype == np.float32 and f.dtype == np.int32 and len(f) > 50
    assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)
    (v64, f64, _), (v32, f32, _) = (TR.mesh(d, tsdf, weight, TR.MESH_ORIGIN, TR.MESH_VOXEL) for d in (np.float64, np.float32))
    (ug, ng, fg), (u64, n64, t64), (u32, _, _) = (TR.canonical(a.astype(np.float64), b) for a, b in ((v, f), (v64, f64), (v32, f32)))
    assert ug.shape == u64.shape == u32.shape and np.array_equal(ng, n64), "vertex sets"
    ratio = assert_elem_close(torch.from_numpy(ug), torch.from_numpy(u64), torch.from_numpy(u32), what="vertices")
    assert np.array_equal(fg, t64), "triangle sets"
    assert np.abs(c - lin(*v.astype(np.float64).T).T).max() < 1e-5  # (a linear colour interpolates to itself)
    print(f"TSDF extract {name}: {len(v)} vertices, {len(f)} triangles, worst vertex error / unit {ratio:.3g} of 8")
    if closed:
        manifold, euler, volume = TR.closed_surface_figures(ug, fg)
        assert manifold and euler == 2 and volume > 0


def test_the_refusals_come_before_any_device_work():
    import diff_gaussian_rasterization as dgr

    lib, d = dgr.lib, 0x1000  # (a dummy non-zero integer stands for a device pointer: nothing is dereferenced)
    good = (8, 8, 8, 0.0, 0.0, 0.0, 0.1, 0.3, d, d, None, 1, 16, 16, d, 1.0, 1.0, d, None, None, 1e9, 0.2, d, 1 << 20, None)
    edit = lambda i, v: good[:i] + (v,) + good[i + 1:]
    for bad in (edit(0, 12), edit(2, 0), edit(7, 0.0), edit(11, 17), edit(8, None), edit(9, None), edit(6, 0.0)):
        assert lib.gsr_tsdf_integrate(*bad) == -1
    assert lib.gsr_tsdf_integrate(*edit(11, 0)) == 0 and lib.gsr_tsdf_integrate(*edit(23, 4)) == -2
    assert lib.gsr_tsdf_integrate_bytes(17, 16, 16) == 0 and lib.gsr_tsdf_extract_bytes(8, 12, 8) == 0
    assert lib.gsr_tsdf_integrate_bytes(2, 17, 16) == 2 * 2 * 1 * 8 and lib.gsr_tsdf_extract_bytes(16, 8, 8) == 2 * 16
    assert lib.gsr_tsdf_count(8, 8, 12, d, d, 0.0, d, d, 1 << 20, d, None) == -1
    assert lib.gsr_tsdf_count(8, 8, 8, d, None, 0.0, d, d, 1 << 20, d, None) == -1
    assert lib.gsr_tsdf_emit(8, 8, 8, 0.0, 0.0, 0.0, 0.1, d, d, None, 0.0, d, d, 1 << 20, 1 << 31, 1, d, d, None, None) == -1
    assert lib.gsr_tsdf_emit(8, 8, 8, 0.0, 0.0, 0.0, 0.1, d, None, None, 0.0, d, d, 1 << 20, 1, 1, d, d, None, None) == -1
    plane = torch.zeros(1, 1, 1, 8, 8, 8)
    args = ((0.0, 0.0, 0.0), 0.1, (8, 8, 8), 0.3, torch.zeros(1, 16, 16), torch.eye(4)[None], 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.tsdf_integrate(plane, plane.clone(), None, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.tsdf_extract(plane, plane.clone(), None, (0.0, 0.0, 0.0), 0.1, (8, 8, 8))
    with pytest.raises(ValueError, match="multiples of 8"):
        dgr.tsdf_integrate(plane, plane.clone(), None, args[0], 0.1, (8, 12, 8), *args[3:])
    with pytest.raises(ValueError, match="at most 16 views"):
        dgr.tsdf_integrate(plane, plane.clone(), None, *args[:4], torch.zeros(17, 16, 16), torch.eye(4).repeat(17, 1, 1), 1.0, 1.0)


@gpu
def test_fuse_views_to_a_mesh(device, tmp_path, monkeypatch):
    import gaussian_renderer as gr
    import meshing
    import synthetic_scene as S
    import test_gpu_normals as TN
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    model = S.SyntheticGaussianModel(2000, TN.PW, TN.PH, seed=3, sh_degree=TN.DEG, device=device)
    g = torch.Generator().manual_seed(5)
    n = torch.nn.functional.normalize(torch.randn(2000, 3, generator=g), dim=1)
    with torch.no_grad():  # flat-ish opaque splats on the sphere of radius 1.5 the cameras orbit
        model._xyz.copy_((n * 1.5 + torch.tensor([0.0, 0.0, 6.0])).to(device))
        model._scaling.fill_(math.log(0.08))
        model._opacity.fill_(3.0)
    TN._single_rank(4)
    cams = S.orbit_cameras(4, TN.PW, TN.PH, device=device)
    strategies, _ = start_strategy_final(cams, DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0))
    vol = meshing.TSDFVolume((-2.0, -2.0, 4.0), 0.125, (30, 32, 32), 0.5, device=device)
    assert vol.dims == (32, 32, 32)
    rendered, handed = [], []
    render, integrate = gr.render_final, vol.integrate

    def spy_render(pkg, st):
        rendered.append(pkg)
        return render(pkg, st)

    def spy_integrate(d, *a, **k):
        handed.append(d.clone())
        return integrate(d, *a, **k)

    monkeypatch.setattr(gr, "render_final", spy_render)
    monkeypatch.setattr(vol, "integrate", spy_integrate)
    pipe = type("P", (), {"debug": False})()
    assert meshing.fuse_views(cams, model, pipe, torch.zeros(3, device=device), strategies, vol) is vol
    assert not gr.get_surfel_pass() and not gr.get_normal_consistency()
    assert len(handed) == 4 and all(torch.equal(h[0].view(torch.int32), p["batched_median_depth"][0].view(torch.int32))
                                    for h, p in zip(handed, rendered))
    v, f, c = vol.extract()
    lo, hi = torch.tensor(vol.origin, device=device), torch.tensor(vol.origin, device=device) + 0.125 * 31
    assert len(v) > 0 and len(f) > 0 and c.shape == v.shape and bool(torch.isfinite(v).all())
    assert bool((v >= lo).all() and (v <= hi).all()) and int(f.min()) >= 0 and int(f.max()) < len(v)
    path = tmp_path / "mesh.ply"
    meshing.save_ply(path, v, f, c)
    head = path.read_bytes().split(b"end_header\n", 1)
    assert f"element vertex {len(v)}\n".encode() in head[0] and f"element face {len(f)}\n".encode() in head[0]
    assert len(head[1]) == len(v) * 15 + len(f) * 13
