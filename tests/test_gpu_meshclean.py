"""Mesh cleaning (csrc/meshclean.hip) against the numpy restatement of tests/meshclean_refs.py.  Everything is integer
work or a copy, so every comparison is exact: labels, triangle counts, and the filtered vertices / faces / colours as raw
int32 views (the vertex data holds a NaN, an infinity and a -0.0).  A second run gives the same bits.  The cases sit at
the union kernel's own chunk and window sizes (MESH_CHUNK_FACES, MESH_WINDOW_VERTICES)."""
import functools

import numpy as np
import pytest
import torch

import meshclean_refs as MR
import tsdf_refs as TR

gpu = pytest.mark.gpu
CASES = ("strip_ordered", "strip_shuffled", "confetti", "ties", "interleaved", "orphans")
PARAMS = [(0, 0), (1, 0), (2, 3), (0, 5)]
FILTER = [(n, k, m) for n in CASES for k, m in PARAMS] + [("ties", k, m) for k, m in ((2, 0), (3, 0), (4, 0), (4, 5))]


def _cases():
    import diff_gaussian_rasterization as dgr

    return MR.cases(dgr.MESH_CHUNK_FACES, dgr.MESH_WINDOW_VERTICES)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(faces, V, vertices, colors, labels, tri_count) of a case: the data and the reference, made once"""
    faces, V = _cases()[name]
    rng = np.random.default_rng(11)
    vertices, colors = (rng.standard_normal((V, 3)).astype(np.float32) for _ in range(2))
    vertices[V // 2], colors[V // 3, 1], vertices[V - 1, 2] = (np.nan, np.inf, -0.0), -np.inf, -0.0
    return (faces, V, vertices, colors) + MR.components(faces, V)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@gpu
@pytest.mark.parametrize("name", CASES)
def test_components_are_exact(device, name):
    import diff_gaussian_rasterization as dgr

    faces, V, _, _, labels, tri_count = _mesh(name)
    runs = [dgr.mesh_components(torch.from_numpy(faces).to(device), V) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*runs)), "two runs differ"
    assert runs[0][0].dtype == runs[0][1].dtype == torch.int32
    assert np.array_equal(runs[0][0].cpu().numpy(), labels), "labels"
    assert np.array_equal(runs[0][1].cpu().numpy(), tri_count), "tri_count"


@gpu
@pytest.mark.parametrize("name,k,m", FILTER)
def test_filter_is_exact(device, name, k, m):
    import diff_gaussian_rasterization as dgr

    faces, V, vertices, colors, labels, tri_count = _mesh(name)
    ref = MR.mesh_filter(vertices, faces, colors, k, m, comps=(labels, tri_count))
    dev = [torch.from_numpy(a).to(device) for a in (vertices, faces, colors)]
    before = [t.clone() for t in dev]
    runs = [dgr.mesh_filter(*dev, keep_largest=k, min_triangles=m) for _ in range(2)]
    assert all(torch.equal(_ti(p), _ti(q)) for p, q in zip(*runs)), "two runs differ"
    assert all(torch.equal(_ti(p), _ti(q)) for p, q in zip(dev, before)), "an input was written"
    for got, src, want, what in zip(runs[0], dev, ref, ("vertices", "faces", "colors")):
        assert got.numel() == 0 or got.data_ptr() != src.data_ptr(), f"{what}: not a copy"
        assert got.shape == want.shape and np.array_equal(_bits(got), want.view(np.int32)), what
    v, f, c = dgr.mesh_filter(dev[0], dev[1], None, keep_largest=k, min_triangles=m)
    assert c is None and torch.equal(_ti(v), _ti(runs[0][0])) and torch.equal(f, runs[0][1])
    print(f"mesh clean {name} k={k} m={m}: {len(faces)} -> {len(ref[1])} triangles, {V} -> {len(ref[0])} vertices")


def _ti(t):
    return t.view(torch.int32)


@gpu
@pytest.mark.parametrize("V", [5, 0])
def test_empty_meshes(device, V):
    import diff_gaussian_rasterization as dgr

    faces = torch.zeros((0, 3), dtype=torch.int32, device=device)
    labels, tri_count = dgr.mesh_components(faces, V)
    assert labels.dtype == tri_count.dtype == torch.int32
    assert labels.tolist() == list(range(V)) and tri_count.tolist() == [0] * V
    vertices = torch.randn(V, 3, device=device)
    for colors in (None, vertices + 1):
        v, f, c = dgr.mesh_filter(vertices, faces, colors, keep_largest=2)
        assert v.shape == (0, 3) and v.dtype == torch.float32 and f.shape == (0, 3) and f.dtype == torch.int32
        assert (c is None) if colors is None else (c.shape == (0, 3) and c.dtype == torch.float32)


@gpu
def test_volume_extract_keeps_the_largest_sphere(device):
    from meshing import TSDFVolume, clean_mesh

    iz, iy, ix = np.meshgrid(*(np.arange(32.0),) * 3, indexing="ij")
    spheres = (((10.13, 10.27, 10.41), 7.3), ((24.19, 22.07, 20.33), 4.6), ((8.23, 25.11, 26.37), 1.3))
    sdf = np.minimum.reduce([np.sqrt((ix - c[0]) ** 2 + (iy - c[1]) ** 2 + (iz - c[2]) ** 2) - r for c, r in spheres])
    tsdf = np.clip(sdf / 3, -1, 1).astype(np.float32)
    vol = TSDFVolume((0.0, 0.0, 0.0), 1.0, (32, 32, 32), 3.0, device=device)
    vol.from_dense(torch.from_numpy(tsdf), torch.ones(32, 32, 32), torch.rand(3, 32, 32, 32))
    full = vol.extract()
    assert all(torch.equal(_ti(p), _ti(q)) for p, q in zip(full, vol.extract(0.0, 0, 0)))
    labels, _ = MR.components(full[1].cpu().numpy(), len(full[0]))
    assert len(np.unique(labels)) == 3
    ref = MR.mesh_filter(*(t.cpu().numpy() for t in full), 1, 0)
    for got in (vol.extract(keep_largest=1), clean_mesh(*full, keep_largest=1)):
        assert all(np.array_equal(_bits(g), w.view(np.int32)) for g, w in zip(got, ref))
    v, f = ref[0].astype(np.float64), ref[1]
    manifold, euler, volume = TR.closed_surface_figures(v, f)
    assert manifold and euler == 2 and volume > 0 and 0 < len(f) < len(full[1])
    assert abs(volume / (4 / 3 * np.pi * 7.3 ** 3) - 1) < 0.05  # (the largest of the three)
