"""The depth sort of the persistent prepare kernel (csrc/binning_persist.h): one global pass by depth bucket plus a
workgroup-local sort (the default) against the four global LSD passes (GSR_BIN_DEPTH_SORT=lsd).  Same lists, bit for
bit -- sorted ids, offsets, segoff, pair count, point_list, ranges -- and, from the kernel's timeline stamps, WHICH path
every launch took: a comparison that cannot tell the paths apart proves nothing."""
import ctypes
import math

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import synthetic_scene as S

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
# stamp slots of bin_prepare_persist_kernel (32 per workgroup) that only one path writes
SLOT_BUCKETS = 28   # behind the bucket path's last barrier
SLOT_FALLBACK = 18  # behind the barrier of the recount that leads from the bucket path back to the four passes
SLOT_LSD_LAST = 20  # behind the last barrier of the four-pass path
BK_BINS, BK_BIN_BITS, BK_CAP, BK_TAIL = 4096, 12, 8192, 255


def _c1_views(device):
    """the c1 views of bench.py (1 M Gaussians, 1080p, seed 0): K1's outputs for camera 0 and camera 3"""
    g = S.make_gaussians(1_000_000, W, H, seed=0, device=device)
    out = {}
    for ci in (0, 3):
        cam = S.orbit_cameras(8, W, H, device=device)[ci]
        rs = dgr.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                                               torch.zeros(3, device=device), 1.0, cam.world_view_transform,
                                               cam.full_proj_transform, 3, cam.camera_center, False, False)
        with torch.no_grad():
            m2, _, co, radii, depths = dgr.GaussianRasterizer(rs).preprocess_gaussians(
                g["means3D"], g["scales"], g["rotations"], g["shs"], g["opacities"], {})
        out[ci] = [t.detach().contiguous() for t in (m2, depths, radii.to(torch.int32), co)]
    return out


@pytest.fixture(scope="module")
def views(device):
    return _c1_views(device)


def _mask(device):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return torch.ones(gx * gy, dtype=torch.uint8, device=device)


def _timeline():
    grid = ctypes.c_int(0)
    buf = np.zeros(1024 * 32, dtype=np.uint64)
    rc = dgr.lib.gsr_bin_timeline(0, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(grid))
    assert rc == 0, rc
    return buf[:grid.value * 32].reshape(grid.value, 32), grid.value


def _path(t):
    """which depth sort the last prepare launch ran, from its stamps"""
    new, fb, lsd = (bool((t[:, k] > 0).any()) for k in (SLOT_BUCKETS, SLOT_FALLBACK, SLOT_LSD_LAST))
    assert (t[:, 2] > 0).all(), "the launch did not pass its first barrier"
    assert new != lsd, "exactly one of the two paths finishes a launch"
    if new:
        assert not fb and (t[:, SLOT_BUCKETS] > 0).all()
        return "buckets"
    assert (t[:, SLOT_LSD_LAST] > 0).all()
    return "fallback" if fb else "lsd"


def _prepare(inp, mask, monkeypatch, lsd):
    """the prepare step through the C entry point bin_gaussians uses, on a workspace of our own: sorted ids, offsets,
    segoff (with their totals), tiles_touched, the pair count, the path and the grid"""
    m2, depths, radii, co = inp
    P = m2.shape[0]
    lib = dgr.lib
    if lsd:
        monkeypatch.setenv("GSR_BIN_DEPTH_SORT", "lsd")
    else:
        monkeypatch.delenv("GSR_BIN_DEPTH_SORT", raising=False)
    nbytes = lib.gsr_bin_prepare_bytes(P, W, H)
    prep = torch.zeros(nbytes, dtype=torch.uint8, device=m2.device)
    ticket = ctypes.c_uint32(0)
    stream = dgr._stream()
    dgr.check(lib.gsr_bin_prepare_async(P, W, H, dgr._ptr(m2), dgr._ptr(depths), dgr._ptr(radii), dgr._ptr(co),
                                        dgr._ptr(mask), dgr._ptr(prep), nbytes, ctypes.byref(ticket), stream),
              "gsr_bin_prepare_async")
    D = ctypes.c_int64(0)
    dgr.check(lib.gsr_bin_count_wait(ticket.value, ctypes.byref(D), stream), "gsr_bin_count_wait")
    torch.cuda.synchronize()
    t, G = _timeline()
    # the workspace: tiles_touched at 0, segoff one (P + 1)-word array further, the sorted ids two more (csrc/binning_host.h:
    # prep_layout); the two totals sit behind their arrays at the offsets the library names
    words = prep.view(torch.int32)
    off_o = lib.gsr_bin_total_offset(P, W, H) // 4 - P
    off_s = lib.gsr_bin_segments_offset(P, W, H) // 4 - P
    stride = off_s
    res = dict(ids=words[3 * stride:3 * stride + P].clone(), offsets=words[off_o:off_o + P + 1].clone(),
               segoff=words[off_s:off_s + P + 1].clone(), tt=words[:P].clone(), D=int(D.value), path=_path(t), G=G)
    return res


def _rule(inp, res):
    """the capacity rule of the bucket path applied on the host to the same keys: bins, map, bucket sizes"""
    keys = inp[1].view(torch.int32).cpu().numpy().view(np.uint32)[(res["tt"] != 0).cpu().numpy()].astype(np.int64)
    if keys.size == 0 or keys.max() == 0xFFFFFFFF:
        return "fallback"
    kmin, kmax = int(keys.min()), int(keys.max())
    sh = max(int(kmax - kmin).bit_length() - BK_BIN_BITS, 0)
    cnt = np.bincount((keys - kmin) >> sh, minlength=BK_BINS)
    start = np.cumsum(cnt) - cnt
    nb = min(res["G"], BK_TAIL)
    size = np.bincount(start * nb // keys.size, weights=cnt, minlength=nb)
    return "buckets" if size.max() <= BK_CAP else "fallback"


def _compare(inp, device, monkeypatch, expect):
    """both depth sorts on one view: equal lists, and the default took the path `expect` ("rule": what the capacity rule
    gives on the host)"""
    mask = _mask(device)
    inp = [t.contiguous() for t in inp]
    monkeypatch.setenv("GSR_BIN_TIMELINE", "1")
    dgr.set_bin_persistent("both")
    dgr.set_speculative_sort(False)
    try:
        dgr.release_workspaces()
        ref = _prepare(inp, mask, monkeypatch, lsd=True)
        pl_ref, rg_ref, D_ref = dgr.bin_gaussians(*inp, mask, W, H)
        pl_ref, rg_ref = pl_ref.clone(), rg_ref.clone()
        got = _prepare(inp, mask, monkeypatch, lsd=False)
        pl, rg, D = dgr.bin_gaussians(*inp, mask, W, H)
        torch.cuda.synchronize()
    finally:
        dgr.set_bin_persistent("env")
        dgr.set_speculative_sort(True)
        dgr.release_workspaces()
    assert ref["path"] == "lsd"
    want = _rule(inp, ref) if expect == "rule" else expect
    print(f"P {inp[0].shape[0]} grid {got['G']} D {got['D']} path {got['path']} (expected {want})")
    assert got["path"] == want
    assert got["D"] == ref["D"] == D == D_ref
    for k in ("tt", "ids", "offsets", "segoff"):
        assert torch.equal(got[k], ref[k]), k
    assert torch.equal(torch.sort(got["ids"]).values, torch.arange(inp[0].shape[0], dtype=torch.int32, device=device))
    assert torch.equal(pl[:D], pl_ref[:D])
    assert torch.equal(rg, rg_ref)
    return got


def _with_depths(inp, depths):
    m2, _, radii, co = inp
    return [m2, depths.to(torch.float32).contiguous(), radii, co]


def _live(inp, device, monkeypatch):
    """rows of the view that K3 gives at least one tile"""
    monkeypatch.setenv("GSR_BIN_TIMELINE", "1")
    return (_prepare(inp, _mask(device), monkeypatch, lsd=True)["tt"] != 0).nonzero().flatten()


@pytest.mark.parametrize("cam", [0, 3])
def test_c1_view(device, monkeypatch, views, cam):
    """(a) the bench's view: 1 M Gaussians at 1080p, thousands of exact depth ties"""
    got = _compare(views[cam], device, monkeypatch, "buckets")
    assert got["D"] > 1_000_000


def test_all_depths_equal_falls_back(device, monkeypatch, views):
    """(b) one key value: one bucket would hold every live Gaussian -- the four passes in the same launch"""
    _compare(_with_depths(views[0], torch.full_like(views[0][1], 3.25)), device, monkeypatch, "fallback")


def test_two_depths_interleaved(device, monkeypatch, views):
    """(c) stability across the global and the local pass: two depth values in turn, 8000 Gaussians (two buckets)"""
    inp = [t[:8000] for t in views[0]]
    dep = torch.where(torch.arange(8000, device=device) % 2 == 0, 2.5, 7.0)
    _compare(_with_depths(inp, dep), device, monkeypatch, "buckets")


def test_heavy_ties(device, monkeypatch, views):
    """(c) 1 M Gaussians on 50 000 distinct depths"""
    gen = torch.Generator(device="cpu").manual_seed(11)
    levels = torch.rand(50_000, generator=gen) * 9.0 + 0.5
    dep = levels[torch.randint(0, 50_000, (1_000_000,), generator=gen)].to(device)
    _compare(_with_depths(views[0], dep), device, monkeypatch, "buckets")


def test_skewed_depths(device, monkeypatch, views):
    """(d) depths over 0.21 .. 1e6 with 99 % of them inside 1 % of the range of the key bits"""
    gen = torch.Generator(device="cpu").manual_seed(12)
    lo = np.array([0.21], dtype=np.float32).view(np.uint32)[0].item()
    hi = np.array([1e6], dtype=np.float32).view(np.uint32)[0].item()
    n = 1_000_000
    bits = torch.randint(lo, hi + 1, (n,), generator=gen, dtype=torch.int64)
    c0 = lo + (hi - lo) // 3
    dense = torch.randint(c0, c0 + (hi - lo) // 100, (n,), generator=gen, dtype=torch.int64)
    bits = torch.where(torch.rand(n, generator=gen) < 0.99, dense, bits)
    bits[0], bits[1] = lo, hi
    dep = bits.to(torch.int32).view(torch.float32).to(device)
    inp = _with_depths(views[0], dep)
    live = _live(views[0], device, monkeypatch)
    inp[1][live[0]], inp[1][live[1]] = 0.21, 1e6  # (the two ends are live whatever K3 culls)
    _compare(inp, device, monkeypatch, "rule")


@pytest.mark.parametrize("P", [1, 4095, 4097])
def test_small_views(device, monkeypatch, views, P):
    """(e) one Gaussian; one row short of a tile; one row into the second tile"""
    first = int(_live(views[0], device, monkeypatch)[0])
    _compare([t[first:first + P] for t in views[0]], device, monkeypatch, "buckets")


def test_every_gaussian_culled(device, monkeypatch, views):
    """(e) nothing live: no key range to cut into buckets -- the four passes"""
    inp = [t[:100_000].clone() for t in views[0]]
    inp[2].zero_()
    got = _compare(inp, device, monkeypatch, "fallback")
    assert got["D"] == 0


def test_padded_slab(device, monkeypatch, views):
    """(f) the shape of a rank of eight: a 1.5 M-row slab, every third row padding (radius 0: key 0xFFFFFFFF); 8192-row
    tiles"""
    inp = [torch.cat([t, t[:500_000]]).contiguous() for t in views[3]]
    inp[2][::3] = 0
    got = _compare(inp, device, monkeypatch, "buckets")
    assert got["G"] < 245  # (tiles of 8192 rows)
