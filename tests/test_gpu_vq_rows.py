"""The codebook kernels of vq.hip (gsr_vq_assign / _update / _segment_sum / _decode) against plain float64 torch on the
host, every row checked, at the smallest shapes at which they can go wrong: the assignment's workgroup owns 256 rows
(16 per MFMA block) and streams the codebook in tiles of 64 (K = 200: the double buffer wraps), D is padded to a multiple
of 16 in registers, the segment reduction cuts the sorted order into chunks of 128; K = 65536 needs 17 key bits and
indices above 32767."""
import pytest
import torch

import diff_gaussian_rasterization as dgr

pytestmark = pytest.mark.gpu

# (P, K, D): a cross-section of P in {1, 255, 256, 257, 300}, K in {1, 63, 64, 65, 200}, D in {1, 3, 4, 45, 48, 64}
CASES = [(1, 1, 1), (255, 63, 3), (256, 64, 4), (257, 65, 45), (300, 200, 48), (300, 200, 64), (257, 200, 1),
         (300, 1, 45), (1, 65, 64), (300, 65536, 45)]
EPS = 2.0 ** -24


def _inputs(kind, P, K, D, seed=0):
    """rows [P,D] and codebook [K,D] (fp32, host).  lattice: distinct integer centroids (the digits of k in the smallest
    base b with b^D >= K), rows = a centroid + noise of 1e-3; ties: small integers with every centroid present twice;
    gauss: N(0,1)"""
    g = torch.Generator().manual_seed(seed + 1000 * D + K)
    if kind == "gauss":
        return torch.randn(P, D, generator=g), torch.randn(K, D, generator=g)
    if kind == "ties":
        half = torch.randint(-3, 4, ((K + 1) // 2, D), generator=g).float()
        return torch.randint(-3, 4, (P, D), generator=g).float(), torch.cat([half, half])[:K].contiguous()
    b = 2
    while b ** D < K:
        b += 1
    k = torch.arange(K)
    cb = torch.stack([(k // b ** d) % b if b ** d < K else torch.zeros_like(k) for d in range(D)], dim=1).float()
    own = torch.randint(0, K, (P,), generator=g)
    return cb[own] + 1e-3 * torch.randn(P, D, generator=g), cb


def _d64(x, c):
    """float64 squared distances [P,K]"""
    x, c = x.double(), c.double()
    return ((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * x @ c.t()).clamp_min(0.0)


@pytest.mark.parametrize("P,K,D", CASES)
@pytest.mark.parametrize("kind", ["lattice", "ties"])
def test_assign_equals_the_float64_argmin(device, kind, P, K, D):
    x, c = _inputs(kind, P, K, D)
    idx = dgr.vq_assign(x.to(device), c.to(device)).cpu()
    assert idx.dtype == torch.int32
    assert torch.equal(idx.long(), _d64(x, c).argmin(dim=1))  # argmin: the first of several minima


@pytest.mark.parametrize("P,K,D", CASES)
def test_assign_gaussian_rows_within_the_fp32_bound(device, P, K, D):
    x, c = _inputs("gauss", P, K, D)
    idx, dist = dgr.vq_assign(x.to(device), c.to(device), return_dist=True)
    idx, dist = idx.cpu().long(), dist.cpu().double()
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    chosen = ((x.double() - c.double()[idx]) ** 2).sum(1)
    bound = 4.0 * (D + 2) * EPS * (x.double().norm(dim=1) + c.double().norm(dim=1).max()) ** 2
    excess = chosen - _d64(x, c).min(dim=1).values
    print(f"max excess / bound {float((excess / bound).max()):.3g}, dist2 {float(((dist - chosen).abs() / bound).max()):.3g}")
    assert bool((excess <= bound).all())
    assert bool((dist >= 0).all()) and bool(((dist - chosen).abs() <= bound).all())
    if K == 65536:  # the uint16 round trip of the stored index
        assert int(idx.max()) > 32767
        assert torch.equal(torch.from_numpy(idx.numpy().astype("uint16").astype("int32")).long(), idx)


def _segment_ref(x, idx, K, w):
    """float64 sums per cluster of w x, of |w x|, of w, and the counts; indices outside [0,K) skipped"""
    ok = (idx >= 0) & (idx < K)
    xi, ii = x.double()[ok], idx[ok].long()
    wi = torch.ones(len(ii), dtype=torch.float64) if w is None else w.double()[ok]
    s = torch.zeros(K, x.shape[1], dtype=torch.float64).index_add_(0, ii, wi[:, None] * xi)
    a = torch.zeros(K, x.shape[1], dtype=torch.float64).index_add_(0, ii, (wi[:, None] * xi).abs())
    return s, a, torch.zeros(K, dtype=torch.float64).index_add_(0, ii, wi), torch.bincount(ii, minlength=K)


def _indices(spread, P, K, g):
    if spread == "one":  # one cluster holds every row
        return torch.full((P,), K - 1, dtype=torch.int32)
    idx = (torch.randint(0, (K + 1) // 2, (P,), generator=g) * 2).int()  # odd clusters stay empty
    if spread == "stray":
        idx[P // 2] = K
        idx[0] = -1
    return idx


@pytest.mark.parametrize("P,K,D", [(1, 1, 1), (255, 63, 3), (257, 65, 45), (300, 200, 64), (300, 65536, 45)])
@pytest.mark.parametrize("spread", ["even", "one", "stray"])
@pytest.mark.parametrize("weighted,integer", [(False, False), (True, False), (True, True)])
def test_update_and_segment_sum(device, P, K, D, spread, weighted, integer):
    g = torch.Generator().manual_seed(P + K + D)
    idx = _indices(spread, P, K, g)
    if integer:  # every sum exact in float64: bit-equal to the rounded reference
        x = torch.randint(-100, 101, (P, D), generator=g).float()
        w = 2.0 ** torch.randint(-3, 4, (P,), generator=g).float()
    else:
        x = torch.randn(P, D, generator=g)
        w = torch.rand(P, generator=g) + 0.1 if weighted else None
    s, a, ws, cnt = _segment_ref(x, idx, K, w)
    cb0 = torch.randn(K, D, generator=g)
    runs = []
    for _ in range(2):
        cb = cb0.clone().to(device)
        count, wsum = dgr.vq_update(x.to(device), idx.to(device), cb, None if w is None else w.to(device))
        runs.append((cb.cpu(), count.cpu(), wsum.cpu(), dgr.vq_segment_sum(x.to(device), idx.to(device), K).cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    cb, count, wsum, sums = runs[0]
    assert torch.equal(count.long(), cnt)
    full = cnt > 0
    assert torch.equal(cb[~full], cb0[~full])  # empty clusters keep their centroid
    mean = s[full] / ws[full][:, None]
    s1, a1 = _segment_ref(x, idx, K, None)[:2]
    if integer:
        assert torch.equal(cb[full], mean.float()) and torch.equal(wsum, ws.float()) and torch.equal(sums, s1.float())
    assert bool(((cb[full].double() - mean).abs() <= 2.0 ** -23 * mean.abs() + 2.0 ** -40 * a[full] / ws[full][:, None]).all())
    assert bool(((wsum.double() - ws).abs() <= 2.0 ** -23 * ws).all())
    assert bool(((sums.double() - s1).abs() <= 2.0 ** -23 * s1.abs() + 2.0 ** -40 * a1).all())


@pytest.mark.parametrize("P,K,D", [(1, 1, 1), (257, 65, 45), (300, 200, 64), (300, 65536, 3)])
def test_decode_and_its_gradient(device, P, K, D):
    g = torch.Generator().manual_seed(7 * P + K)
    cb = torch.randn(K, D, generator=g)
    idx = torch.randint(0, K, (P,), generator=g).int()
    if P > 2:
        idx[1], idx[2] = K, -5  # decoded as zeros, no gradient
    ok = (idx >= 0) & (idx < K)
    ref = torch.where(ok[:, None], cb[idx.long().clamp(0, K - 1)], torch.zeros(()))
    cbd = cb.to(device).requires_grad_(True)
    out = dgr.vq_decode(cbd, idx.to(device))
    assert torch.equal(out.detach().cpu(), ref)
    up = torch.randn(P, D, generator=g)
    out.backward(up.to(device))
    s, a = _segment_ref(up, idx, K, None)[:2]
    assert bool(((cbd.grad.cpu().double() - s).abs() <= 2.0 ** -23 * s.abs() + 2.0 ** -40 * a).all())


def test_shapes_and_host_tensors_are_refused(device):
    x, c = torch.zeros(4, 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.vq_assign(x, c)
    with pytest.raises(ValueError):
        dgr.vq_assign(torch.zeros(4, 65, device=device), torch.zeros(2, 65, device=device))  # D > 64
    with pytest.raises(ValueError):
        dgr.vq_update(x.to(device), torch.zeros(4, dtype=torch.int64, device=device), c.to(device))  # int32 indices
    assert dgr.vq_assign(torch.zeros(0, 3, device=device), c.to(device)).shape == (0,)
    lib = dgr._lib.lib
    assert lib.gsr_vq_assign(4, 65537, 3, 16, 16, 16, None, None) == -1 and lib.gsr_vq_workspace_bytes(4, 2, 0) == 0
