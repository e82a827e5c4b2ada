"""The bilateral-grid colour correction (include/gsraster.h, N1g) restated in torch with explicit index
arithmetic, parameterised by dtype, plus the constructed inputs of its tests.  Shared by tests/test_bilagrid_refs_cpu.py,
which pins the restatement on torch's own grid_sample and verifies the input conditions, and by the GPU files, which hold
the HIP kernels against its fp64 run with its fp32 run as the unit of the tolerance."""
import torch

# (name, W, H, (GW, GH, L), band or None): the cases of tests/test_gpu_bilagrid_slice.py
DEFAULT = (16, 16, 8)
CASES = [
    ("1x1", 1, 1, DEFAULT, None),
    ("33x17", 33, 17, DEFAULT, None),
    ("33x17-band", 33, 17, DEFAULT, (5, 12)),
    ("67x35", 67, 35, DEFAULT, None),             # the width is no multiple of a wave
    ("96x64", 96, 64, DEFAULT, None),             # cells (6.4 x 4.3 pixels) smaller than any tile
    ("67x35-g222", 67, 35, (2, 2, 2), None),      # one cell, six pieces
    ("67x35-g354", 67, 35, (3, 5, 4), None),      # three different sizes: a swapped pair of axes shows
    ("67x35-g5416", 67, 35, (5, 4, 16), None),    # L = 16: three corner sums per lane in the backward
]
MARGIN = 2.0 ** -10  # pz of every unclamped pixel is at least this far from an integer
# a colour in range whose luminance, summed in the stated order, is exactly 1 in float32 AND in float64 (r = g = b = 1
# gives 1 in float32 but 1 - 2^-53 in float64: such a pixel would be clamped in one precision and not in the other)
LUM_ONE = (1.171875, 1.015625, 0.46875)


def _axis(n, g, dtype, lo=0, hi=None):
    """lower node and fraction of the pixel centres lo .. hi-1 of an axis of n pixels under g nodes"""
    p = (torch.arange(lo, n if hi is None else hi, dtype=dtype) + 0.5) / n * (g - 1)
    i0 = torch.floor(p).clamp(max=g - 2)
    return i0.long(), p - i0


def luminance(c):
    return 0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2]


def _lerp(a, b, t):
    return a + t * (b - a)


def slice_reference(image, grid, dtype, y0=0, y1=None):
    """x' of rows [y0, y1) of image [3,H,W] under grid [12,L,GH,GW], computed in `dtype` -> [3, y1 - y0, W].
    Differentiable in both; the guide's derivative is cut (exactly 0) where the luminance is <= 0 or >= 1."""
    _, H, W = image.shape
    _, L, GH, GW = grid.shape
    y1 = H if y1 is None else y1
    c = image[:, y0:y1].to(dtype)
    G = grid.to(dtype)
    ix, tx = _axis(W, GW, dtype)
    iy, ty = _axis(H, GH, dtype, y0, y1)
    ix, tx, iy, ty = ix[None, :], tx[None, :], iy[:, None], ty[:, None]
    lum = luminance(c)
    live = (lum > 0) & (lum < 1)
    pz = torch.where(live, lum, lum.detach().clamp(0, 1)) * (L - 1)
    iz = torch.floor(pz.detach()).clamp(max=L - 2)
    tz = pz - iz
    iz = iz.long()

    def node(dz, dy, dx):
        return G[:, iz + dz, iy + dy, ix + dx]  # [12, rows, W]

    lo = _lerp(_lerp(node(0, 0, 0), node(0, 0, 1), tx), _lerp(node(0, 1, 0), node(0, 1, 1), tx), ty)
    hi = _lerp(_lerp(node(1, 0, 0), node(1, 0, 1), tx), _lerp(node(1, 1, 0), node(1, 1, 1), tx), ty)
    M = _lerp(lo, hi, tz).reshape(3, 4, y1 - y0, W)
    return M[:, 0] * c[0] + M[:, 1] * c[1] + M[:, 2] * c[2] + M[:, 3]


def slice_gridsample(image, grid, dtype, y0=0, y1=None):
    """the same through torch.nn.functional.grid_sample on the 5-D lattice (bilinear, align_corners, border)"""
    _, H, W = image.shape
    y1 = H if y1 is None else y1
    c = image[:, y0:y1].to(dtype)
    rows = y1 - y0
    u = ((torch.arange(W, dtype=dtype) + 0.5) / W).expand(rows, W)
    v = ((torch.arange(y0, y1, dtype=dtype) + 0.5) / H)[:, None].expand(rows, W)
    at = torch.stack([u, v, luminance(c)], dim=-1) * 2 - 1
    M = torch.nn.functional.grid_sample(grid.to(dtype)[None], at[None, None], mode="bilinear", align_corners=True,
                                        padding_mode="border")[0, :, 0].reshape(3, 4, rows, W)
    return M[:, 0] * c[0] + M[:, 1] * c[1] + M[:, 2] * c[2] + M[:, 3]


def slice_with_grads(fn, image, grid, gout, dtype, y0=0, y1=None):
    """-> (x' [3,rows,W], dL/dimage of the band's rows [3,rows,W], dL/dgrid [12,L,GH,GW]) for L = sum(x' * gout)"""
    x = image.to(dtype).clone().requires_grad_(True)
    g = grid.to(dtype).clone().requires_grad_(True)
    _, H, _ = image.shape
    y1 = H if y1 is None else y1
    out = fn(x, g, dtype, y0, y1)
    (out * gout[:, y0:y1].to(dtype)).sum().backward()
    return out.detach(), x.grad[:, y0:y1].clone(), g.grad


def tv_reference(grids):
    """T = (1/N) sum over the axes z, y, x of mean((G shifted by one - G)^2) of grids [N,12,L,GH,GW], in their dtype"""
    T = 0
    for dim in (2, 3, 4):
        n = grids.shape[dim]
        d = grids.narrow(dim, 1, n - 1) - grids.narrow(dim, 0, n - 1)
        T = T + (d * d).mean()  # equal counts per grid: the mean over all N grids is the mean of the per-grid means
    return T


def identity_grid(sizes):
    gw, gh, gl = sizes
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12)
    return eye[:, None, None, None].expand(12, gl, gh, gw).contiguous()


def make_grid(sizes, seed):
    """[I | 0] + N(0, 0.3) noise, float32 [12, L, GH, GW]"""
    g = torch.Generator().manual_seed(4000 + seed)
    return (identity_grid(sizes) + 0.3 * torch.randn(identity_grid(sizes).shape, generator=g)).contiguous()


def dedicated_pixels(W, H):
    """flat pixel indices (black, white) of the pixels whose luminance is exactly 0 / exactly 1 (none in a tiny image)"""
    n = W * H
    if n < 16:
        return [], []
    return [0, 1, n // 2, n // 2 + 1], [2, 3, n // 2 + 2, n // 2 + 3]


def make_image(W, H, L, seed):
    """Colours in [-0.25, 1.25], CONSTRUCTED from a target luminance per pixel: about 3/4 of the pixels get
    l = (k + f) / (L - 1), k a random cell of the guide axis and f in [0.05, 0.95], so pz = k + f stays 0.05 away from
    every integer; the others get l in [-0.2, -0.02] or [1.02, 1.2] (both clamps live, 0.02 away from the ends).  The
    colour is l (1, 1, 1) plus a combination of two directions of zero luminance, so its luminance is l up to rounding.
    A dedicated set of pixels is exactly black and exactly white.  -> float32 [3, H, W]"""
    g = torch.Generator().manual_seed(7000 + 131 * W + 17 * H + L + seed)
    n = W * H
    kind = torch.rand(n, generator=g, dtype=torch.float64)
    k = torch.randint(0, L - 1, (n,), generator=g).double()
    f = 0.05 + 0.9 * torch.rand(n, generator=g, dtype=torch.float64)
    r = torch.rand(n, generator=g, dtype=torch.float64)
    lum = torch.where(kind < 0.75, (k + f) / (L - 1), torch.where(kind < 0.875, -0.2 + 0.18 * r, 1.02 + 0.18 * r))
    a, b = (0.16 * torch.rand(2, n, generator=g, dtype=torch.float64) - 0.08)
    d1 = torch.tensor([0.587, -0.299, 0.0], dtype=torch.float64)
    d2 = torch.tensor([0.0, 0.114, -0.587], dtype=torch.float64)
    c = lum[None, :] + a[None, :] * d1[:, None] + b[None, :] * d2[:, None]
    black, white = dedicated_pixels(W, H)
    c[:, black] = 0.0
    c[:, white] = torch.tensor(LUM_ONE, dtype=torch.float64)[:, None]
    return c.float().reshape(3, H, W).contiguous()


def make_gout(W, H, seed):
    g = torch.Generator().manual_seed(9000 + 31 * W + H + seed)
    return torch.randn(3, H, W, generator=g)


_CASES = {}


def case(name):
    """inputs and both references of one case, computed once and never modified: dict(image, grid, gout, W, H, sizes, band,
    r64, r32), r* = (x', grad_image, grad_grid) of the band's rows from slice_reference in fp64 / fp32"""
    if name in _CASES:
        return _CASES[name]
    _, W, H, sizes, band = next(c for c in CASES if c[0] == name)
    seed = [c[0] for c in CASES].index(name.replace("-band", ""))
    image, grid, gout = make_image(W, H, sizes[2], seed), make_grid(sizes, seed), make_gout(W, H, seed)
    y0, y1 = band if band is not None else (0, H)
    _CASES[name] = dict(image=image, grid=grid, gout=gout, W=W, H=H, sizes=sizes, y0=y0, y1=y1,
                        r64=slice_with_grads(slice_reference, image, grid, gout, torch.float64, y0, y1),
                        r32=slice_with_grads(slice_reference, image, grid, gout, torch.float32, y0, y1))
    return _CASES[name]
