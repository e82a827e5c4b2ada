"""Plain torch restatements of the two definitions of include/gsraster.h's depth-normal consistency section, with autograd:
run in float64 they are the arbiter of tests/test_gpu_normals.py, run in float32 (the same code) the yardstick of
helpers.assert_rows_close.  Nothing here comes from the code under test."""
import torch


def rows_ref(xyz, scaling, rotation, radii, V):
    """(a) the surfel rows [P,5] = (1, t_z, n), in the dtype of xyz; V: the 4 x 4 view matrix, t = [p, 1] V"""
    V = V.to(xyz.dtype)
    P = xyz.shape[0]
    t = xyz @ V[:3, :3] + V[3, :3]
    k = scaling.argmin(dim=1)
    q = rotation / rotation.norm(dim=1, keepdim=True).clamp(min=1e-12)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(P, 3, 3)
    a_c = R[torch.arange(P), :, k] @ V[:3, :3]
    sigma = torch.where((a_c * t).sum(1) > 0, -1.0, 1.0).to(xyz.dtype).detach()
    rows = torch.cat([torch.ones_like(t[:, :1]), t[:, 2:3], sigma[:, None] * a_c], dim=1)
    return torch.where((radii > 0)[:, None], rows, torch.zeros_like(rows))


def consistency_ref(F, tanfovx, tanfovy, weight):
    """(b) -> (loss, n_d [3,H,W]) of the [5,H,W] map F = (A, D, N), in the dtype of F"""
    dt = F.dtype
    H, W = F.shape[1:]
    A, D, N = F[0], F[1], F[2:5]
    ok = A > 1e-6
    z = torch.where(ok, D / torch.where(ok, A, torch.ones_like(A)), torch.zeros_like(A))
    rx = ((2 * torch.arange(W, dtype=dt) + 1) / W - 1) * tanfovx
    ry = ((2 * torch.arange(H, dtype=dt) + 1) / H - 1) * tanfovy
    X = torch.stack([z * rx[None, :], z * ry[:, None], z])
    dx = X[:, 1:-1, 2:] - X[:, 1:-1, :-2]
    dy = X[:, 2:, 1:-1] - X[:, :-2, 1:-1]
    c = torch.cross(dy, dx, dim=0)
    l2 = (c * c).sum(0)
    good = l2 > 1e-24
    n = torch.where(good, c / torch.sqrt(torch.where(good, l2, torch.ones_like(l2))), torch.zeros_like(c))
    e = 1 - A.detach()[1:-1, 1:-1] * (N[:, 1:-1, 1:-1] * n).sum(0)
    n_d = torch.zeros(3, H, W, dtype=dt)
    n_d[:, 1:-1, 1:-1] = n.detach()
    return weight / (H * W) * e.sum(), n_d


def surfel_inputs(P, V, seed):
    """float32 (xyz, scaling, rotation, radii) of P rows whose two decisions keep a margin by construction: the two
    smallest log-scales differ by log 1.5 or more and the minimum sits at i % 3; |a_c . t| is between 0.15 and 0.9 of
    |t|, its sign alternating; |q| runs from 0.3 to 3; every fifth row (not the first) has radii 0"""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(P)
    scaling = -1 - 2 * torch.rand(P, 3, generator=g, dtype=torch.float64)
    scaling[i, i % 3] = scaling.min(dim=1).values - 0.41 - 0.5 * torch.rand(P, generator=g, dtype=torch.float64)
    q = torch.randn(P, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True) * (0.3 + 2.7 * torch.rand(P, 1, generator=g, dtype=torch.float64))
    scaling, q = scaling.float(), q.float()
    radii = torch.where(i % 5 == 4, 0, 3).to(torch.int32)
    # the axis in camera space (either sign), from the rounded inputs; then t at a chosen angle to it
    V64 = V.double()
    a = rows_ref(torch.zeros(P, 3, dtype=torch.float64), scaling.double(), q.double(), torch.ones(P), V64)[:, 2:5]
    w = torch.randn(P, 3, generator=g, dtype=torch.float64)
    perp = w - a * (w * a).sum(1, keepdim=True)
    perp = perp / perp.norm(dim=1, keepdim=True)
    cos = (0.15 + 0.75 * torch.rand(P, 1, generator=g, dtype=torch.float64)) * torch.where(i % 2 == 0, 1.0, -1.0)[:, None]
    t = (2 + 6 * torch.rand(P, 1, generator=g, dtype=torch.float64)) * (cos * a + torch.sqrt(1 - cos * cos) * perp)
    xyz = ((t - V64[3, :3]) @ torch.linalg.inv(V64[:3, :3])).float()
    return xyz, scaling, q, radii


def surfel_map(W, H, holes, seed, tile):
    """float32 [5,H,W] = (A, D, N): a tilted plane with 5 % noise in z, A in [0.3, 1], N = A x a random unit vector;
    `holes`: a block of up to 5 x 5 (3 x 3 at least where the image allows) of A = D = N = 0 across the first tile
    boundary in x and y"""
    g = torch.Generator().manual_seed(seed)
    u = (torch.arange(W, dtype=torch.float64) + 0.5) / W * 2 - 1
    v = (torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1
    z = (3 + 0.4 * u[None, :] + 0.3 * v[:, None]) * (1 + 0.05 * (2 * torch.rand(H, W, generator=g, dtype=torch.float64) - 1))
    A = 0.3 + 0.7 * torch.rand(H, W, generator=g, dtype=torch.float64)
    n = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    F = torch.cat([A[None], (A * z)[None], A[None] * n / n.norm(dim=0, keepdim=True)]).float()
    if holes:
        x0, y0 = max(0, min(W, tile[0]) - 3), max(0, min(H, tile[1]) - 3)
        F[:, y0:y0 + 5, x0:x0 + 5] = 0
    return F
