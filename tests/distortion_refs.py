"""References for the depth distortion maps and their backward (grendel-gs_amd/csrc/distortion.hip): the arbiter that
include/gsraster.h names.  The cases of tests/composite_refs.py with invdepth_refs.depths_of(case) and g = dL_dpixels[0],
plus one family of its own, `far-thin`: single-tile lists of 3, 64, 65 and 130 entries (the chunk and batch boundaries of
the walk) with ascending depths in [50, 50.5] and mapping "depth" -- a depth spread of 1 % of the depth, where raw power
sums (sum w m^2 - (sum w m)^2 / sum w) lose every digit in float32.

`references(case, mapping)` -> (float64 results, float32 results) from the PAIRWISE Definition through autograd: per tile
w = alpha T as invdepth_refs.closed_form forms it (K8's n_contrib, the 0.99 clamp straight-through), D = 1/2 sum_ij w_i
w_j (m_i - m_j)^2 for all the tile's pixels at once (the matrix of squared differences does not depend on the pixel),
differentiated with respect to means2D, conic_opacity and depths with g = dL/dD.  Every term of the double sum is
non-negative and each difference is formed directly, so the float32 run is well conditioned where the depths are close:
it is the unit of helpers.assert_rows_close.  The totals A = sum w, mu = sum w m / A (0 where A = 0), S = sum w (m - mu)^2
(formed as the pairwise sum over A, the same number) are returned beside D.  `closed_form(case, mapping)` restates the
header's backward formulas (e, q, u) in float64 without autograd."""
import functools

import torch

import composite_refs as R
import invdepth_refs as IR

GROUPS = IR.GROUPS
MAPS = ["D", "A", "mu", "S"]
NEAR, FAR = 0.2, 1000.0
COEF = {"depth": (0.0, 1.0, 0.0), "inverse": (0.0, 0.0, 1.0),
        "ndc": (FAR / (FAR - NEAR), 0.0, -FAR * NEAR / (FAR - NEAR))}
FAR_THIN = [3, 64, 65, 130]
# K of helpers.assert_rows_close, per family: K[family of the case, or None][map or group].
# The maps start from composite_refs.K_FORWARD = 8 and keep it on every case of tests/composite_refs.py (worst measured
# 5.7).  The groups start from composite_refs.K_GROUP and invdepth_refs.K_GROUP["d_depth"]; three of them need more and
# are set to TWICE the worst ratio measured on an MI355X across those cases (d_means2D 27.8, d_opacity 55.4, d_depth 37.0;
# d_conic's 11.3 keeps its 12): the entry's "colour" e = A (m - mu)^2 + S is rebuilt per pixel from totals that were
# rounded to float32, and dot = e - rho cancels on top of that, where a colour is an input.
# `far-thin` has a K of its own, again twice the worst measured (D 300, S 413, d_means2D 151, d_conic 144, d_opacity 148,
# d_depth 367): the centred update works on m itself, so every m - mu carries the mean's float32 rounding, 2^-24 x 50,
# against a spread of 0.25 and less -- some hundred half-ulps, which the pairwise float32 reference (unit 4 to 8) does not
# have.  Raw power sums are off by more than the value there.  A and mu keep 8 everywhere.  EXPERIMENTS.md has the table.
K_MAP = {k: R.K_FORWARD for k in MAPS}
K_GROUP = {"d_means2D": 56, "d_conic": IR.K_GROUP["d_conic"], "d_opacity": 111, "d_depth": 74}
K_FAR_THIN = {"D": 600, "A": R.K_FORWARD, "mu": R.K_FORWARD, "S": 826, "d_means2D": 302, "d_conic": 288, "d_opacity": 296,
              "d_depth": 734}


def K_of(case, k):
    return K_FAR_THIN[k] if case.family == "far-thin" else {**K_MAP, **K_GROUP}[k]


def _far_thin_case(L):
    """composite_refs.lengths_case's splats (broad, soft, outside the tile, nobody saturates), every row listed"""
    gen = R._gen(900 + L)
    amax = min(0.3, 4.0 / L)
    m, c, o, rgb = R._soft(gen, L, (2.0, 2.0), (8.0, 8.0), (8.0, 16.0), (0.25 * amax, amax))
    return R.Case("far-thin", str(L), 16, 16, R._outside(gen, m), c, o, rgb, [0.0, 0.0, 0.0], [True],
                  [torch.randperm(L, generator=gen)], 900 + L)


@functools.lru_cache(maxsize=None)
def cases():
    return R.cases() + tuple(_far_thin_case(L) for L in FAR_THIN)


def mapping_of(case):
    """every case runs with m = depth (exact in float32: no rounding of m enters the unit); the two mappings that divide
    run on MAPPING_CASE, a deep case on which the float32 reference stays under helpers.ROW_UNIT_CAP with them"""
    return "depth"


MAPPING_CASE = "deep-256"


@functools.lru_cache(maxsize=None)
def depths_of(case):
    if case.id == "saturating-a":
        # invdepth_refs' depths put the float32 reference's d_opacity at 7788 x 2^-24 of a row, over the cap (one row whose
        # pixels cancel); the same recipe with another seed: 183 at most
        u = torch.rand(case.P, generator=R._gen(7101), dtype=torch.float64)
        d = (IR.DEPTH_LO + (IR.DEPTH_HI - IR.DEPTH_LO) * u).to(torch.float32)
        d[case.lists[0]] = torch.sort(d[case.lists[0]]).values
        return d
    if case.family != "far-thin":
        return IR.depths_of(case)
    u = torch.rand(case.P, generator=R._gen(7000 + case.seed), dtype=torch.float64)
    d = torch.empty(case.P, dtype=torch.float32)
    d[case.lists[0]] = torch.sort(50.0 + 0.5 * u).values.to(torch.float32)  # ascending along the list
    return d


def measure(depth, mapping):
    c0, c1, c2 = COEF[mapping]
    return c0 + c1 * depth + c2 / depth


def _tiles(case, m2, co, dep, mapping):
    """per local tile with a list: (ids, box, dx, dy [L, npx], G, araw, take, T in front of the entry, w, m [L, 1])"""
    nc = R.references(case)[0]["n_contrib"]
    dt = m2.dtype
    for t in range(case.tiles):
        ids = case.lists[t]
        if not bool(case.compute_locally[t]) or ids.numel() == 0:
            continue
        x0, y0, x1, y1 = box = case.tile_box(t)
        py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        last = nc[y0:y1, x0:x1].reshape(-1).to(torch.int64)
        xy, con = m2[ids], co[ids]
        dx, dy = xy[:, 0:1] - px.reshape(-1).to(dt)[None, :], xy[:, 1:2] - py.reshape(-1).to(dt)[None, :]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        G = torch.exp(torch.clamp(power, max=0.0))
        araw = con[:, 3:4] * G
        alpha = araw + (torch.clamp(araw, max=0.99) - araw).detach()  # the clamp is the identity in the backward
        take = (torch.arange(1, ids.numel() + 1)[:, None] <= last[None, :]) & (power <= 0) & (alpha >= R.ALPHA_MIN)
        a = torch.where(take, alpha, torch.zeros_like(alpha))
        T_behind = torch.cumprod(1.0 - a, dim=0)
        T = torch.cat([torch.ones_like(T_behind[:1]), T_behind[:-1]], dim=0)
        yield ids, box, dx, dy, G, araw, take, a, T, a * T, measure(dep[ids], mapping)[:, None]


def _render(case, mapping, dtype):
    m2 = case.means2D.clone().to(dtype).requires_grad_(True)
    co = case.conic_opacity.clone().to(dtype).requires_grad_(True)
    dep = depths_of(case).clone().to(dtype).requires_grad_(True)
    maps = {k: torch.zeros(case.H, case.W, dtype=dtype) for k in MAPS}
    blended = torch.zeros(case.P, dtype=torch.bool)
    loss = torch.zeros((), dtype=dtype)
    gmap = IR.g_of(case).to(dtype)
    for ids, (x0, y0, x1, y1), dx, dy, G, araw, take, a, T, w, m in _tiles(case, m2, co, dep, mapping):
        M = (m - m.T) ** 2                                   # [L, L]: the pairwise squared differences
        D = 0.5 * (w * (M @ w)).sum(dim=0)
        loss = loss + (D * gmap[y0:y1, x0:x1].reshape(-1)).sum()
        wd = w.detach()
        A = wd.sum(dim=0)
        mu = torch.where(A > 0, (wd * m.detach()).sum(dim=0) / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
        # S = sum w (m - mu)^2 = (1/2 sum_ij w_i w_j (m_i - m_j)^2) / A: the pairwise side of the identity, which float32
        # keeps where (m - mu)^2 about a float32 mean does not
        S = torch.where(A > 0, D.detach() / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
        for k, v in zip(MAPS, (D.detach(), A, mu, S)):
            maps[k][y0:y1, x0:x1] = v.view(y1 - y0, x1 - x0)
        blended[ids] |= take.any(dim=1)
    if loss.requires_grad:
        g = torch.autograd.grad(loss, [m2, co, dep], allow_unused=True)
        g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (m2, co, dep))]
    else:
        g = [torch.zeros_like(m2), torch.zeros_like(co), torch.zeros_like(dep)]
    out = {k: v.reshape(-1, 1) for k, v in maps.items()}
    ndc = torch.tensor([0.5 * case.W, 0.5 * case.H], dtype=dtype)  # means2D gradients in K10's units: pixel gradient x (W/2, H/2)
    out.update(n_contrib=R.references(case)[0]["n_contrib"], blended=blended, d_means2D=g[0].detach() * ndc,
               d_conic=g[1][:, :3].contiguous(), d_opacity=g[1][:, 3:].contiguous(), d_depth=g[2].reshape(-1, 1))
    return out


@functools.lru_cache(maxsize=None)
def references(case, mapping=None):
    """-> (float64 results, float32 results); computed once per (case, mapping) and never modified"""
    mapping = mapping or mapping_of(case)
    return _render(case, mapping, torch.float64), _render(case, mapping, torch.float32)


split_record = IR.split_record


def closed_form(case, mapping=None):
    """the backward of include/gsraster.h in float64, no autograd: e = A (m - mu)^2 + S, q = alpha_raw g (T e - R / (1 -
    alpha)), u = 2 g w A (m - mu) -> the four gradient groups"""
    mapping = mapping or mapping_of(case)
    dt = torch.float64
    m2, co, dep = case.means2D.to(dt), case.conic_opacity.to(dt), depths_of(case).to(dt)
    c0, c1, c2 = COEF[mapping]
    gmap = IR.g_of(case).to(dt)
    d2, dcon = torch.zeros(case.P, 2, dtype=dt), torch.zeros(case.P, 3, dtype=dt)
    dop, dm = torch.zeros(case.P, 1, dtype=dt), torch.zeros(case.P, dtype=dt)
    for ids, (x0, y0, x1, y1), dx, dy, G, araw, take, a, T, w, m in _tiles(case, m2, co, dep, mapping):
        g = gmap[y0:y1, x0:x1].reshape(-1)[None, :]
        A = w.sum(dim=0, keepdim=True)
        mu = torch.where(A > 0, (w * m).sum(dim=0, keepdim=True) / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
        S = (w * (m - mu) ** 2).sum(dim=0, keepdim=True)
        e = A * (m - mu) ** 2 + S
        we = w * e
        behind = torch.flip(torch.cumsum(torch.flip(we, [0]), dim=0), [0]) - we
        dLda = torch.where(take, g * (T * e - behind / (1.0 - a)), torch.zeros_like(a))
        q = dLda * araw
        dm.index_add_(0, ids, (2.0 * g * w * A * (m - mu)).sum(dim=1))
        dop.index_add_(0, ids, (dLda * G).sum(dim=1, keepdim=True))
        cA, cB, cC = co[ids][:, 0:1], co[ids][:, 1:2], co[ids][:, 2:3]
        d2.index_add_(0, ids, torch.stack([-(q * (cA * dx + cB * dy)).sum(dim=1) * (0.5 * case.W),
                                           -(q * (cB * dx + cC * dy)).sum(dim=1) * (0.5 * case.H)], dim=1))
        dcon.index_add_(0, ids, torch.stack([-0.5 * (q * dx * dx).sum(dim=1), -(q * dx * dy).sum(dim=1),
                                             -0.5 * (q * dy * dy).sum(dim=1)], dim=1))
    safe = torch.where(dm != 0, dep, torch.ones_like(dep))
    return dict(d_means2D=d2, d_conic=dcon, d_opacity=dop, d_depth=((c1 - c2 / (safe * safe)) * dm).reshape(-1, 1))
