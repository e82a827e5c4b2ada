"""References for the surfel geometry pass and its backward (grendel-gs_amd/csrc/surfels.hip): the arbiter that
include/gsraster.h names.  The cases of tests/distortion_refs.py with distortion_refs.depths_of(case) as the rows' z, plus
one family of its own, `median`, one 16 x 16 tile each: a first entry that already crosses 0.5 (`first`), a final_T above
0.5 (`open`: the median is the last taken entry), a crossing entry at list position 64 / 65 (`cross-64`, `cross-65`: slot
8 of a batch, the first slot behind a chunk), and `mixed`, whose normals tilt either way so that the blended N crosses
zero over the tile (its N maps are compared map-wise, test_gpu_surfel_pixels.py).  One seeded draw per case adds unit
normals facing the camera, dL/dsurfel [5,H,W] and dL/dmedian [H,W]; dL/ddist = invdepth_refs.g_of(case).

`references(case, mapping)` -> (float64, float32 results) in plain torch over the explicit lists: w = alpha T as
distortion_refs._tiles forms it, A = sum w, D = sum w z, N = sum w n, the PAIRWISE distortion, and the median by the
header's rule.  Gradients by autograd of sum_p g . (A, D, N, Dist, med): the median is a gather of z, so its gradient
is the scatter of dL/dmedian into the chosen entry's z.  The float32 run is the unit of helpers.assert_rows_close.

NEAR pixels: some taken entry's front transmittance lies within 2^-10 (relative) of 0.5 in float64, so the inputs do not
settle the median entry.  `near` marks them and `near_rows` the rows whose dL/dz they could feed (the chosen entry, the
near entries, the taken entry in front of the first of them); they are left out of the med / median_pos and the d_z
comparisons only.  At most NEAR_CAP of a case's blended pixels may be near; the cases above it are named in OVER_CAP
(tests/test_surfel_refs_cpu.py: exactly those)."""
import functools

import torch

import composite_refs as R
import distortion_refs as DR
import features_refs as FR

COEF, depths_of, MAPPING_CASE = DR.COEF, DR.depths_of, DR.MAPPING_CASE
MAPS = ["A", "D", "N0", "N1", "N2", "Dist", "mu", "S", "med"]
GROUPS = ["d_means2D", "d_conic", "d_opacity", "d_z", "d_n"]
NEAR_REL = 2.0 ** -10
NEAR_CAP = 0.02
# The cases over NEAR_CAP, by id; the cap is never raised.  Lists of many thin entries: with alpha 0.01 .. 0.05, T passes
# 0.5 in steps of 0.005 .. 0.03 and the window catches 2.3 .. 18.4 % of the pixels (EXPERIMENTS.md has each figure).  They
# do not count as evidence for the median rule -- the other cases hold it -- but their far pixels are compared like any.
OVER_CAP = {"lengths-63", "lengths-64", "lengths-65", "lengths-127", "lengths-128", "lengths-129", "deep-255", "deep-256",
            "deep-512", "deep-513", "deep-600", "deep-long", "saturating-a", "far-thin-64", "far-thin-65", "far-thin-130"}


def K_of(case, k):
    """the project's figures for the summands, nothing minted here: the forward maps keep composite_refs.K_FORWARD, Dist
    and S distortion_refs' K; a gradient group takes the larger of distortion_refs' and features_refs' K for it"""
    if k in ("Dist", "S"):
        return DR.K_of(case, "D" if k == "Dist" else "S")
    if k in MAPS:
        return R.K_FORWARD
    if k == "d_n":
        return FR.K_GROUP["d_features"]
    if k == "d_z":
        return max(DR.K_of(case, "d_depth"), FR.K_GROUP["d_features"])
    return max(DR.K_of(case, k), FR.K_GROUP[k])


def _median_case(name, seed, L, cross):
    """deep_case's very broad splats outside the tile: alpha is 0.65 .. 1 of the opacity on every pixel.  Thin entries
    (alpha 0.005 .. 0.0085) and, at list position `cross` (1-based), one of opacity 0.9"""
    gen = R._gen(seed)
    m, c, o, rgb = R._soft(gen, L, (2.0, 2.0), (10.0, 10.0), (40.0, 90.0), (0.0077, 0.0085))
    lst = torch.randperm(L, generator=gen)
    if cross:
        o[lst[cross - 1]] = 0.9
    return R.Case("median", name, 16, 16, R._outside(gen, m), c, o, rgb, [0.0, 0.0, 0.0], [True], [lst], seed)


def _mixed_case(seed=955):
    """twelve narrow splats INSIDE the tile: the weights differ from pixel to pixel, so the blended normal turns"""
    gen = R._gen(seed)
    m, c, o, rgb = R._soft(gen, 12, (0.0, 0.0), (16.0, 16.0), (3.0, 6.0), (0.2, 0.7))
    return R.Case("median", "mixed", 16, 16, m, c, o, rgb, [0.0, 0.0, 0.0], [True], [torch.randperm(12, generator=gen)], seed)


@functools.lru_cache(maxsize=None)
def cases():
    return DR.cases() + (_median_case("first", 951, 5, 1), _median_case("open", 952, 4, 0),
                         _median_case("cross-64", 953, 70, 64), _median_case("cross-65", 954, 70, 65),
                         _mixed_case())


@functools.lru_cache(maxsize=None)
def draw(case):
    """-> (rows [P,5] = (1, z, n), dL/dsurfel [5,H,W], dL/ddist [H,W], dL/dmedian [H,W]), float32, never modified"""
    # (offtile-mid: the first draw put the float32 reference's d_z at 4140 x 2^-24 of a row, over helpers.ROW_UNIT_CAP)
    gen = R._gen((8100 if case.id == "offtile-mid" else 8000) + case.seed)
    # (tilted one way: a component whose blend crosses zero over the pixels would put the float32 unit over its cap)
    n = torch.cat([0.1 + 0.4 * torch.rand(case.P, 2, generator=gen), -torch.ones(case.P, 1)], dim=1).double()
    if case.id == "median-mixed":
        n[:, :2] *= torch.where(torch.rand(case.P, 2, generator=gen) < 0.5, -1.0, 1.0)
    n = (n / n.norm(dim=1, keepdim=True)).float()
    rows = torch.cat([torch.ones(case.P, 1), depths_of(case).reshape(-1, 1), n], dim=1).contiguous()
    g_s = torch.rand(5, case.H, case.W, generator=gen)
    g_med = torch.rand(case.H, case.W, generator=gen)
    return rows, g_s, DR.IR.g_of(case), g_med


def _render(case, mapping, dtype):
    rows0, g_s, g_dist, g_med = (t.to(dtype) for t in draw(case))
    m2 = case.means2D.clone().to(dtype).requires_grad_(True)
    co = case.conic_opacity.clone().to(dtype).requires_grad_(True)
    rows = rows0.clone().requires_grad_(True)
    dep = rows[:, 1]
    maps = {k: torch.zeros(case.H, case.W, dtype=dtype) for k in MAPS}
    medpos = torch.zeros(case.H, case.W, dtype=torch.int32)
    near = torch.zeros(case.H, case.W, dtype=torch.bool)
    blended, near_rows = torch.zeros(case.P, dtype=torch.bool), torch.zeros(case.P, dtype=torch.bool)
    loss = torch.zeros((), dtype=dtype)
    for ids, (x0, y0, x1, y1), dx, dy, G, araw, take, a, T, w, m in DR._tiles(case, m2, co, dep, mapping):
        L, shape = ids.numel(), (y1 - y0, x1 - x0)
        z, n = dep[ids][:, None], rows[ids, 2:5]
        A, D, N = w.sum(dim=0), (w * z).sum(dim=0), w.T @ n
        Dist = 0.5 * (w * (((m - m.T) ** 2) @ w)).sum(dim=0)
        # the median: the last taken entry with T > 0.5 in front of it (0-based index, -1: the pixel blends nothing)
        front = take & (T.detach() > 0.5)
        pos = torch.where(front.any(dim=0), L - 1 - torch.flip(front, [0]).to(torch.int64).argmax(dim=0),
                          torch.full_like(front[0], -1, dtype=torch.int64))
        med = torch.where(pos >= 0, z[:, 0][pos.clamp(min=0)], torch.zeros_like(A))
        gs = g_s[:, y0:y1, x0:x1].reshape(5, -1)
        loss = loss + (gs[0] * A + gs[1] * D + (gs[2:5].T * N).sum(dim=1) + g_dist[y0:y1, x0:x1].reshape(-1) * Dist
                       + g_med[y0:y1, x0:x1].reshape(-1) * med).sum()
        Ad, wd = A.detach(), w.detach()
        one = torch.ones_like(Ad)
        mu = torch.where(Ad > 0, (wd * m.detach()).sum(dim=0) / torch.where(Ad > 0, Ad, one), torch.zeros_like(Ad))
        S = torch.where(Ad > 0, Dist.detach() / torch.where(Ad > 0, Ad, one), torch.zeros_like(Ad))  # (distortion_refs' reason)
        for k, v in zip(MAPS, (Ad, D, N[:, 0], N[:, 1], N[:, 2], Dist, mu, S, med)):
            maps[k][y0:y1, x0:x1] = v.detach().view(shape)
        medpos[y0:y1, x0:x1] = (pos + 1).to(torch.int32).view(shape)
        nk = take & ((T.detach() - 0.5).abs() <= NEAR_REL * 0.5)
        near[y0:y1, x0:x1] = nk.any(dim=0).view(shape)
        for p in nk.any(dim=0).nonzero().reshape(-1).tolist():  # (few pixels, if any)
            k0 = int(nk[:, p].to(torch.int64).argmax())
            before = take[:k0, p].nonzero().reshape(-1)
            cand = nk[:, p].nonzero().reshape(-1).tolist() + [int(pos[p])] + before[-1:].tolist()
            near_rows[ids[[c for c in cand if c >= 0]]] = True
        blended[ids] |= take.any(dim=1)
    if loss.requires_grad:
        g = torch.autograd.grad(loss, [m2, co, rows], allow_unused=True)
        g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (m2, co, rows))]
    else:
        g = [torch.zeros_like(m2), torch.zeros_like(co), torch.zeros_like(rows)]
    out = {k: v.reshape(-1, 1) for k, v in maps.items()}
    ndc = torch.tensor([0.5 * case.W, 0.5 * case.H], dtype=dtype)  # means2D gradients in K10's units
    out.update(n_contrib=R.references(case)[0]["n_contrib"], blended=blended, median_pos=medpos.reshape(-1),
               near=near.reshape(-1), near_rows=near_rows, d_means2D=g[0].detach() * ndc,
               d_conic=g[1][:, :3].contiguous(), d_opacity=g[1][:, 3:].contiguous(), d_z=g[2][:, 1:2].contiguous(),
               d_n=g[2][:, 2:5].contiguous())
    return out


@functools.lru_cache(maxsize=None)
def references(case, mapping="depth"):
    """-> (float64 results, float32 results); computed once per (case, mapping) and never modified"""
    return _render(case, mapping, torch.float64), _render(case, mapping, torch.float32)


def near_fraction(case, mapping="depth"):
    """near pixels / blended pixels of the case in float64 (0 when it blends nothing)"""
    r64 = references(case, mapping)[0]
    seen = int((r64["A"].reshape(-1) > 0).sum())
    return float(r64["near"].sum()) / seen if seen else 0.0


def split_records(rec, drows):
    """dL_record [P,6] and dL_rows [P,5] -> the five gradient groups"""
    return dict(d_means2D=rec[:, 0:2], d_conic=rec[:, 2:5], d_opacity=rec[:, 5:6], d_z=drows[:, 1:2], d_n=drows[:, 2:5])
