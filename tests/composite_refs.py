"""Seeded cases and references for the composite pair K8 / K10 (grendel-gs_amd/csrc/composite.hip) on EXPLICIT lists.

A case is what gsr_render_forward / gsr_render_backward take: the frame, the per-Gaussian rows (means2D, conic_opacity,
rgb), the background, the tile mask, one list of distinct Gaussian ids per tile (point_list + ranges, the last row of
`ranges` the row hull of the local tiles) and dL/dpixels.  No binning and no projection stand between these inputs and
the result.  Every float is fp32-representable, so the float64 arbiter and the float32 unit see the same numbers.

References (`references(case)` -> (r64, r32)): oracle.torch_oracle.render on the case's lists, once in float64 (the
arbiter) and once in float32 (the unit of helpers.assert_rows_close: the reference's own fp32 error, never a kernel's),
differentiated by autograd.  `cref_results(case)` is the independent plain-fp32 C restatement on the same lists.

Keeping away from the decisions.  The blend takes two discrete decisions per (pixel, entry): alpha >= 1/255 and
T (1 - alpha) >= 1e-4.  `decisions(case, dtype)` restates them as r_a = 255 o exp(power) and r_T = test_T / 1e-4; every
case is settled (`_settle`: the offending Gaussian's opacity is multiplied by 1 - 3 m, a bounded number of times) until
|r_a - 1| >= m and |r_T - 1| >= m, m = 2^-10, on everything the float64 reference evaluates.  m is a condition on the
INPUTS, not a tolerance on a kernel; tests/test_composite_refs_cpu.py checks it on every case."""
import functools
import math

import torch

from oracle import cref as C
from oracle import torch_oracle as O

M = 2.0 ** -10            # margin of the inputs around the two decisions
ALPHA_MIN = 1.0 / 255.0
T_STOP = 0.0001
SEG_LEN, SEG_MAXJ = 256, 16   # composite.hip: a checkpoint every 256 walked entries, at most 16 boundaries carry one
GROUPS = ["d_means2D", "d_conic", "d_opacity", "d_rgb"]
# K of helpers.assert_rows_close.  8 is the project's value (the leaf and projection files use it) and holds for the image,
# final_T and d_rgb.  The other three groups are bounded by twice the worst ratio of the CPU emulation of K10's order of
# operations run AS WRITTEN (`k10_emulation` with nothing moved: 7.66, 6.69 and 5.10 on these cases), rounded down with a
# little room for another machine's float32: tests/test_composite_refs_cpu.py recomputes the emulation and asserts
# K <= min(16, 2 * worst).  EXPERIMENTS.md says where the kernel is above 8 and what the emulation does not show.
K_FORWARD = 8
K_GROUP = {"d_means2D": 14, "d_conic": 12, "d_opacity": 9.5, "d_rgb": 8}
TENSORS = ["image", "final_T"] + GROUPS


def _f32(t):
    return t.to(torch.float32).contiguous()


def conics(sx, sy, theta):
    """inverse of R diag(sx^2, sy^2) R^T, rows (A, B, C): positive definite with margin for the aspect ratios used here"""
    c, s = torch.cos(theta), torch.sin(theta)
    ia, ib = 1.0 / (sx * sx), 1.0 / (sy * sy)
    return torch.stack([c * c * ia + s * s * ib, c * s * (ia - ib), s * s * ia + c * c * ib], dim=1)


class Case:
    def __init__(self, family, name, W, H, means2D, conic, opacity, rgb, bg, mask, lists, seed, band=None):
        self.family, self.name, self.id = family, name, f"{family}-{name}"
        self.W, self.H = W, H
        self.gx, self.gy = (W + 15) // 16, (H + 15) // 16
        self.tiles = self.gx * self.gy
        self.P = means2D.shape[0]
        self.means2D = _f32(means2D.reshape(-1, 2))
        self.conic_opacity = _f32(torch.cat([conic.reshape(-1, 3), opacity.reshape(-1, 1)], dim=1))
        self.rgb = _f32(rgb.reshape(-1, 3))
        self.bg = _f32(torch.as_tensor(bg))
        self.compute_locally = torch.as_tensor(mask, dtype=torch.bool).reshape(-1)
        assert self.compute_locally.numel() == self.tiles and len(lists) == self.tiles
        self.lists = [torch.as_tensor(l, dtype=torch.int64).reshape(-1) for l in lists]
        for l in self.lists:  # distinct ids, as binning guarantees
            assert l.numel() == torch.unique(l).numel() and (l.numel() == 0 or (0 <= int(l.min()) and int(l.max()) < self.P))
        self.point_list = torch.cat(self.lists) if self.lists else torch.zeros(0, dtype=torch.int64)
        ends = torch.cumsum(torch.tensor([l.numel() for l in self.lists]), 0)
        starts = ends - torch.tensor([l.numel() for l in self.lists])
        rows = self.compute_locally.view(self.gy, self.gx).any(dim=1).nonzero().reshape(-1)
        hull = (int(rows.min()), int(rows.max()) + 1) if rows.numel() else (0, 0)
        self.hull = hull
        self.ranges = torch.cat([torch.stack([starts, ends], dim=1), torch.tensor([hull])]).to(torch.int64)
        self.band = band  # (row_lo, row_hi) when the mask is a proper row band, else None
        self.dL_dpixels = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1000 + seed))
        self.seed = seed
        _settle(self)

    def __repr__(self):
        return self.id

    def tile_box(self, t):
        ty, tx = divmod(t, self.gx)
        return tx * 16, ty * 16, min(tx * 16 + 16, self.W), min(ty * 16 + 16, self.H)


# ------------------------------------------------------------------------------------------------ decisions
def decisions(case, dtype=torch.float64):
    """per local tile with a non-empty list, in the arithmetic of oracle.torch_oracle.render: dict(tile, ids, r_a, r_T
    [L, npx], evaluated (entries up to and including the pixel's stop), tested (evaluated and not skipped: a test_T is
    formed), blended, clamped (o exp(power) > 0.99 on a blended pair), stop_idx [npx])"""
    m2, co = case.means2D.to(dtype), case.conic_opacity.to(dtype)
    out = []
    for t in range(case.tiles):
        ids = case.lists[t]
        L = ids.numel()
        if not bool(case.compute_locally[t]) or L == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        pxf, pyf = px.reshape(-1).to(dtype), py.reshape(-1).to(dtype)
        xy, con = m2[ids], co[ids]
        dx, dy = xy[:, 0:1] - pxf[None, :], xy[:, 1:2] - pyf[None, :]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        araw = con[:, 3:4] * torch.exp(torch.clamp(power, max=0.0))
        alpha = torch.clamp(araw, max=0.99)
        skip = (power > 0) | (alpha < ALPHA_MIN)
        a_eff = torch.where(skip, torch.zeros_like(alpha), alpha)
        test_T = torch.cumprod(1.0 - a_eff, dim=0)
        stopped = test_T < T_STOP
        npx = pxf.numel()
        stop_idx = torch.where(stopped.any(dim=0), stopped.to(torch.int64).argmax(dim=0),
                               torch.full((npx,), L, dtype=torch.int64))
        ar = torch.arange(L)[:, None]
        evaluated = ar <= stop_idx[None, :]
        tested = evaluated & ~skip
        blended = (ar < stop_idx[None, :]) & ~skip
        out.append(dict(tile=t, ids=ids, r_a=255.0 * araw, r_T=test_T / T_STOP, evaluated=evaluated, tested=tested,
                        blended=blended, clamped=blended & (araw > 0.99), stop_idx=stop_idx, L=L))
    return out


def margins(case):
    """-> dict: gap_a / gap_T (the smallest |r - 1| the float64 reference meets), dev_a / dev_T (the float32 reference's
    largest deviation from float64, relative to the larger of the value and the threshold 1: what could move a value
    across the threshold), same (both precisions take the same decisions on every evaluated pair)"""
    d64, d32 = decisions(case, torch.float64), decisions(case, torch.float32)
    r = dict(gap_a=math.inf, gap_T=math.inf, dev_a=0.0, dev_T=0.0, same=True)
    for a, b in zip(d64, d32):
        ev, te = a["evaluated"], a["tested"]
        r["same"] &= bool(torch.equal(ev, b["evaluated"]) and torch.equal(te, b["tested"]) and
                          torch.equal(a["blended"], b["blended"]) and torch.equal(a["stop_idx"], b["stop_idx"]))
        if bool(ev.any()):
            r["gap_a"] = min(r["gap_a"], float((a["r_a"][ev] - 1).abs().min()))
            r["dev_a"] = max(r["dev_a"], float(((b["r_a"].double() - a["r_a"]).abs() / a["r_a"].clamp(min=1.0))[ev].max()))
        if bool(te.any()):
            r["gap_T"] = min(r["gap_T"], float((a["r_T"][te] - 1).abs().min()))
            r["dev_T"] = max(r["dev_T"], float(((b["r_T"].double() - a["r_T"]).abs() / a["r_T"].clamp(min=1.0))[te].max()))
    return r


def _settle(case, attempts=24):
    """multiply the opacity of every Gaussian that owns a pair inside the margin by 1 - 3 m (rounded to float32) until no
    pair is; raises when that does not converge"""
    for _ in range(attempts):
        bad = set()
        for d in decisions(case, torch.float64):
            near = (d["evaluated"] & ((d["r_a"] - 1).abs() < 2 * M)) | (d["tested"] & ((d["r_T"] - 1).abs() < 2 * M))
            bad.update(d["ids"][near.any(dim=1)].tolist())
        if not bad:
            return
        idx = torch.tensor(sorted(bad))
        case.conic_opacity[idx, 3] = (case.conic_opacity[idx, 3].double() * (1.0 - 3.0 * M)).float()
    raise RuntimeError(f"{case.id}: the inputs do not settle away from the decisions: change the seed")


# ------------------------------------------------------------------------------------------------ references
def _render(case, dtype):
    m2 = case.means2D.clone().to(dtype).requires_grad_(True)  # (clone: .to() of a float32 tensor is the tensor itself)
    co = case.conic_opacity.clone().to(dtype).requires_grad_(True)
    rgb = case.rgb.clone().to(dtype).requires_grad_(True)
    img, fT, nc = O.render(m2, co, rgb, None, None, case.compute_locally, bg=case.bg.to(dtype), W=case.W, H=case.H,
                           binning=(case.point_list, case.ranges[:case.tiles], None))
    if img.requires_grad and case.P > 0:
        g = torch.autograd.grad((img * case.dL_dpixels.to(dtype)).sum(), [m2, co, rgb], allow_unused=True)
        g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (m2, co, rgb))]
    else:
        g = [torch.zeros_like(m2), torch.zeros_like(co), torch.zeros_like(rgb)]
    HW = case.H * case.W
    return dict(image=img.detach().reshape(3, HW).t().contiguous(), final_T=fT.reshape(HW, 1), n_contrib=nc,
                d_means2D=g[0], d_conic=g[1][:, :3].contiguous(), d_opacity=g[1][:, 3:].contiguous(), d_rgb=g[2])


@functools.lru_cache(maxsize=None)
def references(case):
    """-> (float64 results, float32 results); computed once per case and never modified"""
    return _render(case, torch.float64), _render(case, torch.float32)


def split_record(rec):
    """[P,9] record -> the four gradient groups (columns: 0:2 means2D, 2:5 rgb, 5:8 conic, 8 opacity)"""
    return dict(d_means2D=rec[:, 0:2], d_rgb=rec[:, 2:5], d_conic=rec[:, 5:8], d_opacity=rec[:, 8:9])


def as_rows(img, fT):
    """[3,H,W] image and [H,W] final_T -> [H*W,3] and [H*W,1]"""
    return img.reshape(3, -1).t().contiguous(), fT.reshape(-1, 1)


@functools.lru_cache(maxsize=None)
def cref_results(case):
    """the C restatement (plain fp32) on the case's lists -> the same dict as `references`"""
    pl = case.point_list.to(torch.int32)
    rg = case.ranges[:case.tiles].to(torch.int32).contiguous()
    img, fT, nc = C.render_forward(case.means2D, case.conic_opacity, case.rgb, case.compute_locally, case.bg, case.W,
                                   case.H, pl, rg)
    out = dict(n_contrib=nc)
    out["image"], out["final_T"] = as_rows(img, fT)
    if case.P > 0:
        d2, dco, drgb = C.render_backward(case.means2D, case.conic_opacity, case.rgb, case.compute_locally, case.bg,
                                          case.W, case.H, pl, rg, fT, nc, case.dL_dpixels)
    else:
        d2, dco, drgb = torch.zeros(0, 2), torch.zeros(0, 4), torch.zeros(0, 3)
    out.update(d_means2D=d2, d_conic=dco[:, :3].contiguous(), d_opacity=dco[:, 3:].contiguous(), d_rgb=drgb)
    return out


def boundaries_walked(case):
    """per local tile: the 256-entry boundaries K8's walk crosses, from the float64 decisions (the walk ends behind the
    chunk in which the last pixel stops, or at the end of the list)"""
    out = {}
    for d in decisions(case):
        stop = d["stop_idx"]
        walk = d["L"] if bool((stop >= d["L"]).any()) else int(stop.max()) + 1
        out[d["tile"]] = (walk - 1) // SEG_LEN
    return out


# ------------------------------------------------------------------------------------------------ K10's formulation
LOG2E = 1.4426950408889634


def _fma(a, b, c):
    """fmaf on float32 tensors: the product and the sum in float64 (the product is exact there), rounded once more"""
    return (a.double() * b.double() + c.double()).float()


def _ulps(x, n):
    """x moved by n float32 ulps (n = 0: x itself)"""
    return x if n == 0 else (x.contiguous().view(torch.int32) + n * torch.sign(x).to(torch.int32)).view(torch.float32)


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def k10_emulation(case, rcp_ulps=0, log_ulps=0, exp_ulps=0):
    """A CPU float32 emulation of the ORDER OF OPERATIONS of composite_backward_kernel, for judging whether a figure is a
    property of the formulation (it is never a reference): per pixel the walk back to front from the float32 final_T,
    alpha = exp2(a2 dx^2 + b2 dx dy + c2 dy^2 + log2 o), T divided by (1 - alpha), the scalar recurrence rho, (q, w) per
    (pixel, entry); per quadrant the raw pixel moments about the TILE origin as two fmaf chains over the even / odd
    4-pixel steps; the four quadrants added pairwise; the five moments rebuilt by the binomial expansion; the per-tile
    values added in float64 and rounded once.  Library exp2 / log2 and a correctly rounded division stand in for the
    hardware's approximations, so what this shows is the formulation, not the instruction set; `rcp_ulps`, `log_ulps`
    and `exp_ulps` move the reciprocal, log2 o or exp2 by that many float32 ulps (the hardware functions are good to one),
    to show how far the formulation carries such an error.  -> the gradient groups"""
    f32 = torch.float32
    r64, r32 = references(case)
    acc = torch.zeros(case.P, 9, dtype=torch.float64)
    le = _f(LOG2E)
    for t in range(case.tiles):
        ids = case.lists[t]
        if not bool(case.compute_locally[t]) or ids.numel() == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        yl, xl = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
        inside = ((xl + x0) < case.W) & ((yl + y0) < case.H)
        py, px = (yl + y0).clamp(max=case.H - 1), (xl + x0).clamp(max=case.W - 1)
        g = torch.where(inside[None], case.dL_dpixels[:, py, px], torch.zeros(()))          # [3,16,16]
        T_final = torch.where(inside, r32["final_T"].reshape(case.H, case.W)[py, px].to(f32), torch.zeros(()))
        last = torch.where(inside, r64["n_contrib"][py, px].to(torch.int64), torch.zeros((), dtype=torch.int64))
        pxf, pyf = (xl + x0).to(f32), (yl + y0).to(f32)
        bg = case.bg
        tb = T_final * (bg[0] * g[0] + bg[1] * g[1] + bg[2] * g[2])
        T, rho = T_final.clone(), torch.zeros(16, 16)
        n = int(last.max())
        Q, Wt = torch.zeros(n, 16, 16), torch.zeros(n, 16, 16)
        for k in range(n - 1, -1, -1):
            i = int(ids[k])
            x, y = case.means2D[i]
            A, B, Cc, o = case.conic_opacity[i]
            if not float(o) >= ALPHA_MIN:
                continue
            a2, b2, c2, lo = _f(-0.5) * le * A, -le * B, _f(-0.5) * le * Cc, _ulps(torch.log2(o), log_ulps)
            dx, dy = x - pxf, y - pyf
            pe = _fma(_fma(a2, dx, b2 * dy), dx, _fma(c2 * dy, dy, lo))
            aar = _ulps(torch.exp2(pe), exp_ulps)
            aal = torch.clamp(aar, max=0.99)
            take = (k + 1 <= last) & (pe <= lo) & (aal >= _f(ALPHA_MIN))
            if not bool(take.any()):
                continue
            qx, qy = torch.where(take, aar, torch.zeros(())), torch.where(take, aal, torch.zeros(()))
            inv = _ulps(1.0 / (1.0 - qy), rcp_ulps)
            tbi = inv * tb
            r, gg, b = case.rgb[i]
            cg = _fma(b, g[2], _fma(gg, g[1], r * g[0]))
            Tn = T * inv
            dot = cg - rho
            da = _fma(dot, Tn, -tbi)
            Q[k], Wt[k] = qx * da, qy * Tn
            rho = _fma(qy, dot, rho)
            T = Tn
        # raw moments per quadrant: B operand columns 1, x, y, x^2, x y, y^2 about the tile origin, then dL/dcolour
        xf, yf = xl.to(f32), yl.to(f32)
        cols = [torch.ones(16, 16), xf, yf, xf * xf, xf * yf, yf * yf, g[0], g[1], g[2]]
        quad = []
        for wv in range(4):
            qx0, qy0 = (wv & 1) * 8, (wv >> 1) * 8
            ch = [torch.zeros(n, 9), torch.zeros(n, 9)]
            for tt in range(16):
                for kq in range(4):
                    yy, xx = qy0 + (tt >> 1), qx0 + kq + 4 * (tt & 1)
                    a = torch.cat([Q[:, yy, xx, None].expand(n, 6), Wt[:, yy, xx, None].expand(n, 3)], dim=1)
                    bcol = torch.stack([c[yy, xx] for c in cols])
                    ch[tt & 1] = _fma(a, bcol[None, :].expand(n, 9), ch[tt & 1])
            quad.append(ch[0] + ch[1])
        Sv = (quad[0] + quad[1]) + (quad[2] + quad[3])
        # the flush: moments -> gradients
        idk = ids[:n]
        x, y = case.means2D[idk, 0], case.means2D[idk, 1]
        co = case.conic_opacity[idk]
        a2, b2, c2 = _f(-0.5) * le * co[:, 0], -le * co[:, 1], _f(-0.5) * le * co[:, 2]
        cA, cB, cC = a2 * _f(-2.0 / LOG2E), b2 * _f(-1.0 / LOG2E), c2 * _f(-2.0 / LOG2E)
        ex, ey = x - float(x0), y - float(y0)
        A0, Ax, Ay = Sv[:, 0], Sv[:, 1], Sv[:, 2]
        Mx, My = _fma(ex, A0, -Ax), _fma(ey, A0, -Ay)
        o = torch.zeros(n, 9)
        o[:, 0] = -(cA * Mx + cB * My) * _f(0.5 * case.W)
        o[:, 1] = -(cB * Mx + cC * My) * _f(0.5 * case.H)
        o[:, 2:5] = Sv[:, 6:9]
        o[:, 5] = _f(-0.5) * _fma(_fma(ex, A0, _f(-2.0) * Ax), ex, Sv[:, 3])
        o[:, 6] = -(_fma(ex, My, -ey * Ax) + Sv[:, 4])
        o[:, 7] = _f(-0.5) * _fma(_fma(ey, A0, _f(-2.0) * Ay), ey, Sv[:, 5])
        o[:, 8] = torch.where(A0 == 0, torch.zeros(()), A0 / co[:, 3].clamp(min=1e-30))
        acc.index_add_(0, idk, o.double())
    return split_record(acc.float())


# ------------------------------------------------------------------------------------------------ families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _u(gen, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64)


def _soft(gen, n, lo, hi, sig, op):
    """n splats with means in [lo, hi]^2, standard deviations in `sig`, opacities in `op`"""
    means = torch.stack([_u(gen, n, lo[0], hi[0]), _u(gen, n, lo[1], hi[1])], dim=1)
    con = conics(_u(gen, n, *sig), _u(gen, n, *sig), _u(gen, n, 0.0, math.pi))
    return means, con, _u(gen, n, *op), torch.rand(n, 3, generator=gen, dtype=torch.float64)


def _cat(parts):
    return [torch.cat([p[i] for p in parts]) for i in range(4)]


def _falling_colours(gen, rgb, order):
    """colours that fall from the front of the list to the back, per channel.  With them (c - R) . g, R the colour behind
    an entry, keeps one sign over the pixels (dL/dpixels is positive, the background not brighter than the last entry),
    so the sum over the pixels behind dL/dopacity does not cancel and the row is as well conditioned as the blend allows:
    a relative error eps of alpha then moves the row by about eps, not by eps times a large cancellation factor."""
    n = order.numel()
    vals = torch.sort(0.15 + 0.85 * torch.rand(n, 3, generator=gen, dtype=torch.float64), dim=0, descending=True).values
    rgb[order] = vals
    return rgb


LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129]
# Seeds are chosen on the CPU so that the C restatement (plain fp32, oracle/gsraster_ref.c) stays within K / 2 of the
# float64 reference on every tensor (tests/test_composite_refs_cpu.py): that leaves a kernel a factor of two over an
# independent fp32 implementation.  Where the default seed of a case did not give that with room to spare (the unit is
# another machine's float32 too), the best of about ten seeds tried is here.
LENGTH_SEEDS = {}
DEEP_SEEDS = {255: 404, 256: 404, 257: 402, 512: 400, 513: 400, 600: 402}


def _outside(gen, m):
    """offsets in m -> means that far OUTSIDE the 16 x 16 tile, on either side in x and in y: dx and dy keep their sign over
    the tile, so the first moments behind dL/dmean do not cancel (a broad splat centred in the tile is the opposite: its
    dL/dmean is the small difference of ex M0 and Ax, and carries every error of q many times over; EXPERIMENTS.md)"""
    side = torch.rand(m.shape[0], 2, generator=gen, dtype=torch.float64) < 0.5
    return torch.where(side, -m, 16.0 + m)


def lengths_case(L, seed=None):
    """one 16 x 16 tile, broad soft splats, nobody saturates: every residue of K8's 4-slot groups, K10's pairs and 8-entry
    batches, the 64-entry chunk edges.  Three rows more than the list holds stay out of it."""
    seed = LENGTH_SEEDS.get(L, 100 + L) if seed is None else seed
    gen = _gen(seed)
    P = L + 3
    amax = min(0.3, 4.0 / max(L, 1))  # sum of alpha <= 4: T stays above e^-4
    m, c, o, rgb = _soft(gen, P, (2.0, 2.0), (8.0, 8.0), (8.0, 16.0), (0.25 * amax, amax))
    m = _outside(gen, m)
    ids = torch.randperm(P, generator=gen)[:L]
    rgb = _falling_colours(gen, rgb, ids)
    return Case("lengths", str(L), 16, 16, m, c, o, rgb, [0.0, 0.0, 0.0], [True], [ids], seed)


DEEP = [255, 256, 257, 512, 513, 600]
DEEP_LONG = 16 * SEG_LEN + 304  # 4400 entries: 17 boundaries walked, the last one past the 16 that may carry a checkpoint


def deep_case(L, seed=None):
    """one tile, alpha in about [0.006, 0.02] on every pixel (very broad splats), nobody stops"""
    seed = DEEP_SEEDS.get(L, 200 + L) if seed is None else seed
    gen = _gen(seed)
    hi = min(0.02, 7.0 / L + 0.004)
    m, c, o, rgb = _soft(gen, L, (2.0, 2.0), (10.0, 10.0), (40.0, 90.0), (0.0075, hi))
    m = _outside(gen, m)
    lst = torch.randperm(L, generator=gen)
    return Case("deep", str(L), 16, 16, m, c, o, _falling_colours(gen, rgb, lst), [0.1, 0.15, 0.05], [True], [lst], seed)


def deep_long_case(seed=71):
    """DEEP_LONG entries, about 300 of which blend; the others are fillers whose alpha is below 1/255 on every pixel
    (opacity below 1/255, or a small splat far from the tile).  20 of the blending entries lie behind entry 4096."""
    gen = _gen(seed)
    L, nb = DEEP_LONG, 300
    m, c, o, rgb = _soft(gen, nb, (2.0, 2.0), (10.0, 10.0), (40.0, 90.0), (0.0075, 0.02))
    m = _outside(gen, m)
    nf = L - nb
    fm, fc, fo, frgb = _soft(gen, nf, (-4.0, -4.0), (20.0, 20.0), (3.0, 10.0), (0.0008, 0.0035))
    far = torch.arange(nf) % 3 == 0  # a third of the fillers: a real opacity, but 150 px and more from the tile
    fm[far] = fm[far] + 150.0 + _u(gen, int(far.sum()), 0.0, 50.0)[:, None]
    fo[far] = _u(gen, int(far.sum()), 0.3, 0.9)
    fc[far] = conics(_u(gen, int(far.sum()), 2.0, 4.0), _u(gen, int(far.sum()), 2.0, 4.0), _u(gen, int(far.sum()), 0.0, math.pi))
    means, con, op, col = _cat([(m, c, o, rgb), (fm, fc, fo, frgb)])
    # list positions of the blending entries: 280 in front of entry 4096, 20 behind it, the last entry among them
    front = torch.randperm(16 * SEG_LEN, generator=gen)[:nb - 20]
    back = 16 * SEG_LEN + torch.randperm(L - 16 * SEG_LEN - 2, generator=gen)[:18] + 1
    pos = torch.cat([front, back, torch.tensor([16 * SEG_LEN, L - 1])])
    lst = torch.empty(L, dtype=torch.int64)
    is_b = torch.zeros(L, dtype=torch.bool)
    is_b[pos] = True
    lst[is_b] = torch.randperm(nb, generator=gen)
    lst[~is_b] = nb + torch.randperm(nf, generator=gen)
    col = _falling_colours(gen, col, lst[is_b])
    return Case("deep", "long", 16, 16, means, con, op, col, [0.1, 0.15, 0.05], [True], [lst], seed)


def saturating_case(name, seed):
    """one tile; twelve nearly opaque blobs inside quadrant 0 come first, then broad splats of medium opacity over the whole
    tile: quadrant 0 stops within a few entries, the others much later and at different positions, and the tail of the
    list lies behind every pixel's stop"""
    gen = _gen(seed)
    a = _soft(gen, 12, (0.5, 0.5), (6.5, 6.5), (4.0, 6.0), (0.9, 0.97))
    b = _soft(gen, 56, (-2.0, -2.0), (18.0, 18.0), (6.0, 12.0), (0.3, 0.7))
    m, c, o, rgb = _cat([a, b])
    lst = torch.cat([torch.randperm(12, generator=gen), 12 + torch.randperm(56, generator=gen)])
    return Case("saturating", name, 16, 16, m, c, o, rgb, [0.1, 0.4, 0.9], [True], [lst], seed)


def clamp_case(name, seed):
    """opacities in (0.99, 1] (one exactly 1) with means on or near distinct pixel centres, narrow enough that a pixel is
    clamped by one entry only; Gaussian 0 lies exactly on the centre of pixel (5, 9): power == 0.  Soft splats around"""
    gen = _gen(seed)
    n = 10
    cells = torch.randperm(25, generator=gen)[:n]  # distinct pixels on a 5 x 5 grid of stride 2, from (1, 1)
    centres = torch.stack([1.0 + 2.0 * (cells % 5), 1.0 + 2.0 * (cells // 5)], dim=1).double()
    centres[0] = torch.tensor([5.0, 9.0])
    off = (torch.rand(n, 2, generator=gen, dtype=torch.float64) - 0.5) * 0.1
    off[:3] = 0.0  # three means exactly on a pixel centre
    sx, sy = _u(gen, n, 4.0, 7.0), _u(gen, n, 4.0, 7.0)
    op = _u(gen, n, 0.992, 1.0)
    op[0], op[1] = 1.0, 0.9999
    hard = (centres + off, conics(sx, sy, _u(gen, n, 0.0, math.pi)), op, torch.rand(n, 3, generator=gen, dtype=torch.float64))
    soft = _soft(gen, 6, (-2.0, -2.0), (18.0, 18.0), (7.0, 12.0), (0.05, 0.3))
    m, c, o, rgb = _cat([hard, soft])
    lst = torch.randperm(n + 6, generator=gen)
    lst = torch.cat([torch.tensor([0]), lst[lst != 0]])  # Gaussian 0 in front: the pixel under it blends it with T = 1
    return Case("clamp", name, 16, 16, m, c, o, rgb, [0.3, 0.3, 0.3], [True], [lst], seed)


def offtile_case(name, seed, dmax=2000.0):
    """large anisotropic splats whose means lie 100 .. dmax px outside a 16 x 16 frame, long axis towards the frame: the
    moment expansion about the tile origin with large ex, ey.  The short axis is at least d / 25, which bounds the
    cancellation inside `power` (terms of about (d / sigma_s)^2 / 4 that cancel to order 1) to what float32 resolves."""
    gen = _gen(seed)
    n = 12
    d = torch.cat([_u(gen, n - 2, 100.0, dmax), torch.tensor([dmax, 0.75 * dmax], dtype=torch.float64)])
    phi = _u(gen, n, 0.0, 2.0 * math.pi)
    phi[-2] = 0.25 * math.pi
    means = 8.0 + d[:, None] * torch.stack([torch.cos(phi), torch.sin(phi)], dim=1)
    ss = torch.maximum(_u(gen, n, 8.0, 30.0), d / 25.0)
    sl = d / _u(gen, n, 1.2, 2.0)
    theta = phi + _u(gen, n, -0.2, 0.2) * ss / d
    m, c, o, rgb = means, conics(sl, ss, theta), _u(gen, n, 0.3, 0.9), torch.rand(n, 3, generator=gen, dtype=torch.float64)
    return Case("offtile", name, 16, 16, m, c, o, rgb, [0.0, 0.1, 0.2], [True], [torch.randperm(n, generator=gen)], seed)


def edges_case(name, W, H, mask, seed, P=40, band=None):
    """lists that differ per tile (the Gaussians within 3 sigma of the tile, shuffled, plus the broad ones every tile
    shares), non-zero background, tiles that are not ours -- whose lists are full all the same"""
    gen = _gen(seed)
    nb = 6
    a = _soft(gen, P - nb, (-4.0, -4.0), (W + 4.0, H + 4.0), (4.0, 8.0), (0.1, 0.8))
    b = _soft(gen, nb, (0.0, 0.0), (float(W), float(H)), (14.0, 25.0), (0.1, 0.3))  # in every tile's list
    m, c, o, rgb = _cat([a, b])
    gx, gy = (W + 15) // 16, (H + 15) // 16
    reach = 3.0 * 8.0
    lists = []
    for t in range(gx * gy):
        ty, tx = divmod(t, gx)
        x0, y0, x1, y1 = tx * 16, ty * 16, min(tx * 16 + 16, W), min(ty * 16 + 16, H)
        near = ((m[:, 0] > x0 - reach) & (m[:, 0] < x1 + reach) & (m[:, 1] > y0 - reach) & (m[:, 1] < y1 + reach))
        near[P - nb:] = True
        ids = near.nonzero().reshape(-1)
        lists.append(ids[torch.randperm(ids.numel(), generator=gen)])
    return Case("edges", name, W, H, m, c, o, rgb, [0.1, 0.4, 0.9], mask, lists, seed, band=band)


def inert_case(seed=5):
    """32 x 16: tile 0 is ours, tile 1 is not.  Rows 0-3 blend in tile 0.  Row 4 is in no list, row 5 only in the list of
    tile 1, row 6 has opacity exactly 0, row 7 an opacity below 1/255, row 8 a real opacity but lies 120 px away (alpha
    below 1/255 on every pixel), row 9 blends in tile 0 and is ALSO in tile 1's list"""
    gen = _gen(seed)
    m, c, o, rgb = _soft(gen, 10, (2.0, 2.0), (14.0, 14.0), (3.0, 8.0), (0.2, 0.7))
    m[5] = torch.tensor([24.0, 8.0], dtype=torch.float64)
    o[6] = 0.0
    o[7] = 0.003
    m[8] = torch.tensor([-120.0, 8.0], dtype=torch.float64)
    lists = [torch.tensor([3, 7, 0, 6, 9, 8, 2, 1]), torch.tensor([9, 5])]
    return Case("inert", "rows", 32, 16, m, c, o, rgb, [0.5, 0.2, 0.1], [True, False], lists, seed)


def inert_p1_case():
    """P = 1: one row with a real opacity 120 px from the tile, in the list"""
    m = torch.tensor([[-120.0, 8.0]], dtype=torch.float64)
    c = conics(torch.tensor([3.0], dtype=torch.float64), torch.tensor([4.0], dtype=torch.float64),
               torch.tensor([0.3], dtype=torch.float64))
    return Case("inert", "P1", 16, 16, m, c, torch.tensor([0.6]), torch.tensor([[0.2, 0.7, 0.4]]), [0.5, 0.2, 0.1], [True],
                [torch.tensor([0])], 6)


def inert_p0_case():
    z = torch.zeros(0, dtype=torch.float64)
    return Case("inert", "P0", 16, 16, z.reshape(0, 2), z.reshape(0, 3), z, z.reshape(0, 3), [0.5, 0.2, 0.1], [True],
                [torch.zeros(0, dtype=torch.int64)], 7)


@functools.lru_cache(maxsize=None)
def cases():
    """every case, in a fixed order (built once: the generators are deterministic)"""
    out = [lengths_case(L) for L in LENGTHS]
    out += [deep_case(L) for L in DEEP] + [deep_long_case()]
    out += [saturating_case("a", 30), saturating_case("b", 33)]
    out += [clamp_case("a", 41), clamp_case("b", 42)]
    out += [offtile_case("far", 51), offtile_case("mid", 52, dmax=750.0)]
    out += [edges_case("16x16", 16, 16, [True], 61),
            edges_case("17x17", 17, 17, [False, False, True, True], 62, band=(1, 2)),
            edges_case("37x21", 37, 21, [True] * 6, 63),
            edges_case("37x21-holes", 37, 21, [True, False, True, False, True, True], 64),
            edges_case("40x24", 40, 24, [True, True, True, False, False, False], 65, band=(0, 1)),
            edges_case("8x8", 8, 8, [True], 66, P=16)]
    out += [inert_case(), inert_p1_case(), inert_p0_case()]
    return tuple(out)


def family(name):
    return [c for c in cases() if c.family == name]


FAMILIES = ["lengths", "deep", "saturating", "clamp", "offtile", "edges", "inert"]
VARIANT_FAMILIES = ["deep", "edges", "inert"]
