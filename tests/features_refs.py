"""References for the N-channel feature map and its backward (grendel-gs_amd/csrc/features.hip) on the cases of
tests/composite_refs.py, each extended with seeded float32 `features` [P, C] in [0, 1] and g = dL/dout [C, H, W]:
channel c of g is case.dL_dpixels[c % 3] times a seeded per-channel factor in [0.5, 1.5].

`references(case, C)` -> (float64 results, float32 results): oracle.torch_oracle.render on the case's lists with bg = 0,
three channels at a time (the last group zero-padded), the groups' losses summed before ONE autograd.grad -- the arbiter,
and the unit of helpers.assert_rows_close (the reference's own fp32 error, never a kernel's).
`closed_form(case, C)` writes the Definition of include/gsraster.h out in float64 without autograd;
`kernel_emulation(case, C)` runs the ORDER OF OPERATIONS of composite_features_backward_kernel in float32 on the CPU
(never a reference: it shows what the formulation costs, with library exp2 / log2 and correctly rounded divisions
standing in for the hardware's, and an fmaf chain standing in for the matrix pipe).

K of helpers.assert_rows_close: 8 for the map and for d_features (the project's value for linear accumulations);
d_means2D, d_conic and d_opacity start from composite_refs.K_GROUP (14, 12, 9.5), and a K is raised to min(16, 2 x the
emulation's worst ratio) only where that ratio exceeds half of it.  The emulation's worst ratios against the float64
reference over every (case, C) of EMULATED (tests/test_features_refs_cpu.py recomputes and asserts them):
    d_means2D 3.91 (inert-rows, C = 4; K 14), d_conic 3.33 (lengths-129, C = 4; K 12),
    d_opacity 3.81 (edges-17x17, C = 17; K 9.5), d_features 3.26 (lengths-129, C = 4; K 8)
-- none exceeds half of its K, so the three stay at composite_refs.K_GROUP.  The figures are in EXPERIMENTS.md."""
import functools
import os
import re

import torch

import composite_refs as R
from oracle import torch_oracle as O

GROUPS = ["d_means2D", "d_conic", "d_opacity", "d_features"]
K_MAP = R.K_FORWARD
K_GROUP = {"d_means2D": R.K_GROUP["d_means2D"], "d_conic": R.K_GROUP["d_conic"], "d_opacity": R.K_GROUP["d_opacity"],
           "d_features": 8}

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    src = open(os.path.join(_ROOT, "include", "gsraster.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))


CH = _header_constant("GSR_FEATURES_CHUNK")   # channels per chunk of the kernels
CAP = _header_constant("GSR_FEATURES_MAX")
SWEEP = [1, 2, CH - 1, CH, CH + 1, 2 * CH + 3]


def chunk_width(C):
    """channels per walk of the kernels: the narrow instantiation serves C <= 4"""
    return 4 if C <= 4 else CH


@functools.lru_cache(maxsize=None)
def features_of(case, C):
    """float32 [P, C] in [0, 1], seeded per (case, C); never modified.  A case with ONE list gets every channel falling
    along the list (composite_refs._falling_colours, invdepth_refs.depths_of): f - (what lies behind, normalised) then
    keeps one sign over the pixels and the sums behind a row do not cancel.  The cases with several tiles shuffle their
    lists tile by tile and keep unordered features: the kernels assume no order."""
    gen = torch.Generator().manual_seed(9000 + 131 * case.seed + C)
    f = torch.rand(case.P, C, generator=gen, dtype=torch.float64)
    if len(case.lists) == 1 and case.lists[0].numel() > 1:
        ids = case.lists[0]
        f[ids] = torch.sort(0.15 + 0.85 * f[ids], dim=0, descending=True).values
    return f.to(torch.float32).clamp(0.0, 1.0).contiguous()


@functools.lru_cache(maxsize=None)
def g_of(case, C):
    """dL/dout [C,H,W] (float32): the case's dL_dpixels channels cycled, each with a seeded factor in [0.5, 1.5]"""
    fac = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(9500 + case.seed + 17 * C), dtype=torch.float64)
    return (case.dL_dpixels[torch.arange(C) % 3].double() * fac[:, None, None]).to(torch.float32).contiguous()


def _render(case, C, dtype):
    m2 = case.means2D.clone().to(dtype).requires_grad_(True)
    co = case.conic_opacity.clone().to(dtype).requires_grad_(True)
    f = features_of(case, C).clone().to(dtype).requires_grad_(True)
    g = g_of(case, C).to(dtype)
    maps, loss, fT, nc = [], 0.0, None, None
    for c0 in range(0, C, 3):
        n = min(3, C - c0)
        rgb = torch.cat([f[:, c0:c0 + n], torch.zeros(case.P, 3 - n, dtype=dtype)], dim=1)
        img, fT, nc = O.render(m2, co, rgb, None, None, case.compute_locally, bg=torch.zeros(3, dtype=dtype), W=case.W,
                               H=case.H, binning=(case.point_list, case.ranges[:case.tiles], None))
        maps.append(img[:n])
        loss = loss + (img[:n] * g[c0:c0 + n]).sum()
    out = torch.cat(maps, dim=0)
    if out.requires_grad and case.P > 0:
        gr = torch.autograd.grad(loss, [m2, co, f], allow_unused=True)
        gr = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(gr, (m2, co, f))]
    else:
        gr = [torch.zeros_like(m2), torch.zeros_like(co), torch.zeros_like(f)]
    HW = case.H * case.W
    return dict(map=out.detach().reshape(C, HW).t().contiguous(), n_contrib=nc, final_T=fT.reshape(HW, 1),
                d_means2D=gr[0], d_conic=gr[1][:, :3].contiguous(), d_opacity=gr[1][:, 3:].contiguous(), d_features=gr[2])


@functools.lru_cache(maxsize=None)
def references(case, C):
    """-> (float64 results, float32 results); `map` as rows [H*W, C]; computed once per (case, C) and never modified"""
    return _render(case, C, torch.float64), _render(case, C, torch.float32)


def split_records(rec, dfeat):
    """[P,6] record (columns: 0:2 means2D, 2:5 conic, 5 opacity) and [P,C] feature gradient -> the four groups"""
    return dict(d_means2D=rec[:, 0:2], d_conic=rec[:, 2:5], d_opacity=rec[:, 5:6], d_features=dfeat)


def map_rows(out):
    """[C,H,W] -> [H*W, C]"""
    return out.reshape(out.shape[0], -1).t().contiguous()


# ------------------------------------------------------------------------------------------------ closed forms
@functools.lru_cache(maxsize=None)
def closed_form(case, C):
    """the Definition of include/gsraster.h in float64, no autograd -> dict(map [HW,C], the four groups)"""
    dt = torch.float64
    m2, co, feat = case.means2D.to(dt), case.conic_opacity.to(dt), features_of(case, C).to(dt)
    nc = R.references(case)[0]["n_contrib"]
    g_all = g_of(case, C).to(dt)
    out = torch.zeros(C, case.H, case.W, dtype=dt)
    d2, dcon = torch.zeros(case.P, 2, dtype=dt), torch.zeros(case.P, 3, dtype=dt)
    dop, df = torch.zeros(case.P, 1, dtype=dt), torch.zeros(case.P, C, dtype=dt)
    for t in range(case.tiles):
        ids = case.lists[t]
        L = ids.numel()
        if not bool(case.compute_locally[t]) or L == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        pxf, pyf = px.reshape(-1).to(dt), py.reshape(-1).to(dt)
        last = nc[y0:y1, x0:x1].reshape(-1).to(torch.int64)
        g = g_all[:, y0:y1, x0:x1].reshape(C, -1)                                # [C, npx]
        xy, con, f = m2[ids], co[ids], feat[ids]                                 # f [L, C]
        dx, dy = xy[:, 0:1] - pxf[None, :], xy[:, 1:2] - pyf[None, :]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        G = torch.exp(torch.clamp(power, max=0.0))
        araw = con[:, 3:4] * G
        alpha = torch.clamp(araw, max=0.99)
        pos1 = torch.arange(1, L + 1)[:, None]
        take = (pos1 <= last[None, :]) & (power <= 0) & (alpha >= R.ALPHA_MIN)
        a = torch.where(take, alpha, torch.zeros_like(alpha))
        T_behind = torch.cumprod(1.0 - a, dim=0)
        T = torch.cat([torch.ones_like(T_behind[:1]), T_behind[:-1]], dim=0)   # in front of the entry
        w = a * T                                                                # [L, npx]
        out[:, y0:y1, x0:x1] = (f.t() @ w).view(C, y1 - y0, x1 - x0)
        fg = f @ g                                                               # sum_c g_c f_i[c]      [L, npx]
        wfg = w * fg
        Sg = torch.flip(torch.cumsum(torch.flip(wfg, [0]), dim=0), [0]) - wfg    # sum_c g_c S_i[c], behind the entry
        dLda = torch.where(take, T * fg - Sg / (1.0 - a), torch.zeros_like(a))
        q = dLda * araw                                                           # dL/dpower (the clamp is the identity)
        df.index_add_(0, ids, w @ g.t())
        dop.index_add_(0, ids, (dLda * G).sum(dim=1, keepdim=True))
        A, B, Cc = con[:, 0:1], con[:, 1:2], con[:, 2:3]
        d2.index_add_(0, ids, torch.stack([-(q * (A * dx + B * dy)).sum(dim=1) * (0.5 * case.W),
                                           -(q * (B * dx + Cc * dy)).sum(dim=1) * (0.5 * case.H)], dim=1))
        dcon.index_add_(0, ids, torch.stack([-0.5 * (q * dx * dx).sum(dim=1), -(q * dx * dy).sum(dim=1),
                                             -0.5 * (q * dy * dy).sum(dim=1)], dim=1))
    return dict(map=map_rows(out), d_means2D=d2, d_conic=dcon, d_opacity=dop, d_features=df)


# ------------------------------------------------------------------------------------------------ the kernel's order
_fma, _f = R._fma, R._f


@functools.lru_cache(maxsize=None)
def kernel_emulation(case, C):
    """A CPU float32 emulation of the ORDER OF OPERATIONS of composite_features_backward_kernel (see the module
    docstring): per channel chunk and pixel the walk back to front from the float32 final_T, Tn = T / (1 - alpha), cg =
    the fmaf chain of g_c f_c over the chunk's channels, the ONE scalar recurrence rho, (q, u) per (pixel, entry); per
    quadrant row the sums of q over its eight pixels in order about dx = (x - qx0) - k, the moments in dy as products, the
    eight rows combined as a balanced tree; the feature gradient as two fmaf chains over the K-steps of four pixels
    (even and odd steps), added; every value per (quadrant, entry, chunk) added in float64 and rounded once.
    -> the gradient groups"""
    f32 = torch.float32
    r64, r32 = R.references(case)
    feat, gmap = features_of(case, C), g_of(case, C)
    acc = torch.zeros(case.P, 6 + C, dtype=torch.float64)
    le = _f(R.LOG2E)
    cw = chunk_width(C)
    zero = torch.zeros(())
    for ch0 in range(0, C, cw):
        chans = list(range(ch0, min(ch0 + cw, C)))
        for t in range(case.tiles):
            ids = case.lists[t]
            if not bool(case.compute_locally[t]) or ids.numel() == 0:
                continue
            x0, y0, x1, y1 = case.tile_box(t)
            yl, xl = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
            inside = ((xl + x0) < case.W) & ((yl + y0) < case.H)
            py, px = (yl + y0).clamp(max=case.H - 1), (xl + x0).clamp(max=case.W - 1)
            g = [torch.where(inside, gmap[c][py, px], zero) for c in chans]
            T = torch.where(inside, r32["final_T"].reshape(case.H, case.W)[py, px].to(f32), torch.ones(()))
            last = torch.where(inside, r64["n_contrib"][py, px].to(torch.int64), torch.zeros((), dtype=torch.int64))
            pxf, pyf = (xl + x0).to(f32), (yl + y0).to(f32)
            rho = torch.zeros(16, 16)
            for k in range(int(last.max()) - 1, -1, -1):
                i = int(ids[k])
                x, y = case.means2D[i]
                A, B, Cc, o = case.conic_opacity[i]
                if not float(o) >= R.ALPHA_MIN:
                    continue
                a2, b2, c2, lo = _f(-0.5) * le * A, -le * B, _f(-0.5) * le * Cc, torch.log2(o)
                dx, dy = x - pxf, y - pyf
                pe = _fma(_fma(a2, dx, b2 * dy), dx, _fma(c2 * dy, dy, lo))
                aar = torch.exp2(pe)
                aal = torch.clamp(aar, max=0.99)
                take = (k + 1 <= last) & (pe <= lo) & (aal >= _f(R.ALPHA_MIN))
                if not bool(take.any()):
                    continue
                ar, al = torch.where(take, aar, zero), torch.where(take, aal, zero)
                cg = torch.zeros(16, 16)
                for j, c in enumerate(chans):
                    cg = _fma(g[j], feat[i, c].expand(16, 16), cg)
                Tn = T / (1.0 - al)
                dot = cg - rho
                Q, U = ar * (Tn * dot), al * Tn
                rho = _fma(al, dot, rho)
                T = Tn
                for wv in range(4):
                    qx0, qy0 = (wv & 1) * 8, (wv >> 1) * 8
                    if not bool(take[qy0:qy0 + 8, qx0:qx0 + 8].any()):
                        continue
                    ex = x - _f(float(x0 + qx0))
                    dyr = y - (torch.arange(8).to(f32) + float(y0 + qy0))           # per row of the quadrant
                    s0, s1, s2 = torch.zeros(8), torch.zeros(8), torch.zeros(8)
                    for kk in range(8):
                        qk = Q[qy0:qy0 + 8, qx0 + kk]
                        dxk = ex - _f(float(kk))
                        s0 = s0 + qk
                        s1 = _fma(qk, dxk.expand(8), s1)
                        s2 = _fma(qk * dxk, dxk.expand(8), s2)
                    rows = [s0, s1, dyr * s0, s2, dyr * s1, dyr * (dyr * s0)]

                    def tree(r):
                        return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))

                    M0, Mx, My, Mxx, Mxy, Myy = [tree(r) for r in rows]
                    vals = [-(A * Mx + B * My) * _f(0.5 * case.W), -(B * Mx + Cc * My) * _f(0.5 * case.H), _f(-0.5) * Mxx,
                            -Mxy, _f(-0.5) * Myy, M0 / o if float(M0) != 0.0 else _f(0.0)]
                    acc[i, :6] += torch.stack([val.to(torch.float64) for val in vals])
                    # the contraction on the matrix pipe: pixel p = 4 t + k of the quadrant, two chains (t even / odd)
                    uq = U[qy0:qy0 + 8, qx0:qx0 + 8].reshape(64)
                    gq = torch.stack([gj[qy0:qy0 + 8, qx0:qx0 + 8].reshape(64) for gj in g])   # [channels, 64]
                    ch = [torch.zeros(len(chans)), torch.zeros(len(chans))]
                    for p in range(64):
                        ch[(p >> 2) & 1] = _fma(uq[p].expand(len(chans)), gq[:, p], ch[(p >> 2) & 1])
                    acc[i, 6 + ch0:6 + ch0 + len(chans)] += (ch[0] + ch[1]).to(torch.float64)
    rec = acc.float()
    return split_records(rec[:, :6], rec[:, 6:])
