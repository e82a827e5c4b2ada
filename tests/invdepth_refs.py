"""References for the inverse-depth map and its backward (grendel-gs_amd/csrc/invdepth.hip) on the cases of
tests/composite_refs.py, each extended with seeded float32 `depths` in [0.25, 60] and dL/dinvdepth = dL_dpixels[0].

`references(case)` -> (float64 results, float32 results): oracle.torch_oracle.render on the case's lists with
rgb = (v, 0, 0), v = 1 / depth, and bg = 0 -- channel 0 of its image IS the map of include/gsraster.h -- differentiated by
autograd: the arbiter, and the unit of helpers.assert_rows_close (the reference's own fp32 error, never a kernel's).
`closed_form(case)` writes the header's formulas out in float64 without autograd; `kernel_emulation(case)` runs the
ORDER OF OPERATIONS of composite_invdepth_backward_kernel in float32 on the CPU (never a reference: it shows what the
formulation costs, with library exp2 / log2 and correctly rounded divisions standing in for the hardware's).

K of helpers.assert_rows_close: 8 for the map and for d_depth (a linear accumulation like d_rgb), composite_refs.K_GROUP
for d_means2D, d_conic and d_opacity (K10's chain from dL/dalpha on).  tests/test_invdepth_refs_cpu.py recomputes the
emulation and asserts that it stays within HALF of each K on every case, so the kernel keeps a factor of two over its
own formulation; the measured ratios are in EXPERIMENTS.md."""
import functools

import torch

import composite_refs as R
from oracle import torch_oracle as O

GROUPS = ["d_means2D", "d_conic", "d_opacity", "d_depth"]
K_MAP = R.K_FORWARD
K_GROUP = {"d_means2D": R.K_GROUP["d_means2D"], "d_conic": R.K_GROUP["d_conic"], "d_opacity": R.K_GROUP["d_opacity"],
           "d_depth": 8}
DEPTH_LO, DEPTH_HI = 0.25, 60.0


@functools.lru_cache(maxsize=None)
def depths_of(case):
    """float32 [P] in [0.25, 60], seeded per case; never modified.  The binning sorts every list by depth, so a case with
    ONE list gets its depths ascending along the list, as a real list has them: v then falls from the front to the back,
    v - (what lies behind, normalised) keeps one sign over the pixels, and the sums over the pixels behind a row do not
    cancel (composite_refs._falling_colours does the same for the colours).  The cases with several tiles shuffle their
    lists tile by tile, no order satisfies all of them, and they keep unordered depths: the kernels assume no order."""
    u = torch.rand(case.P, generator=torch.Generator().manual_seed(7000 + case.seed), dtype=torch.float64)
    d = (DEPTH_LO + (DEPTH_HI - DEPTH_LO) * u).to(torch.float32).clamp(DEPTH_LO, DEPTH_HI)
    if len(case.lists) == 1 and case.lists[0].numel() > 1:
        ids = case.lists[0]
        d[ids] = torch.sort(d[ids]).values
    return d


def g_of(case):
    """dL/dinvdepth [H,W] (float32)"""
    return case.dL_dpixels[0].contiguous()


def _render(case, dtype):
    m2 = case.means2D.clone().to(dtype).requires_grad_(True)
    co = case.conic_opacity.clone().to(dtype).requires_grad_(True)
    d = depths_of(case).clone().to(dtype).requires_grad_(True)
    v = 1.0 / d
    rgb = torch.stack([v, torch.zeros_like(v), torch.zeros_like(v)], dim=1)
    img, fT, nc = O.render(m2, co, rgb, None, None, case.compute_locally, bg=torch.zeros(3, dtype=dtype), W=case.W,
                           H=case.H, binning=(case.point_list, case.ranges[:case.tiles], None))
    inv = img[0]
    if inv.requires_grad and case.P > 0:
        g = torch.autograd.grad((inv * g_of(case).to(dtype)).sum(), [m2, co, d], allow_unused=True)
        g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (m2, co, d))]
    else:
        g = [torch.zeros_like(m2), torch.zeros_like(co), torch.zeros_like(d)]
    return dict(invdepth=inv.detach().reshape(-1, 1), n_contrib=nc, final_T=fT.reshape(-1, 1), d_means2D=g[0],
                d_conic=g[1][:, :3].contiguous(), d_opacity=g[1][:, 3:].contiguous(), d_depth=g[2].reshape(-1, 1))


@functools.lru_cache(maxsize=None)
def references(case):
    """-> (float64 results, float32 results); computed once per case and never modified"""
    return _render(case, torch.float64), _render(case, torch.float32)


def split_record(rec):
    """[P,7] record -> the four gradient groups (columns: 0:2 means2D, 2:5 conic, 5 opacity, 6 depth)"""
    return dict(d_means2D=rec[:, 0:2], d_conic=rec[:, 2:5], d_opacity=rec[:, 5:6], d_depth=rec[:, 6:7])


# ------------------------------------------------------------------------------------------------ closed forms
@functools.lru_cache(maxsize=None)
def closed_form(case):
    """the Definition of include/gsraster.h in float64, no autograd -> dict(invdepth [HW,1], the four groups)"""
    dt = torch.float64
    m2, co, dep = case.means2D.to(dt), case.conic_opacity.to(dt), depths_of(case).to(dt)
    nc = R.references(case)[0]["n_contrib"]
    g_all = g_of(case).to(dt)
    inv = torch.zeros(case.H, case.W, dtype=dt)
    d2, dcon = torch.zeros(case.P, 2, dtype=dt), torch.zeros(case.P, 3, dtype=dt)
    dop, dv = torch.zeros(case.P, 1, dtype=dt), torch.zeros(case.P, dtype=dt)
    for t in range(case.tiles):
        ids = case.lists[t]
        L = ids.numel()
        if not bool(case.compute_locally[t]) or L == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        pxf, pyf = px.reshape(-1).to(dt), py.reshape(-1).to(dt)
        last = nc[y0:y1, x0:x1].reshape(-1).to(torch.int64)
        g = g_all[y0:y1, x0:x1].reshape(-1)
        xy, con, v = m2[ids], co[ids], (1.0 / dep[ids])[:, None]
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
        w = a * T
        wv = w * v
        inv[y0:y1, x0:x1] = wv.sum(dim=0).view(y1 - y0, x1 - x0)
        S = torch.flip(torch.cumsum(torch.flip(wv, [0]), dim=0), [0]) - wv      # behind the entry
        dLda = torch.where(take, g[None, :] * (T * v - S / (1.0 - a)), torch.zeros_like(a))
        q = dLda * araw                                                           # dL/dpower (the clamp is the identity)
        dv.index_add_(0, ids, (g[None, :] * w).sum(dim=1))
        dop.index_add_(0, ids, (dLda * G).sum(dim=1, keepdim=True))
        A, B, C = con[:, 0:1], con[:, 1:2], con[:, 2:3]
        d2.index_add_(0, ids, torch.stack([-(q * (A * dx + B * dy)).sum(dim=1) * (0.5 * case.W),
                                           -(q * (B * dx + C * dy)).sum(dim=1) * (0.5 * case.H)], dim=1))
        dcon.index_add_(0, ids, torch.stack([-0.5 * (q * dx * dx).sum(dim=1), -(q * dx * dy).sum(dim=1),
                                             -0.5 * (q * dy * dy).sum(dim=1)], dim=1))
    safe = torch.where(dv != 0, dep, torch.ones_like(dep))
    return dict(invdepth=inv.reshape(-1, 1), d_means2D=d2, d_conic=dcon, d_opacity=dop,
                d_depth=(-dv / (safe * safe)).reshape(-1, 1))


def depth_to_means3D(d_depth, radii, viewmatrix):
    """the closed form of gsr_depth_backward_means3d in the dtype of its arguments: rows with radii <= 0 are zero"""
    col = torch.stack([viewmatrix[0, 2], viewmatrix[1, 2], viewmatrix[2, 2]])
    out = d_depth.reshape(-1, 1) * col[None, :]
    return torch.where((radii > 0)[:, None], out, torch.zeros_like(out))


# ------------------------------------------------------------------------------------------------ the kernel's order
_fma, _f = R._fma, R._f


@functools.lru_cache(maxsize=None)
def kernel_emulation(case):
    """A CPU float32 emulation of the ORDER OF OPERATIONS of composite_invdepth_backward_kernel (see the module
    docstring): per pixel the walk back to front from the float32 final_T, Tn = T / (1 - alpha), the scalar recurrence
    rho, (q, u) per (pixel, entry); per quadrant row the sums over its eight pixels in order about dx = (x - qx0) - k,
    the moments in dy as products, the eight rows combined as a balanced tree; the seven values per (quadrant, entry)
    added in float64 and rounded once, the depth column through -1 / depth^2 in float64.  -> the gradient groups"""
    f32 = torch.float32
    r64, r32 = R.references(case)
    dep = depths_of(case)
    acc = torch.zeros(case.P, 7, dtype=torch.float64)
    le = _f(R.LOG2E)
    gmap = g_of(case)
    for t in range(case.tiles):
        ids = case.lists[t]
        if not bool(case.compute_locally[t]) or ids.numel() == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        yl, xl = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
        inside = ((xl + x0) < case.W) & ((yl + y0) < case.H)
        py, px = (yl + y0).clamp(max=case.H - 1), (xl + x0).clamp(max=case.W - 1)
        g = torch.where(inside, gmap[py, px], torch.zeros(()))
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
            ar, al = torch.where(take, aar, torch.zeros(())), torch.where(take, aal, torch.zeros(()))
            v = _f(1.0) / dep[i]
            Tn = T / (1.0 - al)
            dot = v - rho
            gT = g * Tn
            Q, U = ar * (gT * dot), al * gT
            rho = _fma(al, dot, rho)
            T = Tn
            for wv in range(4):
                qx0, qy0 = (wv & 1) * 8, (wv >> 1) * 8
                if not bool(take[qy0:qy0 + 8, qx0:qx0 + 8].any()):
                    continue
                ex = x - _f(float(x0 + qx0))
                dyr = y - (torch.arange(8).to(f32) + float(y0 + qy0))           # per row of the quadrant
                s0, s1, s2, su = torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(8)
                for kk in range(8):
                    qk, uk = Q[qy0:qy0 + 8, qx0 + kk], U[qy0:qy0 + 8, qx0 + kk]
                    dxk = ex - _f(float(kk))
                    s0 = s0 + qk
                    s1 = _fma(qk, dxk.expand(8), s1)
                    s2 = _fma(qk * dxk, dxk.expand(8), s2)
                    su = su + uk
                rows = [s0, s1, dyr * s0, s2, dyr * s1, dyr * (dyr * s0), su]

                def tree(r):
                    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))

                M0, Mx, My, Mxx, Mxy, Myy, Su = [tree(r) for r in rows]
                vals = [-(A * Mx + B * My) * _f(0.5 * case.W), -(B * Mx + Cc * My) * _f(0.5 * case.H), _f(-0.5) * Mxx,
                        -Mxy, _f(-0.5) * Myy, M0 / o if float(M0) != 0.0 else _f(0.0), Su]
                acc[i] += torch.stack([val.to(torch.float64) for val in vals])
    d = dep.double()
    safe = torch.where(acc[:, 6] != 0, d, torch.ones_like(d))
    acc[:, 6] = -acc[:, 6] / (safe * safe)
    return split_record(acc.float())
