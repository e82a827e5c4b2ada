"""References for the absolute screen-space gradient (grendel-gs_amd/csrc/absgrad.hip) on the cases of
tests/composite_refs.py, which are imported and never modified: the frame, rows, lists, background and dL/dpixels are the
composite pair's own.

`closed_form(case, dtype)` writes the Definition of include/gsraster.h (gsr_render_absgrad) out without autograd, with
n_contrib from composite_refs.references: per (pixel, entry) dL/dalpha, q = o G dL/dalpha and the two terms
q (A dx + B dy) (W/2), q (B dx + C dy) (H/2), summed over the pixels once with their signs (`signed`: up to the sign
columns 0:2 of K10's record, which pins the per-pixel term against autograd) and once as magnitudes (`absgrad`).  The
float64 run is the arbiter; the float32 run is the unit of helpers.assert_rows_close (the reference's own fp32 error,
never a kernel's).  `kernel_emulation(case)` runs the ORDER OF OPERATIONS of composite_absgrad_kernel in float32 on the
CPU (never a reference: it shows what the formulation costs, with library exp2 / log2 and a correctly rounded division
standing in for the hardware's).

K of helpers.assert_rows_close is that of d_means2D (composite_refs.K_GROUP): the same chain from dL/dalpha on.
tests/test_absgrad_refs_cpu.py asserts that the emulation stays within HALF of K on every case."""
import functools

import torch

import composite_refs as R

K = R.K_GROUP["d_means2D"]
_fma, _f = R._fma, R._f


@functools.lru_cache(maxsize=None)
def closed_form(case, dtype=torch.float64):
    """-> dict(absgrad [P,2], signed [P,2], hits [P] the number of pixels that blend the row) in `dtype`"""
    dt = dtype
    m2, co, rgb, bg = case.means2D.to(dt), case.conic_opacity.to(dt), case.rgb.to(dt), case.bg.to(dt)
    nc = R.references(case)[0]["n_contrib"]
    g_all = case.dL_dpixels.to(dt)
    ab, sg = torch.zeros(case.P, 2, dtype=dt), torch.zeros(case.P, 2, dtype=dt)
    hits = torch.zeros(case.P, dtype=torch.int64)
    for t in range(case.tiles):
        ids = case.lists[t]
        L = ids.numel()
        if not bool(case.compute_locally[t]) or L == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        pxf, pyf = px.reshape(-1).to(dt), py.reshape(-1).to(dt)
        last = nc[y0:y1, x0:x1].reshape(-1).to(torch.int64)
        g = g_all[:, y0:y1, x0:x1].reshape(3, -1)                                   # [3, npx]
        xy, con, col = m2[ids], co[ids], rgb[ids]
        dx, dy = xy[:, 0:1] - pxf[None, :], xy[:, 1:2] - pyf[None, :]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        G = torch.exp(torch.clamp(power, max=0.0))
        araw = con[:, 3:4] * G
        alpha = torch.clamp(araw, max=0.99)
        pos1 = torch.arange(1, L + 1)[:, None]
        take = (pos1 <= last[None, :]) & (power <= 0) & (alpha >= R.ALPHA_MIN)
        a = torch.where(take, alpha, torch.zeros_like(alpha))
        T_behind = torch.cumprod(1.0 - a, dim=0)
        T = torch.cat([torch.ones_like(T_behind[:1]), T_behind[:-1]], dim=0)       # in front of the entry
        T_final = T_behind[-1]
        w = a * T
        dLda = -(T_final * (bg[:, None] * g).sum(dim=0))[None, :] / (1.0 - a)
        for c in range(3):
            wc = w * col[:, c:c + 1]
            S = torch.flip(torch.cumsum(torch.flip(wc, [0]), dim=0), [0]) - wc      # behind the entry
            dLda = dLda + g[c][None, :] * (T * col[:, c:c + 1] - S / (1.0 - a))
        q = torch.where(take, dLda * araw, torch.zeros_like(a))                     # (the clamp is the identity)
        A, B, C = con[:, 0:1], con[:, 1:2], con[:, 2:3]
        tx, ty = q * (A * dx + B * dy) * (0.5 * case.W), q * (B * dx + C * dy) * (0.5 * case.H)
        sg.index_add_(0, ids, torch.stack([tx.sum(dim=1), ty.sum(dim=1)], dim=1))
        ab.index_add_(0, ids, torch.stack([tx.abs().sum(dim=1), ty.abs().sum(dim=1)], dim=1))
        hits.index_add_(0, ids, take.sum(dim=1))
    return dict(absgrad=ab, signed=sg, hits=hits)


@functools.lru_cache(maxsize=None)
def kernel_emulation(case):
    """A CPU float32 emulation of the ORDER OF OPERATIONS of composite_absgrad_kernel (see the module docstring): per
    pixel the walk back to front from the float32 final_T, inv = 1 / (1 - alpha), Tn = T inv, the scalar recurrence rho
    on c . g, dL/dalpha = (c . g - rho) Tn - inv T_final (bg . g), q = o G dL/dalpha and the two magnitudes
    |q (2 a2 dx + b2 dy)|, |q (b2 dx + 2 c2 dy)| on the pre-scaled conic; per quadrant row the sum over its eight pixels in
    order, the eight rows combined as a balanced tree, the factor ln 2 (W/2, H/2) once per (quadrant, entry); the values
    added in float64 and rounded once.  -> absgrad float32 [P,2]"""
    f32 = torch.float32
    r64, r32 = R.references(case)
    acc = torch.zeros(case.P, 2, dtype=torch.float64)
    le = _f(R.LOG2E)
    ln2 = _f(0.6931471805599453)
    sx, sy = ln2 * _f(0.5 * case.W), ln2 * _f(0.5 * case.H)
    bg = case.bg
    for t in range(case.tiles):
        ids = case.lists[t]
        if not bool(case.compute_locally[t]) or ids.numel() == 0:
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        yl, xl = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
        inside = ((xl + x0) < case.W) & ((yl + y0) < case.H)
        py, px = (yl + y0).clamp(max=case.H - 1), (xl + x0).clamp(max=case.W - 1)
        g = torch.where(inside[None], case.dL_dpixels[:, py, px], torch.zeros(()))          # [3,16,16]
        T = torch.where(inside, r32["final_T"].reshape(case.H, case.W)[py, px].to(f32), torch.ones(()))
        last = torch.where(inside, r64["n_contrib"][py, px].to(torch.int64), torch.zeros((), dtype=torch.int64))
        tb = torch.where(inside, T * (bg[0] * g[0] + bg[1] * g[1] + bg[2] * g[2]), torch.zeros(()))
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
            inv = _f(1.0) / (1.0 - al)
            r, gg, b = case.rgb[i]
            cg = _fma(b, g[2], _fma(gg, g[1], r * g[0]))
            Tn = T * inv
            dot = cg - rho
            da = _fma(dot, Tn, -(inv * tb))
            q = ar * da
            ux = _fma((a2 + a2).expand(16, 16), dx, b2 * dy)
            uy = _fma(b2.expand(16, 16), dx, (c2 + c2) * dy)
            M0, M1 = (q * ux).abs(), (q * uy).abs()
            rho = _fma(al, dot, rho)
            T = Tn
            for wv in range(4):
                qx0, qy0 = (wv & 1) * 8, (wv >> 1) * 8
                if not bool(take[qy0:qy0 + 8, qx0:qx0 + 8].any()):
                    continue
                s0, s1 = torch.zeros(8), torch.zeros(8)
                for kk in range(8):
                    s0 = s0 + M0[qy0:qy0 + 8, qx0 + kk]
                    s1 = s1 + M1[qy0:qy0 + 8, qx0 + kk]

                def tree(r):
                    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))

                acc[i] += torch.stack([(tree(s0) * sx).to(torch.float64), (tree(s1) * sy).to(torch.float64)])
    return acc.float()
