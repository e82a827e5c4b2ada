"""Masks, references and deliberately wrong references of the masked L1 + SSIM loss (include/gsraster.h, N1m): shared by
the CPU file that shows the tolerance separates right from wrong and by the GPU files that apply it to the HIP kernels.

Definition: m = byte / 255 per pixel, shared by the channels; inside the band x' = m x (with an exposure E = [A | b]:
x' = m (A x + b)) and y' = m gt / 255, outside the band both are 0; the loss is leaf_refs.loss_reference on (x', y');
dL/dx = m g' (with E: m A^T g'), dL/dA[c][k] = sum m g'[c] x[k], dL/db[c] = sum m g'[c], g' = dL/dx'."""
import torch

import leaf_refs as R

f32, f64, u8 = torch.float32, torch.float64, torch.uint8

MASK_FAMILIES = ["ones", "zeros", "edge", "toprows", "checker", "soft"]
# the image family (leaf_refs.loss_inputs) each mask family is laid over
IMAGE_OF = {"ones": "noise", "zeros": "noise", "edge": "smooth", "toprows": "noise", "checker": "range", "soft": "noise"}
WRONGS = ["x_only", "maps", "grad_no_m", "m256", "pad"]
EXPOSURES = {
    None: None,
    # (the two of tests/test_gpu_exposure_loss.py) well conditioned: identity plus off-diagonal entries <= 0.2, |b| <= 0.1
    "full": [[1.10, 0.15, -0.20, 0.05], [-0.10, 0.90, 0.20, -0.10], [0.20, -0.15, 1.05, 0.08]],
    # a large offset: padding or a masked pixel that leaks b (instead of 0) moves every window it touches
    "offset": [[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.125]],
}
EDGE_COLUMN = 17  # `edge`: zero left of this column -- off every 32-wide tile and every 4-wide vector boundary


def mask_weight_fp32(b):
    """the fp32 expression of the kernels: (float)byte * (1.0f / 255.0f), for a uint8 tensor"""
    return b.to(f32) * torch.tensor(1.0 / 255.0, dtype=f32)


def make_mask(family, H, W, y0, y1, seed=0):
    """-> uint8 [H, W] of one family.  The rows outside the band [y0, y1) hold bytes too (255 for the structured
    families, random ones for `soft`): a launch must never look at them."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * H + W + 3 * MASK_FAMILIES.index(family))
    m = torch.full((H, W), 255, dtype=u8)
    if family == "ones":
        pass
    elif family == "zeros":
        m[y0:y1] = 0
    elif family == "edge":
        m[:, :EDGE_COLUMN] = 0
    elif family == "toprows":
        m[y0:min(y0 + 3, y1)] = 0
    elif family == "checker":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        m[((yy // 3 + xx // 5) % 2) == 0] = 0
    elif family == "soft":
        m = torch.randint(0, 256, (H, W), generator=g, dtype=u8)
    else:
        raise ValueError(family)
    return m.contiguous()


def apply_exposure(x, E):
    """x' [3,R,W] = A x + b in x's dtype (E None: x)"""
    if E is None:
        return x
    E = E.to(x.dtype)
    return torch.stack([E[c, 0] * x[0] + E[c, 1] * x[1] + E[c, 2] * x[2] + E[c, 3] for c in range(3)])


def _maps_wrong(xe, y, m, dtype):
    """the mistake "mask applied to the L1 / SSIM maps": sums of m |x - y| and m ssim_map(x, y) on the unmasked inputs"""
    xe = xe.detach().clone().requires_grad_(True)
    w1 = R.window_1d().to(dtype)
    ssim, M1, M2, M3 = R._terms(xe, y, w1, 0.03 ** 2)
    l1, ss = (m * (xe - y).abs()).sum(), (m * ssim).sum()
    grads = []
    for g_l1, g_ssim, s_l1, s_ssim in R.COEFS:
        (gr,) = torch.autograd.grad(g_l1 * s_l1 * l1 + g_ssim * s_ssim * ss, xe, retain_graph=True)
        grads.append(gr.detach())
    return dict(l1=l1.detach(), ssim=ss.detach(), M=(M1.detach(), M2.detach(), M3.detach()), grads=grads)


def masked_reference(x_full, gt_full, mask_full, y0, y1, dtype, E=None, wrong=None):
    """The definition in `dtype` on the CPU.  x_full [C,H,W] float32 (finite everywhere), gt_full uint8 [C,H,W],
    mask_full uint8 [H,W], E float32 [3,4] or None.  -> dict(l1, ssim, M: (M1, M2, M3) [C,rows,W], grads: dL/dx per entry of
    leaf_refs.COEFS, gE: dL/dE [3,4] per entry (None without E)).  wrong=None is the reference; the others restate it with
    ONE deliberate mistake: "x_only" (y is not masked), "maps" (the mask multiplies the L1 / SSIM maps, not the inputs),
    "grad_no_m" (dL/dx = g', the factor m forgotten), "m256" (m = byte / 256), "pad" (the SSIM window sees the masked
    image's neighbouring rows around the band instead of zeros)."""
    C, H, W = x_full.shape
    x = x_full.to(dtype)
    Ed = None if E is None else E.to(dtype)
    m = mask_full.to(dtype) / (256.0 if wrong == "m256" else 255.0)
    xe = apply_exposure(x, Ed)                      # (rows outside the band matter to wrong == "pad" only)
    gtf = gt_full.to(dtype)
    if wrong == "maps":
        r = _maps_wrong(xe[:, y0:y1], gtf[:, y0:y1] / 255.0, m[y0:y1], dtype)
        mg = torch.ones_like(m)
    else:
        xp = m * xe
        # loss_reference forms y = gt / 255 itself: hand it m * gt (x_only: gt)
        yp255 = gtf if wrong == "x_only" else m * gtf
        r = R.loss_reference(xp, yp255, y0, y1, dtype, wrong="pad" if wrong == "pad" else None)
        mg = torch.ones_like(m) if wrong == "grad_no_m" else m
    mb, xb = mg[y0:y1], x[:, y0:y1]
    gx, gE = [], []
    for gp in r["grads"]:
        gm = mb * gp
        if Ed is None:
            gx.append(gm)
            gE.append(None)
            continue
        gx.append(torch.stack([sum(Ed[c, k] * gm[c] for c in range(3)) for k in range(3)]))
        ge = torch.zeros(3, 4, dtype=dtype)
        for c in range(3):
            for k in range(3):
                ge[c, k] = (gm[c] * xb[k]).sum()
            ge[c, 3] = gm[c].sum()
        gE.append(ge)
    return dict(l1=r["l1"], ssim=r["ssim"], M=r["M"], grads=gx, gE=gE)


def _inputs(image_family, ename, C, H, W, seed):
    """x float32 [C,H,W] such that x_e = A x + b is the family's image moved away from y: |x_e - y| >= 4e-4 or an exact tie
    (no exposure: leaf_refs.loss_inputs as it is, |x - y| >= 1e-4 or a tie)"""
    xp, gt, ties = R.loss_inputs(image_family, C, H, W, seed=seed)
    if ename is None:
        return xp, gt
    E = torch.tensor(EXPOSURES[ename], dtype=f32)
    y = gt.double() / 255.0
    d = xp.double() - y
    xp64 = torch.where((d.abs() < 4e-4) & ~ties, y + torch.where(d >= 0, 4e-4, -4e-4), xp.double())
    A, b = E[:, :3].double(), E[:, 3].double()
    x = torch.linalg.solve(A, (xp64 - b[:, None, None]).reshape(3, -1)).reshape(C, H, W).float()
    return x, gt


def signs_agree(x, gt, mask, E):
    """sign(x' - y') of the fp32 and of the fp64 restatement, on every pixel"""
    s = []
    for dt in (f32, f64):
        m = mask.to(dt) / 255.0
        d = m * apply_exposure(x.to(dt), E) - m * (gt.to(dt) / 255.0)
        s.append(torch.sign(d).to(torch.int8))
    return bool((s[0] == s[1]).all())


_CASES = {}


def masked_case(mfamily, ename, C, H, W, y0, y1):
    """Inputs and both references of one (mask family, exposure, shape), computed once and never modified:
    dict(x [C,H,W] finite, img (x with NaN rows outside the band), gt_full, gt (band), mask_full [H,W], mask (band), E,
    r64, r32).  sign(x' - y') agrees between fp32 and fp64 on every pixel (asserted); a draw that violates it is replaced
    by the next seed's."""
    key = (mfamily, ename, C, H, W, y0, y1)
    if key in _CASES:
        return _CASES[key]
    E = None if ename is None else torch.tensor(EXPOSURES[ename], dtype=f32)
    for seed in range(8):
        x, gt = _inputs(IMAGE_OF[mfamily], ename, C, H, W, seed)
        mask = make_mask(mfamily, H, W, y0, y1, seed)
        if signs_agree(x, gt, mask, E):
            break
    else:
        raise AssertionError(f"{key}: no seed gives inputs whose sign(x' - y') agrees in fp32 and fp64")
    assert signs_agree(x, gt, mask, E)
    img = torch.full_like(x, float("nan"))  # rows outside the band are NaN: zero padding has to BE zero padding
    img[:, y0:y1] = x[:, y0:y1]
    _CASES[key] = dict(x=x, img=img, gt_full=gt, gt=gt[:, y0:y1].contiguous(), mask_full=mask,
                       mask=mask[y0:y1].contiguous(), E=E, seed=seed,
                       r64=masked_reference(x, gt, mask, y0, y1, f64, E), r32=masked_reference(x, gt, mask, y0, y1, f32, E))
    return _CASES[key]
