"""Plain references of the evaluation metrics (csrc/metrics.hip, evaluation.py), with the deliberately wrong ones: shared
by tests/test_metrics_cpu.py (which pins the fp64 restatement on values the reference's own functions produced and shows
that the tolerance separates right from wrong) and the GPU files that apply the same tolerance to the HIP kernels."""
import math

import torch

from helpers import assert_elem_close
from oracle.loss_oracle import ssim_map

K = 8
SUM_FLOOR = 2e-5  # relative floor of a sum's unit: the one tests/test_gpu_loss_edges.py uses for its two sums
QUANTIZE, NO_SSIM = 1, 2  # include/gsraster.h: GSR_METRICS_*
WRONG = ("noclamp", "y256", "bandpad", "pooled", "trunc")

# the case list of tests/test_gpu_loss_edges.py: (C, H, W, y0, y1)
CASES = [(3, 1, 1, 0, 1), (3, 1, 37, 0, 1), (1, 5, 4, 0, 5), (3, 11, 11, 0, 11),       # degenerate sizes
         (3, 32, 32, 0, 32), (3, 64, 64, 0, 64),                                      # exact tiles
         (3, 33, 36, 0, 33), (4, 40, 68, 0, 40),                                      # vector loads, partial tiles on both axes
         (3, 33, 37, 0, 33), (3, 83, 131, 0, 83)]                                     # scalar template
CASES += [(3, 96, W, y0, y1) for W in (100, 101) for y0, y1 in ((0, 1), (95, 96), (27, 70), (32, 64))]


def quantize_u8(image, wrong=None):
    """the byte a saved PNG holds: mul(255).add_(0.5).clamp_(0, 255).to(uint8) of the clamped image.  Defined in float32
    (that IS the definition: the sequence runs on the rendered float32 image), whatever precision the metrics then use."""
    x = image.float().clamp(0.0, 1.0)
    if wrong == "trunc":
        return x.mul(255).clamp_(0, 255).to(torch.uint8)
    return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def metric_sums(image, gt_u8, y0, y1, dtype, ssim=True, quantize=False, wrong=None):
    """-> [C,3] in `dtype`: per channel (sum |x - y|, sum (x - y)^2, sum ssim_map(x, y)) over rows [y0, y1) of the full image
    [C,H,W] against the full ground truth: x = clamp(image, 0, 1) (quantize: quantize_u8 / 255), y = clamp(gt / 255, 0, 1) as
    train_internal.py:471-478 forms them, oracle.loss_oracle.ssim_map on the FULL image (zero padding at the image's edges
    only).  wrong: ONE deliberate mistake -- "noclamp" (x = image), "y256" (y = gt / 256), "bandpad" (the SSIM window sees
    the band alone, zero rows around it), "trunc" (the quantiser truncates); ("pooled" is a mistake of metrics_of)."""
    if quantize:
        x = quantize_u8(image, wrong).to(dtype) / 255.0
    else:
        x = image.to(dtype) if wrong == "noclamp" else torch.clamp(image.to(dtype), 0.0, 1.0)
    y = torch.clamp(gt_u8.to(dtype) / (256.0 if wrong == "y256" else 255.0), 0.0, 1.0)
    d = (x - y)[:, y0:y1]
    out = torch.zeros(image.shape[0], 3, dtype=dtype)
    out[:, 0] = d.abs().sum(dim=(1, 2))
    out[:, 1] = (d * d).sum(dim=(1, 2))
    if ssim:
        m = ssim_map(x[:, y0:y1], y[:, y0:y1]) if wrong == "bandpad" else ssim_map(x, y)[:, y0:y1]
        out[:, 2] = m.sum(dim=(1, 2))
    return out


def metrics_of(sums, H, W, wrong=None):
    """sums [C,3] of a whole image -> python floats (l1, psnr, ssim): psnr = the mean of the per-channel PSNRs
    (utils/image_utils.py:19-21 followed by .mean()); wrong="pooled": ONE PSNR of the mse pooled over the channels"""
    s = sums.double()
    C, n = s.shape[0], float(H * W)
    if wrong == "pooled":
        psnr = 20.0 * torch.log10(1.0 / torch.sqrt(s[:, 1].sum() / (C * n)))
    else:
        psnr = (20.0 * torch.log10(1.0 / torch.sqrt(s[:, 1] / n))).mean()
    return float(s[:, 0].sum() / (C * n)), float(psnr), float(s[:, 2].sum() / (C * n))


def sum_units(r64, r32):
    """per sum: max(distance of the plain fp32 restatement from the fp64 one, SUM_FLOOR * |fp64|) -- never the kernel's"""
    r64, r32 = r64.double(), r32.double()
    return torch.maximum((r32 - r64).abs(), SUM_FLOOR * r64.abs())


def check_sums(got, r64, r32, tag, columns=(0, 1, 2), quiet=False):
    """every sum on its own through helpers.assert_elem_close with its own unit -> worst observed ratio per column"""
    got, r64 = got.double().cpu(), r64.double()
    unit = sum_units(r64, r32)
    worst = {}
    for j in columns:
        for c in range(r64.shape[0]):
            a = r64[c, j].reshape(1)
            ratio = assert_elem_close(got[c, j].reshape(1), a, a + unit[c, j], K=K, what=f"{tag} sum[{c},{j}]")
            worst[j] = max(worst.get(j, 0.0), ratio)
    if not quiet:
        for j, name in zip((0, 1, 2), ("l1", "sse", "ssim")):
            if j in worst:
                print(f"RATIO metrics sum_{name} {tag} {worst[j]:.4g}")
    return worst


def worst_margin(wrong_sums, r64, r32, columns=(0, 1, 2)):
    """max over the sums of |wrong - fp64| / (K * unit): > 1 means the GPU test's tolerance rejects `wrong_sums`"""
    unit = sum_units(r64, r32)
    err = (wrong_sums.double() - r64.double()).abs()
    m = 0.0
    for j in columns:
        for c in range(r64.shape[0]):
            u, e = float(unit[c, j]), float(err[c, j])
            m = max(m, (e / (K * u)) if u > 0 else (0.0 if e == 0 else math.inf))
    return m


def psnr_tolerance_db(rel):
    """a relative error `rel` of a channel's sum of squares moves its PSNR = -10 log10(SSE / n) by at most
    10 |log10(1 - rel)| dB (the larger of the two directions); the mean over the channels by no more"""
    return 10.0 * abs(math.log10(1.0 - rel)) if rel < 1.0 else math.inf
