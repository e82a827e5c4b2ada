"""csrc/metrics.hip at its edges: the [C,3] sums of every flag combination through the C ABI, sum by sum against the fp64
restatement (tests/metric_refs.py, pinned on the reference's own functions by tests/test_metrics_cpu.py), with guard bands
around every buffer, NaN image rows outside the rows the window may read, misaligned bases and padded channel strides.
Tolerance: helpers.assert_elem_close with, per sum, the unit max(|fp32 torch restatement - fp64|, 2e-5 |fp64|) and K = 8 --
the restatement's own noise, never the kernel's.  Observed ratios are printed (`RATIO metrics ...`); EXPERIMENTS.md,
"leaf-kernel element-wise noise", keeps the maxima."""
import math

import pytest
import torch

import leaf_refs as R
import metric_refs as M
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

f32, u8, i64, f64 = torch.float32, torch.uint8, torch.int64, torch.float64
FLAGS = [0, M.QUANTIZE, M.NO_SSIM, M.QUANTIZE | M.NO_SSIM]


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


_REFS = {}


def _case(family, C, H, W, y0, y1):
    """inputs and all references of one (family, case), computed once and never modified"""
    key = (family, C, H, W, y0, y1)
    if key not in _REFS:
        x, gt, _ = R.loss_inputs(family, C, H, W)
        a, b = max(0, y0 - 5), min(H, y1 + 5)
        img = torch.full_like(x, float("nan"))  # rows the window may not read are NaN ...
        img[:, a:b] = x[:, a:b]                 # ... rows inside the halo are real data
        band_only = torch.full_like(x, float("nan"))
        band_only[:, y0:y1] = x[:, y0:y1]       # (NO_SSIM reads the band alone)
        gtk = torch.full_like(gt, 0xA5)
        gtk[:, a:b] = gt[:, a:b]
        ref = {}
        for q in (False, True):
            ref[q] = (M.metric_sums(x, gt, y0, y1, f64, quantize=q), M.metric_sums(x, gt, y0, y1, f32, quantize=q))
        _REFS[key] = dict(x=x, gt=gt, img=img, band_only=band_only, gtk=gtk, ref=ref, q=M.quantize_u8(x)[:, y0:y1])
    return _REFS[key]


def run_metrics(dev, img, gt, y0, y1, flags, img_off=0, gt_off=0, img_extra=0, gt_extra=0, want_u8=True):
    """one gsr_image_metrics + two gsr_image_metrics_finalize through the C ABI on guarded buffers.  *_off: misalignment of
    a base (elements), *_extra: added to the channel stride.  -> dict(sums float64 [C,3] (cpu), u8 [C,rows,W] or None)"""
    lib = _lib()
    C, H, W = img.shape
    rows = y1 - y0
    ics, gcs = H * W + img_extra, H * W + gt_extra
    gI = Guard(C * ics, f32, dev, offset=img_off)
    gI.t.view(C, ics)[:, :H * W] = img.reshape(C, H * W).to(dev)
    gG = Guard(C * gcs, u8, dev, offset=gt_off)
    gG.t.view(C, gcs)[:, :H * W] = gt.reshape(C, H * W).to(dev)
    nb = lib.gsr_image_metrics_num_partials(C, rows, W)
    assert nb == C * math.ceil(rows / 32) * math.ceil(W / 32)
    gP = Guard(3 * nb, f32, dev)
    gU = Guard(C * rows * W, u8, dev)
    gS = [Guard(3 * C, i64, dev) for _ in range(2)]  # doubles, compared as bits (NaN padding would not compare equal)
    for g in [gI, gG, gP, gU] + gS:
        g.seal()
    rc = lib.gsr_image_metrics(C, H, W, gI.ptr, ics, gG.ptr, gcs, y0, y1, flags, gP.ptr, gU.ptr if want_u8 else None,
                               _stream())
    assert rc == 0
    for g in gS:
        assert lib.gsr_image_metrics_finalize(C, nb, gP.ptr, g.ptr, _stream()) == 0
    torch.cuda.synchronize()
    gI.check("image", whole=True), gG.check("ground truth", whole=True)
    gP.check("partials"), gS[0].check("sums"), gS[1].check("sums (second finalize)")
    partials = gP.t.view(nb, 3).cpu()
    assert bool(torch.isfinite(partials).all()), "a partial sum was not written or is not finite"
    assert torch.equal(gS[0].t, gS[1].t), "two runs of the finalize differ in bits"
    sums = gS[0].t.view(f64).view(C, 3).cpu()
    # the finalize is the fixed-order fp64 sum of the channel's partials: within 2^-50 of the exact sum's magnitude
    exact = partials.double().view(C, nb // C, 3)
    assert bool(((sums - exact.sum(1)).abs() <= 2.0 ** -50 * exact.abs().sum(1)).all())
    if want_u8:
        gU.check("out_u8")
        out = gU.t.view(C, rows, W).cpu()
    else:
        gU.check("out_u8 (not asked for)", whole=True)
        out = None
    return dict(sums=sums, u8=out)


def _check(res, c, flags, tag):
    r64, r32 = c["ref"][bool(flags & M.QUANTIZE)]
    if flags & M.NO_SSIM:
        assert bool((res["sums"][:, 2] == 0).all()), f"{tag}: NO_SSIM must leave the third sum exactly 0"
        M.check_sums(res["sums"], r64, r32, tag, columns=(0, 1))
    else:
        M.check_sums(res["sums"], r64, r32, tag)
    if res["u8"] is not None:
        assert torch.equal(res["u8"], c["q"]), f"{tag}: out_u8 is not mul(255).add_(0.5).clamp_(0, 255).to(uint8)"


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C,H,W,y0,y1", M.CASES)
def test_metrics_every_sum_against_fp64(device, family, C, H, W, y0, y1):
    c = _case(family, C, H, W, y0, y1)
    for flags in FLAGS:
        tag = f"{family} {C}x{H}x{W}[{y0}:{y1}] flags={flags}"
        img = c["band_only"] if flags & M.NO_SSIM else c["img"]
        _check(run_metrics(device, img, c["gtk"], y0, y1, flags), c, flags, tag)


LAYOUTS = {"image_base_4B": dict(img_off=1), "gt_base_1B": dict(gt_off=1), "image_cstride_odd": dict(img_extra=1),
           "image_cstride_padded": dict(img_extra=8), "gt_cstride_odd": dict(gt_extra=3),
           "gt_cstride_padded": dict(gt_extra=8), "all": dict(img_off=3, gt_off=2, img_extra=5, gt_extra=7)}


@pytest.mark.parametrize("which", sorted(LAYOUTS))
@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 33, 36, 0, 33), (3, 96, 100, 27, 70)])
def test_metrics_layouts_are_bit_equal_to_the_dense_aligned_launch(device, which, C, H, W, y0, y1):
    """a misaligned base or an odd channel stride takes the scalar template, a padded stride keeps the vector one: the
    same arithmetic in the same order either way -- same bits, and the fp64 check again"""
    c = _case("noise", C, H, W, y0, y1)
    for flags in FLAGS:
        img = c["band_only"] if flags & M.NO_SSIM else c["img"]
        dense = run_metrics(device, img, c["gtk"], y0, y1, flags)
        other = run_metrics(device, img, c["gtk"], y0, y1, flags, **LAYOUTS[which])
        _check(other, c, flags, f"noise layout {which} {C}x{H}x{W}[{y0}:{y1}] flags={flags}")
        assert torch.equal(other["sums"].view(i64), dense["sums"].view(i64)), (which, flags)
        assert torch.equal(other["u8"], dense["u8"])


@pytest.mark.parametrize("flags", FLAGS)
def test_metrics_without_out_u8_gives_the_same_sums(device, flags):
    c = _case("noise", 3, 96, 100, 27, 70)
    img = c["band_only"] if flags & M.NO_SSIM else c["img"]
    a = run_metrics(device, img, c["gtk"], 27, 70, flags)
    b = run_metrics(device, img, c["gtk"], 27, 70, flags, want_u8=False)
    assert torch.equal(a["sums"].view(i64), b["sums"].view(i64))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("W", [100, 101])
def test_metrics_band_sums_add_up_to_the_full_image(device, family, W):
    """bands (0,16), (16,64), (64,96) of H = 96: their sums, added, and one full-image call are both inside the tolerance
    of the SAME fp64 value (tests/test_metrics_cpu.py shows that in fp64 the per-pixel terms of a band are the full
    image's bit for bit)"""
    H = 96
    full_case = _case(family, 3, H, W, 0, H)
    for flags in (0, M.QUANTIZE):
        r64, r32 = full_case["ref"][bool(flags)]
        full = run_metrics(device, full_case["img"], full_case["gtk"], 0, H, flags)["sums"]
        total = torch.zeros_like(full)
        for y0, y1 in ((0, 16), (16, 64), (64, 96)):
            c = _case(family, 3, H, W, y0, y1)
            total += run_metrics(device, c["img"], c["gtk"], y0, y1, flags)["sums"]
        M.check_sums(full, r64, r32, f"{family} 3x{H}x{W} full flags={flags}")
        M.check_sums(total, r64, r32, f"{family} 3x{H}x{W} bands-added flags={flags}")


def test_metrics_argument_checks_launch_nothing(device):
    lib = _lib()
    C, H, W = 3, 33, 36
    c = _case("noise", C, H, W, 0, H)
    gI, gG = Guard(C * H * W, f32, device), Guard(C * H * W, u8, device)
    gI.t.copy_(c["x"].reshape(-1)), gG.t.copy_(c["gt"].reshape(-1))
    nb = lib.gsr_image_metrics_num_partials(C, H, W)
    gP, gU, gS = Guard(3 * nb, f32, device), Guard(C * H * W, u8, device), Guard(3 * C, i64, device)
    every = [gI, gG, gP, gU, gS]
    for g in every:
        g.seal()
    s = _stream()
    for args in ((None, gG.ptr, 0, H, 0, gP.ptr), (gI.ptr, None, 0, H, 0, gP.ptr), (gI.ptr, gG.ptr, 0, H, 0, None),
                 (gI.ptr, gG.ptr, -1, H, 0, gP.ptr), (gI.ptr, gG.ptr, 5, 5, 0, gP.ptr), (gI.ptr, gG.ptr, 6, 5, 0, gP.ptr),
                 (gI.ptr, gG.ptr, 0, H + 1, 0, gP.ptr), (gI.ptr, gG.ptr, 0, H, 4, gP.ptr)):
        img, gt, y0, y1, flags, part = args
        assert lib.gsr_image_metrics(C, H, W, img, H * W, gt, H * W, y0, y1, flags, part, gU.ptr, s) == -1, args
    assert lib.gsr_image_metrics_finalize(C, nb + 1, gP.ptr, gS.ptr, s) == -1
    assert lib.gsr_image_metrics_finalize(C, nb, None, gS.ptr, s) == -1
    torch.cuda.synchronize()
    for g in every:
        g.check("argument checks", whole=True)


@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 96, 100, 27, 70), (3, 33, 37, 0, 33)])
def test_image_metrics_wrapper_against_fp64(device, C, H, W, y0, y1):
    """the operator module's entry: same sums, the quantised band, and an exact match scores inf dB"""
    from diff_gaussian_rasterization import image_metrics, kernel_timer, metrics_from_sums

    c = _case("noise", C, H, W, y0, y1)
    for ssim in (True, False):
        for quantize in (False, True):
            flags = (M.QUANTIZE if quantize else 0) | (0 if ssim else M.NO_SSIM)
            out = torch.empty((C, y1 - y0, W), dtype=u8, device=device)
            img = (c["img"] if ssim else c["band_only"]).to(device)
            sums = image_metrics(img, c["gtk"].to(device), y0, y1, ssim=ssim, quantize=quantize, out_u8=out)
            assert sums.dtype == f64 and sums.is_cuda and tuple(sums.shape) == (C, 3)
            _check(dict(sums=sums.cpu(), u8=out.cpu()), c, flags, f"wrapper {C}x{H}x{W}[{y0}:{y1}] flags={flags}")
    # the saved image scored against itself
    full = c["x"].to(device)
    q = torch.empty((C, H, W), dtype=u8, device=device)
    image_metrics(full, c["gt"].to(device), ssim=False, out_u8=q)
    kernel_timer.reset()
    kernel_timer.enabled = True
    try:
        same = image_metrics(full, q, quantize=True)
        torch.cuda.synchronize()
        assert kernel_timer.summary_ms()["image_metrics"][0] == 1
    finally:
        kernel_timer.enabled = False
        kernel_timer.reset()
    l1, psnr, ssim = metrics_from_sums(same, H, W)
    assert float(l1) == 0.0 and math.isinf(float(psnr)) and abs(float(ssim) - 1.0) <= 1e-6
