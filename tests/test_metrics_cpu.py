"""CPU side of the evaluation metrics (csrc/metrics.hip, evaluation.py): the fp64 restatement of tests/metric_refs.py is
pinned on what the reference's own l1_loss / psnr / ssim gave (tests/golden/reference_eval_metrics.json), the tolerance
the GPU files apply separates it from restatements with one deliberate mistake, band sums are additive, and everything
that needs no device (argument validation, the evaluation schedule, the report line) behaves."""
import json
import math
import os

import pytest
import torch

import leaf_refs as R
import metric_refs as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_eval_metrics.json")
GSR_EINVAL = -1


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(a, b, tol):
    return (math.isinf(a) and a == b) or abs(a - b) <= tol


@pytest.mark.parametrize("family", R.FAMILIES)
def test_fp64_restatement_agrees_with_the_reference_functions(family):
    """bounds: 7-9 x the distance of the reference's own float32 values from fp64 on these inputs (1.5e-5 relative on L1,
    1.1e-4 dB, 1.3e-5 on SSIM; the worst case is `flat`, where y = 128 / 255 rounds the same way everywhere)"""
    cases = [c for c in _golden()["metrics"] if c["family"] == family]
    assert len(cases) == 4
    for c in cases:
        C, H, W = c["C"], c["H"], c["W"]
        x, gt, _ = R.loss_inputs(family, C, H, W)
        chk = [float(x.double().sum()), float(x.double().abs().sum()), float(gt.double().sum())]
        assert all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(chk, c["checksum"])), "inputs are not the frozen ones"
        l1, psnr, ssim = M.metrics_of(M.metric_sums(x, gt, 0, H, torch.float64), H, W)
        print(f"{family} {C}x{H}x{W}: l1 rel {abs(l1 - c['l1']) / c['l1']:.3g}, psnr {abs(psnr - c['psnr']):.3g} dB, "
              f"ssim {abs(ssim - c['ssim']):.3g}")
        assert _same(l1, c["l1"], 1e-4 * abs(c["l1"]))
        assert _same(psnr, c["psnr"], 1e-3)
        assert _same(ssim, c["ssim"], 1e-4)


_REFS = {}


def _refs(family, C, H, W, y0, y1, quantize=False):
    key = (family, C, H, W, y0, y1, quantize)
    if key not in _REFS:
        x, gt, _ = R.loss_inputs(family, C, H, W)
        _REFS[key] = (x, gt, M.metric_sums(x, gt, y0, y1, torch.float64, quantize=quantize),
                      M.metric_sums(x, gt, y0, y1, torch.float32, quantize=quantize))
    return _REFS[key]


@pytest.mark.parametrize("wrong", M.WRONG)
def test_tolerance_rejects_a_wrong_restatement(wrong):
    """every deliberately wrong restatement lies outside the GPU test's tolerance (K x the unit of metric_refs.sum_units;
    for "pooled" that tolerance carried through the PSNR) on at least one case of the GPU test's list"""
    quantize = wrong == "trunc"
    worst, where = 0.0, None
    for family in R.FAMILIES:
        for C, H, W, y0, y1 in M.CASES:
            x, gt, r64, r32 = _refs(family, C, H, W, y0, y1, quantize)
            if wrong == "pooled":
                if (y0, y1) != (0, H):
                    continue
                unit = M.sum_units(r64, r32)
                if not bool((r64[:, 1] > 0).all()):
                    continue  # (an exact match: inf either way)
                rel = float((M.K * unit[:, 1] / r64[:, 1]).max())
                tol = M.psnr_tolerance_db(rel)
                margin = abs(M.metrics_of(r64, H, W, wrong="pooled")[1] - M.metrics_of(r64, H, W)[1]) / tol
            else:
                bad = M.metric_sums(x, gt, y0, y1, torch.float64, quantize=quantize, wrong=wrong)
                margin = M.worst_margin(bad, r64, r32)
            if margin > worst and not math.isinf(margin):  # (inf: a sum that is exactly 0 in both precisions, unit 0)
                worst, where = margin, (family, C, H, W, y0, y1)
            # and the plain fp32 restatement is inside the tolerance by construction
            assert M.worst_margin(r32, r64, r32) <= 1.0 / M.K + 1e-12
    print(f"wrong={wrong}: worst |wrong - ref| / tolerance = {worst:.3g} at {where}")
    assert worst > 1.0


@pytest.mark.parametrize("W", [100, 101])
def test_band_sums_are_additive_in_fp64(W):
    """the per-pixel terms of a band are the full image's, bit for bit (the window sees the neighbouring rows, never a
    zero band edge), so the band sums add up to the full image's up to the order of the additions: 1e-13 relative"""
    from oracle.loss_oracle import ssim_map

    H = 96
    x, gt, _ = R.loss_inputs("noise", 3, H, W)
    xd, yd = x.double().clamp(0, 1), gt.double() / 255.0
    full_map = ssim_map(xd, yd)
    full = M.metric_sums(x, gt, 0, H, torch.float64)
    total = torch.zeros_like(full)
    for y0, y1 in ((0, 16), (16, 64), (64, 96)):
        a, b = max(0, y0 - 5), min(H, y1 + 5)
        crop = ssim_map(xd[:, a:b], yd[:, a:b])[:, y0 - a:y0 - a + (y1 - y0)]  # the rows the kernel reads, nothing else
        assert torch.equal(crop, full_map[:, y0:y1])
        total += M.metric_sums(x, gt, y0, y1, torch.float64)
    assert float(((total - full).abs() / full.abs()).max()) <= 1e-13
    # with the band padded by zeros instead, the sums do NOT add up
    padded = sum(M.metric_sums(x, gt, y0, y1, torch.float64, wrong="bandpad") for y0, y1 in ((0, 16), (16, 64), (64, 96)))
    assert float(((padded - full).abs() / full.abs()).max()) > 1e-4


def test_quantiser_is_the_saved_byte():
    x = torch.tensor([[[-0.2, 0.0, 0.5 / 255, 0.49999 / 255, 1.5 / 255, 0.5, 1.0 - 1e-7, 1.0, 1.7]]])
    q = M.quantize_u8(x)
    assert q.tolist() == [[[0, 0, 1, 0, 2, 128, 255, 255, 255]]]
    assert M.quantize_u8(x, wrong="trunc").tolist() == [[[0, 0, 0, 0, 1, 127, 254, 255, 255]]]


def test_argument_validation_needs_no_device():
    from diff_gaussian_rasterization import _lib

    lib = _lib.lib
    p = 0x1000  # a non-null pointer that is never dereferenced: every call below is refused before any device work
    ok = dict(C=3, H=64, W=64, img=p, ics=64 * 64, gt=p, gcs=64 * 64, y0=0, y1=64, flags=0, part=p, out=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsr_image_metrics(a["C"], a["H"], a["W"], a["img"], a["ics"], a["gt"], a["gcs"], a["y0"], a["y1"],
                                     a["flags"], a["part"], a["out"], None)

    for bad in (dict(img=None), dict(gt=None), dict(part=None), dict(y0=-1), dict(y0=64), dict(y0=10, y1=10),
                dict(y0=20, y1=10), dict(y1=65), dict(flags=4), dict(flags=-1), dict(flags=1 | 2 | 8), dict(C=0),
                dict(H=0), dict(W=0), dict(ics=64 * 64 - 1), dict(gcs=0)):
        assert call(**bad) == GSR_EINVAL, bad
    assert lib.gsr_image_metrics_finalize(3, 12, None, p, None) == GSR_EINVAL
    assert lib.gsr_image_metrics_finalize(3, 12, p, None, None) == GSR_EINVAL
    assert lib.gsr_image_metrics_finalize(3, 13, p, p, None) == GSR_EINVAL  # not a multiple of the channels
    assert lib.gsr_image_metrics_finalize(0, 0, p, p, None) == GSR_EINVAL
    assert lib.gsr_image_metrics_num_partials(3, 0, 64) == 0
    assert lib.gsr_image_metrics_num_partials(3, 33, 65) == 3 * 2 * 3
    assert lib.gsr_image_metrics_num_partials(3, 1080, 1920) == lib.gsr_l1_ssim_num_partials(3, 1080, 1920)
    assert lib.gsr_abi_version() == 15  # the entry points are an addition


def test_operator_refuses_host_tensors_and_forms_the_metrics():
    import diff_gaussian_rasterization as dgr

    assert "image_metrics" in dgr.__all__ and "metrics_from_sums" in dgr.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.image_metrics(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8, dtype=torch.uint8))
    x, gt, _ = R.loss_inputs("noise", 3, 33, 37)
    sums = M.metric_sums(x, gt, 0, 33, torch.float64)
    got = [float(v) for v in dgr.metrics_from_sums(sums, 33, 37)]
    want = M.metrics_of(sums, 33, 37)
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, want))
    batch = dgr.metrics_from_sums(torch.stack([sums, 2 * sums]), 33, 37)
    assert batch[0].shape == (2,) and abs(float(batch[1][0]) - want[1]) <= 1e-12
    exact = sums.clone()
    exact[:, :2] = 0.0
    l1, psnr, _ = dgr.metrics_from_sums(exact, 33, 37)
    assert float(l1) == 0.0 and math.isinf(float(psnr)) and float(psnr) > 0  # psnr(image, image) is inf in the reference


def test_schedule_equals_the_reference():
    import utils.general_utils as utils

    rows = _golden()["schedule"]
    assert len(rows) > 300 and any(r[4] for r in rows) and not all(r[4] for r in rows)
    for it, bsz, interval, residual, want in rows:
        assert bool(utils.check_update_at_this_iter(it, bsz, interval, residual)) == want, (it, bsz, interval)


@pytest.mark.parametrize("l1,psnr", [(0.0123456789012345, 23.456789012345678), (1e-7, float("inf")), (0.5, 5.0)])
def test_report_line_round_trips_through_the_analysis_script(l1, psnr):
    from evaluation import report_line

    line = report_line(7000, "test", l1, psnr) + "\n"
    assert line.startswith("[ITER 7000] Evaluating test: L1 ")
    # examples/mip360/analyze_results.py:59-64 of the reference
    assert float(line.split("L1 ")[1].split(" PSNR")[0]) == l1
    assert float(line.split("PSNR ")[1]) == psnr
