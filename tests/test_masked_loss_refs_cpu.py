"""CPU side of the masked-loss checks (include/gsraster.h, N1m): the fp32 mask weight on all 256 bytes, the tolerance of
tests/test_gpu_masked_loss.py (helpers.assert_elem_close, K = 8, on the fp32 restatement against fp64) accepting the right
reference and rejecting one deliberately wrong reference per mistake the kernels can make, and the new entry points'
argument checks (they return before any device work, so they run without a GPU)."""
import pytest
import torch

import leaf_refs as R
import masked_loss_refs as MR
from helpers import assert_elem_close

K = 8
SUM_FLOOR = 2e-5  # the relative floor of the two sums (test_gpu_loss_edges.SUM_FLOOR)
f32, f64 = torch.float32, torch.float64
SHAPES = [(3, 33, 37, 0, 33), (3, 96, 100, 27, 70)]


def test_mask_weight_on_all_256_bytes():
    """m = (float)byte * (1.0f / 255.0f): exactly 0 and 1 at the ends, strictly increasing, within 1.5 fp32 ulp of
    byte / 255 (the constant is off by up to 2^-24 relative, which is one ulp of a product just below a power of two, and
    the product is rounded once more) -- and a correctly rounded byte / 255 lies within half an ulp"""
    b = torch.arange(256, dtype=torch.uint8)
    m = MR.mask_weight_fp32(b)
    assert m.dtype == f32
    assert float(m[0]) == 0.0 and float(m[255]) == 1.0
    assert bool((m[1:] > m[:-1]).all())
    exact = b.double() / 255.0
    ulp = torch.tensor([2.0 ** (torch.tensor(max(float(v), 2.0 ** -126)).log2().floor().item() - 23) for v in exact],
                       dtype=f64)
    assert bool(((m.double() - exact).abs() <= 1.5 * ulp).all())
    assert bool((((b.float() / 255.0).double() - exact).abs() <= 0.5 * ulp).all())


def _flat(r):
    """the checked tensors of a reference, by name"""
    out = {"l1": r["l1"].reshape(1), "ssim": r["ssim"].reshape(1)}
    for i in range(3):
        out[f"M{i + 1}"] = r["M"][i]
    for i, g in enumerate(r["grads"]):
        out[f"grad{i}"] = g
    for i, g in enumerate(r["gE"]):
        if g is not None:
            out[f"gE{i}"] = g
    return out


def _accepts(got, r64, r32):
    """the GPU file's check, on a dict of tensors: -> (ok, the name of the first tensor that fails)"""
    a, w, s = _flat(got), _flat(r64), _flat(r32)
    for name in w:
        if name in ("l1", "ssim"):
            want = float(w[name])
            unit = max(abs(float(s[name]) - want), SUM_FLOOR * abs(want))
            err = abs(float(a[name]) - want)
            if not (err <= K * unit):
                return False, name
            continue
        try:
            assert_elem_close(a[name], w[name], s[name], K=K, what=name)
        except AssertionError:
            return False, name
    return True, None


@pytest.mark.parametrize("ename", [None, "full", "offset"])
@pytest.mark.parametrize("mfamily", MR.MASK_FAMILIES)
@pytest.mark.parametrize("C,H,W,y0,y1", SHAPES)
def test_tolerance_accepts_the_fp32_restatement(mfamily, ename, C, H, W, y0, y1):
    c = MR.masked_case(mfamily, ename, C, H, W, y0, y1)
    ok, name = _accepts(c["r32"], c["r64"], c["r32"])
    assert ok, name
    # and the mask does what its name says inside the band
    m = c["mask"]
    assert m.shape == (y1 - y0, W) and m.dtype == torch.uint8
    if mfamily == "ones":
        assert bool((m == 255).all())
    if mfamily == "zeros":
        assert bool((m == 0).all())
        for g in c["r64"]["grads"]:
            assert bool((g == 0).all())
    if mfamily == "edge":
        assert bool((m[:, :MR.EDGE_COLUMN] == 0).all()) and bool((m[:, MR.EDGE_COLUMN:] == 255).all())
    if mfamily == "toprows":
        assert bool((m[:3] == 0).all()) and bool((m[3:] == 255).all())


@pytest.mark.parametrize("ename", [None, "full"])
@pytest.mark.parametrize("wrong", MR.WRONGS)
def test_tolerance_rejects_every_wrong_reference(wrong, ename):
    """each mistake, restated in fp64, is thrown out by the check on at least one mask family (and never on `ones` for the
    mistakes an all-255 mask cannot show)"""
    C, H, W, y0, y1 = 3, 96, 100, 27, 70
    rejected = []
    for mfamily in MR.MASK_FAMILIES:
        c = MR.masked_case(mfamily, ename, C, H, W, y0, y1)
        bad = MR.masked_reference(c["x"], c["gt_full"], c["mask_full"], y0, y1, f64, c["E"], wrong=wrong)
        ok, name = _accepts(bad, c["r64"], c["r32"])
        if not ok:
            rejected.append((mfamily, name))
    print(f"WRONG {wrong} exposure={ename}: rejected on {rejected}")
    assert rejected, f"the tolerance accepts the wrong reference {wrong!r} on every mask family"
    fams = [f for f, _ in rejected]
    if wrong in ("x_only", "maps", "grad_no_m"):
        assert "ones" not in fams  # m = 1 everywhere: these restatements ARE the definition
        assert "soft" in fams and "checker" in fams
    if wrong == "pad":
        assert "toprows" in fams  # the family that tells a masked row from padding


def test_manual_chain_rule_is_autograd():
    """dL/dx = m g' and the 12 sums of masked_reference against torch.autograd through m (A x + b) end to end"""
    from oracle.loss_oracle import l1_map, ssim_map

    C, H, W, y0, y1 = 3, 33, 37, 0, 33
    for ename in (None, "full"):
        c = MR.masked_case("soft", ename, C, H, W, y0, y1)
        x = c["x"].double().clone().requires_grad_(True)
        E = None if c["E"] is None else c["E"].double().clone().requires_grad_(True)
        m = c["mask_full"].double() / 255.0
        xp, yp = m * MR.apply_exposure(x, E), m * (c["gt_full"].double() / 255.0)
        l1, ss = l1_map(xp, yp).sum(), ssim_map(xp, yp).sum()
        assert torch.allclose(l1, c["r64"]["l1"], rtol=1e-12) and torch.allclose(ss, c["r64"]["ssim"], rtol=1e-12)
        for i, (g_l1, g_ssim, s_l1, s_ssim) in enumerate(R.COEFS):
            gs = torch.autograd.grad(g_l1 * s_l1 * l1 + g_ssim * s_ssim * ss, [x] + ([E] if E is not None else []),
                                     retain_graph=True)
            assert torch.allclose(gs[0], c["r64"]["grads"][i], rtol=1e-9, atol=1e-13)
            if E is not None:
                assert torch.allclose(gs[1], c["r64"]["gE"][i], rtol=1e-9, atol=1e-12)


def test_signs_agree_on_every_generated_case():
    for mfamily in MR.MASK_FAMILIES:
        for ename in (None, "full", "offset"):
            for C, H, W, y0, y1 in SHAPES:
                c = MR.masked_case(mfamily, ename, C, H, W, y0, y1)
                assert MR.signs_agree(c["x"], c["gt_full"], c["mask_full"], c["E"])


def test_masked_abi_symbols_and_refusals():
    """both symbols exported, ABI 15 unchanged, and every refusal returns GSR_EINVAL (-1) before any launch.  Dummy
    non-zero integers stand for device pointers: nothing is dereferenced."""
    import ctypes

    from diff_gaussian_rasterization import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "gsr_l1_ssim_forward_masked") and hasattr(raw, "gsr_l1_ssim_backward_masked")
    lib = _lib.lib
    assert lib.gsr_abi_version() == 15 and _lib.ABI_VERSION == 15
    d = 0x1000

    def fwd(C=3, rows=32, W=32, img=d, gt=d, mask=d, partials=d, maps=(d, d, d), band=None, expo=None):
        return lib.gsr_l1_ssim_forward_masked(C, rows, W, img, 32 * 32, gt, mask, partials, *maps, band, expo, None)

    def bwd(C=3, rows=32, W=32, img=d, gt=d, mask=d, maps=(d, d, d), g=d, grad=d, band=None, expo=None, ep=None, ge=None):
        return lib.gsr_l1_ssim_backward_masked(C, rows, W, img, 32 * 32, gt, mask, *maps, g, g, 1.0, 1.0, grad, 32 * 32,
                                               band, expo, ep, ge, None)

    for band in (None, d):
        assert fwd(mask=None, band=band) == -1 and bwd(mask=None, band=band) == -1
        for kw in (dict(C=0), dict(rows=0), dict(rows=-3), dict(W=0)):
            assert fwd(band=band, **kw) == -1 and bwd(band=band, **kw) == -1, kw
        for ch in (1, 4):
            assert fwd(C=ch, expo=d, band=band) == -1 and bwd(C=ch, expo=d, ep=d, ge=d, band=band) == -1
        assert bwd(expo=d, ep=None, ge=d, band=band) == -1 and bwd(expo=d, ep=d, ge=None, band=band) == -1
        assert fwd(img=None, band=band) == -1 and fwd(gt=None, band=band) == -1 and fwd(partials=None, band=band) == -1
        assert fwd(maps=(d, None, d), band=band) == -1
        assert bwd(img=None, band=band) == -1 and bwd(gt=None, band=band) == -1 and bwd(grad=None, band=band) == -1
        assert bwd(maps=(d, d, None), band=band) == -1 and bwd(g=None, band=band) == -1
