"""The MASK instantiations of csrc/loss.hip (include/gsraster.h, N1m): x' = m x (m (A x + b) with an exposure) and
y' = m y formed inside the fused L1 + SSIM kernels.  Every element of the partial sums, the three maps, the image gradient
and the exposure gradient against the fp64 restatement (tests/masked_loss_refs.py), in the static and the device-band
form, with guard bands around every buffer and NaN rows around every band; the two exact properties of the header (an
all-255 mask writes the unmasked launches' bits; a zero byte gives an exactly zero gradient whatever finite x lies under
it).  Tolerance: helpers.assert_elem_close with K = 8 -- K times the restatement's own fp32 error, never the kernel's.
Observed ratios are printed (`RATIO masked ...`); EXPERIMENTS.md, "leaf-kernel element-wise noise", keeps the maxima."""
import math

import pytest
import torch

import leaf_refs as R
import masked_loss_refs as MR
from helpers import assert_elem_close
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

K = 8
SUM_FLOOR = 2e-5  # the relative floor of the two sums (test_gpu_loss_edges.SUM_FLOOR)
GSR_EINVAL = -1
f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32

CASES = [(3, 1, 1, 0, 1), (3, 11, 11, 0, 11), (3, 33, 36, 0, 33), (3, 33, 37, 0, 33), (3, 96, 100, 27, 70),
         (3, 96, 101, 32, 64)]
CASE_C1 = (1, 33, 37, 0, 33)


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _cap_of(rows, dyn):
    """the device-band form runs at a capacity of 40 rows where the band fits, at the row count otherwise"""
    return None if not dyn else (40 if rows <= 40 else rows)


def run_masked(dev, img, gt_band, mask_band, y0, y1, E=None, cap=None, coefs=R.COEFS, mask_off=0):
    """One masked forward (+ one backward per entry of `coefs`) through the C ABI on guarded buffers.  cap=None: the
    static form (band pointer, band_rows NULL); cap >= rows: the device-band form at that capacity.  mask_off: bytes of
    misalignment of the mask's base.  The rows of gt and mask above the band keep the guards' 0xA5 bytes.
    -> dict(partials [nb, 2], M [3, C, rows, W], grads, gE ([3,4] each, or None without E))"""
    lib = _lib()
    C, H, W = img.shape
    rows = y1 - y0
    cap_rows = rows if cap is None else cap
    cs = gs = H * W
    gI = Guard(C * cs, f32, dev)
    gI.t.view(C, cs)[:, :H * W] = img.reshape(C, H * W).to(dev)
    gG = Guard(C * cap_rows * W, u8, dev)
    gG.t.view(C, cap_rows, W)[:, :rows] = gt_band.to(dev)
    gK = Guard(cap_rows * W, u8, dev, offset=mask_off)
    gK.t.view(cap_rows, W)[:rows] = mask_band.to(dev)
    nb_cap, nb = lib.gsr_l1_ssim_num_partials(C, cap_rows, W), lib.gsr_l1_ssim_num_partials(C, rows, W)
    ne_cap, ne = lib.gsr_l1_ssim_exposure_num_partials(cap_rows, W), lib.gsr_l1_ssim_exposure_num_partials(rows, W)
    assert nb == C * math.ceil(rows / 32) * math.ceil(W / 32) and nb_cap >= nb
    gP = Guard(2 * nb_cap, f32, dev)
    gM = [Guard(C * cap_rows * W, f32, dev) for _ in range(3)]
    gB, gE = Guard(2, i32, dev), Guard(12, f32, dev)
    gB.t.copy_(torch.tensor([y0, y1], dtype=i32))
    if E is not None:
        gE.t.copy_(E.reshape(-1))
    for g in [gI, gG, gK, gP, gB, gE] + gM:
        g.seal()
    img_ptr = gI.ptr + 4 * y0 * W if cap is None else gI.ptr
    band_ptr = None if cap is None else gB.ptr
    e_ptr = None if E is None else gE.ptr
    rc = lib.gsr_l1_ssim_forward_masked(C, cap_rows, W, img_ptr, cs, gG.ptr, gK.ptr, gP.ptr, gM[0].ptr, gM[1].ptr,
                                        gM[2].ptr, band_ptr, e_ptr, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for g, what in ((gI, "image"), (gG, "ground truth"), (gK, "mask"), (gB, "band"), (gE, "exposure")):
        g.check(what, whole=True)
    gP.check("partials")
    partials = gP.t.view(nb_cap, 2).cpu()
    assert bool(torch.isfinite(partials).all()), "a partial sum was not written or is not finite"
    assert bool((partials[nb:] == 0).all()), "slots above the band's tile count must be exactly zero"
    in_band = torch.zeros(C, cap_rows, W, dtype=torch.bool, device=dev)
    in_band[:, :rows] = True
    for i, g in enumerate(gM):
        g.check(f"map {i}")
        g.untouched(~in_band.reshape(-1), f"map {i}, rows above the band")
    M = torch.stack([g.t.view(C, cap_rows, W)[:, :rows] for g in gM]).cpu()
    assert bool(torch.isfinite(M).all()), "a map element of the band was not written or is not finite"
    grads, gEs = [], []
    band_px = torch.zeros(C, gs, dtype=torch.bool, device=dev)
    band_px[:, y0 * W:y1 * W] = True
    for g_l1, g_ssim, s_l1, s_ssim in coefs:
        gD, gEP, gGE = Guard(C * gs, f32, dev), Guard(12 * ne_cap, f32, dev), Guard(12, f32, dev)
        g1, g2 = Guard(1, f32, dev), Guard(1, f32, dev)
        g1.t.fill_(g_l1), g2.t.fill_(g_ssim)
        for g in [gD, gEP, gGE, g1, g2] + gM + [gP]:
            g.seal()
        grad_ptr = gD.ptr + 4 * y0 * W if cap is None else gD.ptr
        rc = lib.gsr_l1_ssim_backward_masked(C, cap_rows, W, img_ptr, cs, gG.ptr, gK.ptr, gM[0].ptr, gM[1].ptr, gM[2].ptr,
                                             g1.ptr, g2.ptr, s_l1, s_ssim, grad_ptr, gs, band_ptr, e_ptr,
                                             None if E is None else gEP.ptr, None if E is None else gGE.ptr, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        for g in [gI, gG, gK, gB, gE, g1, g2, gP] + gM:
            g.check("backward input", whole=True)
        gD.check("gradient")
        gD.untouched(~band_px.reshape(-1), "gradient outside the band (the launch writes the band's rows only)")
        gr = gD.t.view(C, gs)[:, y0 * W:y1 * W].reshape(C, rows, W).cpu()
        assert bool(torch.isfinite(gr).all()), "a gradient element of the band was not written or is not finite"
        grads.append(gr)
        if E is None:  # nothing of the exposure's outputs is touched without one
            gEP.check("exposure partials", whole=True), gGE.check("exposure gradient", whole=True)
            gEs.append(None)
            continue
        gEP.check("exposure partials"), gGE.check("exposure gradient")
        ep = gEP.t.view(ne_cap, 12).cpu()
        assert bool(torch.isfinite(ep).all()), "a partial row was not written or is not finite"
        assert bool((ep[ne:] == 0).all()), "partial rows above the band's tile count must be exactly zero"
        ge = gGE.t.view(3, 4).cpu()
        assert bool(torch.isfinite(ge).all()), "an exposure gradient was not written or is not finite"
        gEs.append(ge)
    return dict(partials=partials[:nb].clone(), M=M, grads=grads, gE=gEs)


def _check_against_fp64(res, c, tag):
    r64, r32 = c["r64"], c["r32"]
    for j, name in enumerate(("l1", "ssim")):
        got = float(res["partials"][:, j].double().sum())
        want, w32 = float(r64[name]), float(r32[name])
        unit = max(abs(w32 - want), SUM_FLOOR * abs(want))
        ratio = abs(got - want) / unit if unit > 0 else (0.0 if got == want else float("inf"))  # (an exact 0 sum)
        print(f"RATIO masked sum_{name} {tag} {ratio:.4g}")
        assert ratio <= K, f"{tag}: sum {name}: got {got!r}, fp64 {want!r}, error / unit = {ratio:.3g} > {K}"
    for i in range(3):
        ratio = assert_elem_close(res["M"][i], r64["M"][i], r32["M"][i], K=K, what=f"{tag} M{i + 1}")
        print(f"RATIO masked map{i + 1} {tag} {ratio:.4g}")
    for i, gr in enumerate(res["grads"]):
        ratio = assert_elem_close(gr, r64["grads"][i], r32["grads"][i], K=K, what=f"{tag} grad[{i}]")
        print(f"RATIO masked grad{i} {tag} {ratio:.4g}")
    for i, ge in enumerate(res["gE"]):
        if ge is not None:
            ratio = assert_elem_close(ge, r64["gE"][i], r32["gE"][i], K=K, what=f"{tag} grad_exposure[{i}]")
            print(f"RATIO masked gE{i} {tag} {ratio:.4g}")


def _bit_equal(a, b, what):
    assert torch.equal(a["partials"].view(i32), b["partials"].view(i32)), f"{what}: partial sums differ in bits"
    assert torch.equal(a["M"].view(i32), b["M"].view(i32)), f"{what}: maps differ in bits"
    assert len(a["grads"]) == len(b["grads"]) > 0
    for x, y in zip(a["grads"], b["grads"]):
        assert torch.equal(x.view(i32), y.view(i32)), f"{what}: image gradients differ in bits"
    for x, y in zip(a.get("gE", []), b.get("gE", [])):
        if x is not None and y is not None:
            assert torch.equal(x.view(i32), y.view(i32)), f"{what}: exposure gradients differ in bits"


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("ename", [None, "full", "offset"])
@pytest.mark.parametrize("mfamily", MR.MASK_FAMILIES)
@pytest.mark.parametrize("C,H,W,y0,y1", CASES)
def test_masked_every_element_against_fp64(device, mfamily, ename, dyn, C, H, W, y0, y1):
    c = MR.masked_case(mfamily, ename, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    res = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"], cap=cap)
    _check_against_fp64(res, c, f"{mfamily} {ename} {C}x{H}x{W}[{y0}:{y1}] cap{cap}")


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("mfamily", MR.MASK_FAMILIES)
def test_masked_one_channel_against_fp64(device, mfamily, dyn):
    C, H, W, y0, y1 = CASE_C1
    c = MR.masked_case(mfamily, None, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    res = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, cap=cap)
    _check_against_fp64(res, c, f"{mfamily} None {C}x{H}x{W}[{y0}:{y1}] cap{cap}")


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("C,H,W,y0,y1", CASES + [CASE_C1])
def test_ones_mask_is_bit_equal_to_the_plain_launches(device, dyn, C, H, W, y0, y1):
    """gsr_l1_ssim_forward / _backward (static) and their _band forms (device band)"""
    from test_gpu_loss_edges import run_loss

    c = MR.masked_case("ones", None, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    res = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, cap=cap)
    plain = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap)
    _bit_equal(res, plain, f"ones mask against the plain launch, cap {cap}")


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("ename", ["full", "offset"])
@pytest.mark.parametrize("C,H,W,y0,y1", CASES)
def test_ones_mask_is_bit_equal_to_the_exposure_pair(device, ename, dyn, C, H, W, y0, y1):
    from test_gpu_exposure_loss import run_expo

    c = MR.masked_case("ones", ename, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    res = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"], cap=cap)
    expo = run_expo(device, c["img"], c["gt"], y0, y1, c["E"], cap=cap)
    _bit_equal(res, expo, f"ones mask against the exposure pair, cap {cap}")
    assert all(g is not None for g in res["gE"])


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("ename", [None, "full"])
@pytest.mark.parametrize("mfamily", ["zeros", "edge", "checker"])
@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 33, 36, 0, 33), (3, 96, 100, 27, 70), (3, 96, 101, 32, 64)])
def test_zero_bytes_give_zero_gradients_and_hide_x(device, mfamily, ename, dyn, C, H, W, y0, y1):
    """where m = 0 the gradient is exactly zero (of every channel, with and without an exposure), and rewriting x there
    with other finite values -- other signs, other magnitudes -- changes no output bit"""
    c = MR.masked_case(mfamily, ename, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    a = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"], cap=cap)
    dead = (c["mask"] == 0)
    assert bool(dead.any())
    for gr in a["grads"]:
        assert bool((gr[:, dead] == 0).all()), "a pixel under a zero mask byte received a gradient"
        assert bool((gr[:, dead].view(i32) == 0).all()), "the zero under a zero mask byte is not +0"
    g = torch.Generator().manual_seed(5)
    other = (torch.rand(c["img"].shape, generator=g) - 0.5) * 2.0e3
    other[:, ::2] = -other[:, ::2].abs() * 1e-3
    img2 = c["img"].clone()
    band = img2[:, y0:y1]
    band[:, dead] = other[:, y0:y1][:, dead]
    assert not torch.equal(img2[:, y0:y1], c["img"][:, y0:y1])
    b = run_masked(device, img2, c["gt"], c["mask"], y0, y1, E=c["E"], cap=cap)
    _bit_equal(a, b, "x rewritten under the zero mask bytes")


@pytest.mark.parametrize("ename", [None, "full"])
@pytest.mark.parametrize("dyn", [False, True])
def test_misaligned_mask_is_bit_equal_to_the_aligned_launch(device, ename, dyn):
    """W = 100: the aligned launch fetches the mask four bytes at a time, a base off by one byte takes the scalar path"""
    C, H, W, y0, y1 = 3, 96, 100, 27, 70
    c = MR.masked_case("soft", ename, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    a = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"], cap=cap)
    b = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"], cap=cap, mask_off=1)
    _bit_equal(a, b, "mask base off by one byte")


@pytest.mark.parametrize("ename", [None, "full"])
@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 33, 36, 0, 33), (3, 96, 101, 32, 64)])
def test_masked_backward_is_reproducible(device, ename, C, H, W, y0, y1):
    c = MR.masked_case("soft", ename, C, H, W, y0, y1)
    a = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"])
    b = run_masked(device, c["img"], c["gt"], c["mask"], y0, y1, E=c["E"])
    _bit_equal(a, b, "two launches on the same inputs")


@pytest.mark.parametrize("ename", [None, "full"])
@pytest.mark.parametrize("W", [100, 101])
def test_masked_capacity_above_the_band(device, ename, W):
    """capacity 96 on a 43-row band: the slots above the band's tile count are zero (run_masked asserts it) and every
    result equals the launch sized for the band, bit for bit"""
    c = MR.masked_case("soft", ename, 3, 96, W, 27, 70)
    big = run_masked(device, c["img"], c["gt"], c["mask"], 27, 70, E=c["E"], cap=96)
    own = run_masked(device, c["img"], c["gt"], c["mask"], 27, 70, E=c["E"], cap=43)
    _bit_equal(big, own, "capacity 96 against capacity 43")


def test_masked_argument_checks_launch_nothing(device):
    lib = _lib()
    C, H, W = 3, 33, 36
    c = MR.masked_case("soft", "full", C, H, W, 0, H)
    n4 = 4 * H * W  # room for a 4-channel call
    gI, gG, gK = Guard(n4, f32, device), Guard(n4, u8, device), Guard(H * W, u8, device)
    gI.t[:C * H * W] = c["img"].reshape(-1).to(device)
    gG.t[:C * H * W] = c["gt"].reshape(-1).to(device)
    gK.t.copy_(c["mask"].reshape(-1))
    gP, gD = Guard(2 * lib.gsr_l1_ssim_num_partials(4, H, W), f32, device), Guard(n4, f32, device)
    gM = [Guard(n4, f32, device) for _ in range(3)]
    gB, g1, gE = Guard(2, i32, device), Guard(1, f32, device), Guard(12, f32, device)
    gEP, gGE = Guard(12 * lib.gsr_l1_ssim_exposure_num_partials(H, W), f32, device), Guard(12, f32, device)
    gB.t.copy_(torch.tensor([0, H], dtype=i32))
    g1.t.fill_(1.0)
    gE.t.copy_(c["E"].reshape(-1))
    every = [gI, gG, gK, gP, gD, gB, g1, gE, gEP, gGE] + gM
    for g in every:
        g.seal()
    s = _stream()
    m = [g.ptr for g in gM]

    def fwd(ch=C, rows=H, width=W, mask=gK.ptr, expo=gE.ptr, partials=gP.ptr, band=None):
        return lib.gsr_l1_ssim_forward_masked(ch, rows, width, gI.ptr, H * W, gG.ptr, mask, partials, m[0], m[1], m[2],
                                              band, expo, s)

    def bwd(ch=C, rows=H, width=W, mask=gK.ptr, expo=gE.ptr, ep=gEP.ptr, ge=gGE.ptr, band=None):
        return lib.gsr_l1_ssim_backward_masked(ch, rows, width, gI.ptr, H * W, gG.ptr, mask, m[0], m[1], m[2], g1.ptr,
                                               g1.ptr, 1.0, 1.0, gD.ptr, H * W, band, expo, ep, ge, s)

    for band in (None, gB.ptr):
        for expo in (None, gE.ptr):
            assert fwd(mask=None, expo=expo, band=band) == GSR_EINVAL
            assert bwd(mask=None, expo=expo, band=band) == GSR_EINVAL
            for kw in (dict(ch=0), dict(rows=0), dict(rows=-1), dict(width=0)):
                assert fwd(expo=expo, band=band, **kw) == GSR_EINVAL and bwd(expo=expo, band=band, **kw) == GSR_EINVAL
        for ch in (1, 4):
            assert fwd(ch=ch, band=band) == GSR_EINVAL and bwd(ch=ch, band=band) == GSR_EINVAL
        assert fwd(partials=None, band=band) == GSR_EINVAL
        assert bwd(ep=None, band=band) == GSR_EINVAL and bwd(ge=None, band=band) == GSR_EINVAL
    torch.cuda.synchronize()
    for g in every:  # outputs still hold their poison, the guards are intact
        g.check("argument checks", whole=True)


@pytest.mark.parametrize("ename", [None, "full"])
@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 96, 100, 27, 70), (3, 33, 37, 0, 33)])
def test_masked_wrapper_against_fp64(device, C, H, W, y0, y1, dyn, ename):
    """fused_band_loss_masked: loss, Ll1, ssim and both gradients against autograd in fp64 through the band oracle"""
    from diff_gaussian_rasterization import fused_band_loss_masked
    from oracle.loss_oracle import band_loss

    c = MR.masked_case("soft", ename, C, H, W, y0, y1)
    rows, n, lam = y1 - y0, H * W * 3, 0.2
    ref = {}
    for dt in (f64, f32):
        x = c["x"][:, y0:y1].to(dt).clone().requires_grad_(True)
        E = None if c["E"] is None else c["E"].to(dt).clone().requires_grad_(True)
        m = c["mask"].to(dt) / 255.0
        # band_loss forms y = gt / 255 itself: hand it m * gt
        loss, Ll1, ssim = band_loss(m * MR.apply_exposure(x, E), m * c["gt"].to(dt), H, W, lam)
        loss.backward()
        ref[dt] = (loss.detach(), Ll1.detach(), ssim.detach(), x.grad, None if E is None else E.grad)
    xi = c["img"].to(device).requires_grad_(True)
    Ei = None if c["E"] is None else c["E"].to(device).requires_grad_(True)
    if dyn:
        cap = rows + 7
        gt = torch.full((C, cap, W), 0xA5, dtype=u8, device=device)
        gt[:, :rows] = c["gt"].to(device)
        mk = torch.full((1, cap, W), 0xA5, dtype=u8, device=device)
        mk[0, :rows] = c["mask"].to(device)
        out = fused_band_loss_masked(xi, gt, mk, 0, 0, lam, n, band_rows=torch.tensor([y0, y1], dtype=i32, device=device),
                                     exposure=Ei)
    else:
        out = fused_band_loss_masked(xi, c["gt"].to(device), c["mask"].to(device), y0, y1, lam, n, exposure=Ei)
    out[0].backward()
    tag = f"{ename} {C}x{H}x{W}[{y0}:{y1}] dyn={dyn}"
    for j, name in enumerate(("loss", "Ll1", "ssim")):
        want, w32 = float(ref[f64][j]), float(ref[f32][j])
        ratio = abs(float(out[j].detach()) - want) / max(abs(w32 - want), SUM_FLOOR * abs(want))
        print(f"RATIO masked wrapper_{name} {tag} {ratio:.4g}")
        assert ratio <= K, (name, float(out[j].detach()), want)
    assert not out[1].requires_grad and not out[2].requires_grad
    g = xi.grad.cpu()
    ratio = assert_elem_close(g[:, y0:y1], ref[f64][3], ref[f32][3], K=K, what="wrapper image gradient")
    print(f"RATIO masked wrapper_grad {tag} {ratio:.4g}")
    outside = torch.ones(H, dtype=torch.bool)
    outside[y0:y1] = False
    assert bool((g[:, outside] == 0).all()), "the gradient outside the band must be exactly zero"
    if Ei is not None:
        assert tuple(Ei.grad.shape) == (3, 4)
        ratio = assert_elem_close(Ei.grad.cpu(), ref[f64][4], ref[f32][4], K=K, what="wrapper exposure gradient")
        print(f"RATIO masked wrapper_gE {tag} {ratio:.4g}")
