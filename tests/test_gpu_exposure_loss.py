"""The exposure instantiations of csrc/loss.hip (include/gsraster.h, N1x): x' = A x + b formed inside the fused L1 + SSIM
kernels.  Every element of the three maps, the image gradient and the 12 exposure gradients against the fp64 restatement
(x' formed on the CPU, zero outside the band, leaf_refs.loss_reference on it, the three gradient formulas), in the static
and the device-band form, with guard bands around every buffer and NaN rows around every band.  Tolerance:
helpers.assert_elem_close -- K times the restatement's own fp32 error, never the kernel's.  Observed ratios are printed
(`RATIO ...`); EXPERIMENTS.md, "leaf-kernel element-wise noise", keeps the maxima."""
import math

import pytest
import torch

import leaf_refs as R
from helpers import assert_elem_close
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

K = 8
SUM_FLOOR = 2e-5  # the relative floor of the two sums (test_gpu_loss_edges.SUM_FLOOR)
GSR_EINVAL = -1
f32, f64, u8, i32 = torch.float32, torch.float64, torch.uint8, torch.int32

CASES = [(3, 1, 1, 0, 1), (3, 11, 11, 0, 11), (3, 32, 32, 0, 32), (3, 33, 36, 0, 33), (3, 33, 37, 0, 33),
         (3, 96, 100, 27, 70), (3, 96, 101, 32, 64)]
FAMILIES = ["noise", "smooth", "range"]
EXPOSURES = {
    # well conditioned: identity plus off-diagonal entries of magnitude <= 0.2, |b| <= 0.1
    "full": [[1.10, 0.15, -0.20, 0.05], [-0.10, 0.90, 0.20, -0.10], [0.20, -0.15, 1.05, 0.08]],
    # a large offset: padding that leaks b (instead of 0) moves every border window
    "offset": [[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.125]],
    "identity": [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
}


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _cap_of(rows, dyn):
    """the device-band form runs at a capacity of 40 rows where the band fits, at the row count otherwise"""
    return None if not dyn else (40 if rows <= 40 else rows)


def _apply(x, E):
    """x' [3,R,W] = A x + b in x's dtype"""
    E = E.to(x.dtype)
    return torch.stack([E[c, 0] * x[0] + E[c, 1] * x[1] + E[c, 2] * x[2] + E[c, 3] for c in range(3)])


def reference(x_band, E, gt, H, y0, y1, dtype):
    """The definition in `dtype` on the CPU: x' of the band's pixels, 0 outside the band, leaf_refs.loss_reference on it
    (sums, maps, g' per entry of COEFS), then dL/dx = A^T g', dL/dA[c][k] = sum g'[c] x[k], dL/db[c] = sum g'[c]."""
    xb = x_band.to(dtype)
    Ed = E.to(dtype)
    C, rows, W = xb.shape
    full = torch.zeros(C, H, W, dtype=dtype)
    full[:, y0:y1] = _apply(xb, Ed)
    r = R.loss_reference(full, gt, y0, y1, dtype)
    gx, gE = [], []
    for gp in r["grads"]:
        gx.append(torch.stack([sum(Ed[c, k] * gp[c] for c in range(3)) for k in range(3)]))
        ge = torch.zeros(3, 4, dtype=dtype)
        for c in range(3):
            for k in range(3):
                ge[c, k] = (gp[c] * xb[k]).sum()
            ge[c, 3] = gp[c].sum()
        gE.append(ge)
    return dict(l1=r["l1"], ssim=r["ssim"], M=r["M"], grads=gx, gE=gE)


_REFS = {}


def _case(family, ename, C, H, W, y0, y1):
    """inputs and both references of one (family, exposure, case), computed once and never modified.  x' is drawn from the
    family and moved away from y (|x' - y| >= 4e-4), x solves A x + b = x' in fp64 and is rounded to fp32: the fp32 and
    the fp64 x' of that x then keep |x' - y| >= 1e-4, so sign(x' - y) is the same in both -- asserted here."""
    key = (family, ename, C, H, W, y0, y1)
    if key in _REFS:
        return _REFS[key]
    E = torch.tensor(EXPOSURES[ename], dtype=f32)
    xp, gt_full, _ = R.loss_inputs(family, C, H, W)
    y = gt_full.double() / 255.0
    d = xp.double() - y
    xp64 = torch.where(d.abs() < 4e-4, y + torch.where(d >= 0, 4e-4, -4e-4), xp.double())
    if ename == "identity":
        x = xp64.float()
    else:
        A, b = E[:, :3].double(), E[:, 3].double()
        x = torch.linalg.solve(A, (xp64 - b[:, None, None]).reshape(3, -1)).reshape(C, H, W).float()
    for dt in (f32, f64):  # the property the sign of the L1 term rests on, on the x' both precisions form
        dd = (_apply(x.to(dt), E) - (gt_full.to(dt) * torch.tensor(1.0 / 255.0, dtype=dt) if dt == f32 else y)).abs()
        assert bool((dd >= 1e-4).all()), f"|x' - y| < 1e-4 somewhere ({dt})"
    img = torch.full_like(x, float("nan"))  # rows outside the band are NaN: zero padding has to BE zero padding
    img[:, y0:y1] = x[:, y0:y1]
    gt = gt_full[:, y0:y1].contiguous()
    xb = x[:, y0:y1]
    _REFS[key] = dict(img=img, gt=gt, E=E, xb=xb, r64=reference(xb, E, gt_full, H, y0, y1, f64),
                      r32=reference(xb, E, gt_full, H, y0, y1, f32))
    return _REFS[key]


def run_expo(dev, img, gt_band, y0, y1, E, cap=None, coefs=R.COEFS):
    """One exposure forward (+ one backward per entry of `coefs`) through the C ABI on guarded buffers.  cap=None: the
    static form (band pointer, band_rows NULL); cap >= rows: the device-band form at that capacity.
    -> dict(partials [nb, 2], M [3, C, rows, W], grads, gE [3,4] each, ep: the [ne_cap, 12] partial rows of the last
    backward, ne: the band's own row count)"""
    lib = _lib()
    C, H, W = img.shape
    rows = y1 - y0
    cap_rows = rows if cap is None else cap
    cs = gs = H * W
    gI = Guard(C * cs, f32, dev)
    gI.t.view(C, cs)[:, :H * W] = img.reshape(C, H * W).to(dev)
    gG = Guard(C * cap_rows * W, u8, dev)
    gG.t.view(C, cap_rows, W)[:, :rows] = gt_band.to(dev)
    nb_cap, nb = lib.gsr_l1_ssim_num_partials(C, cap_rows, W), lib.gsr_l1_ssim_num_partials(C, rows, W)
    ne_cap, ne = lib.gsr_l1_ssim_exposure_num_partials(cap_rows, W), lib.gsr_l1_ssim_exposure_num_partials(rows, W)
    assert ne == math.ceil(rows / 32) * math.ceil(W / 32) and ne_cap >= ne and nb == 3 * ne
    gP = Guard(2 * nb_cap, f32, dev)
    gM = [Guard(C * cap_rows * W, f32, dev) for _ in range(3)]
    gB, gE = Guard(2, i32, dev), Guard(12, f32, dev)
    gB.t.copy_(torch.tensor([y0, y1], dtype=i32))
    gE.t.copy_(E.reshape(-1))
    for g in [gI, gG, gP, gB, gE] + gM:
        g.seal()
    img_ptr = gI.ptr + 4 * y0 * W if cap is None else gI.ptr
    band_ptr = None if cap is None else gB.ptr
    rc = lib.gsr_l1_ssim_forward_exposure(C, cap_rows, W, img_ptr, cs, gG.ptr, gP.ptr, gM[0].ptr, gM[1].ptr, gM[2].ptr,
                                          band_ptr, gE.ptr, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for g, what in ((gI, "image"), (gG, "ground truth"), (gB, "band"), (gE, "exposure")):
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
    grads, gEs, ep = [], [], None
    band_px = torch.zeros(C, gs, dtype=torch.bool, device=dev)
    band_px[:, y0 * W:y1 * W] = True
    for g_l1, g_ssim, s_l1, s_ssim in coefs:
        gD, gEP, gGE = Guard(C * gs, f32, dev), Guard(12 * ne_cap, f32, dev), Guard(12, f32, dev)
        g1, g2 = Guard(1, f32, dev), Guard(1, f32, dev)
        g1.t.fill_(g_l1), g2.t.fill_(g_ssim)
        for g in [gD, gEP, gGE, g1, g2] + gM + [gP]:
            g.seal()
        grad_ptr = gD.ptr + 4 * y0 * W if cap is None else gD.ptr
        rc = lib.gsr_l1_ssim_backward_exposure(C, cap_rows, W, img_ptr, cs, gG.ptr, gM[0].ptr, gM[1].ptr, gM[2].ptr,
                                               g1.ptr, g2.ptr, s_l1, s_ssim, grad_ptr, gs, band_ptr, gE.ptr, gEP.ptr,
                                               gGE.ptr, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        for g in [gI, gG, gB, gE, g1, g2, gP] + gM:
            g.check("backward input", whole=True)
        gD.check("gradient"), gEP.check("exposure partials"), gGE.check("exposure gradient")
        gD.untouched(~band_px.reshape(-1), "gradient outside the band (the launch writes the band's rows only)")
        gr = gD.t.view(C, gs)[:, y0 * W:y1 * W].reshape(C, rows, W).cpu()
        assert bool(torch.isfinite(gr).all()), "a gradient element of the band was not written or is not finite"
        ep = gEP.t.view(ne_cap, 12).cpu()
        assert bool(torch.isfinite(ep).all()), "a partial row was not written or is not finite"
        assert bool((ep[ne:] == 0).all()), "partial rows above the band's tile count must be exactly zero"
        ge = gGE.t.view(3, 4).cpu()
        assert bool(torch.isfinite(ge).all()), "an exposure gradient was not written or is not finite"
        grads.append(gr), gEs.append(ge)
    return dict(partials=partials[:nb].clone(), M=M, grads=grads, gE=gEs, ep=ep, ne=ne)


def _check_sums(partials, r64, r32, tag):
    for j, name in enumerate(("l1", "ssim")):
        got = float(partials[:, j].double().sum())
        want, w32 = float(r64[name]), float(r32[name])
        unit = max(abs(w32 - want), SUM_FLOOR * abs(want))
        ratio = abs(got - want) / unit if unit > 0 else (0.0 if got == want else float("inf"))
        print(f"RATIO exposure sum_{name} {tag} {ratio:.4g}")
        assert ratio <= K, f"{tag}: sum {name}: got {got!r}, fp64 {want!r}, error / unit = {ratio:.3g} > {K}"


def _check_gE(res, c, tag):
    for i, ge in enumerate(res["gE"]):
        r64, r32 = c["r64"]["gE"][i], c["r32"]["gE"][i]
        print(f"INFO exposure gE{i} {tag} restatement fp32 error {float((r32.double() - r64).abs().max()):.3g} "
              f"kernel error {float((ge.double() - r64).abs().max()):.3g} max |ref| {float(r64.abs().max()):.3g}")
        ratio = assert_elem_close(ge, r64, r32, K=K, what=f"{tag} grad_exposure[{i}]")
        print(f"RATIO exposure gE{i} {tag} {ratio:.4g}")


def _check_against_fp64(res, c, tag):
    r64, r32 = c["r64"], c["r32"]
    _check_sums(res["partials"], r64, r32, tag)
    for i in range(3):
        ratio = assert_elem_close(res["M"][i], r64["M"][i], r32["M"][i], K=K, what=f"{tag} M{i + 1}")
        print(f"RATIO exposure map{i + 1} {tag} {ratio:.4g}")
    for i, gr in enumerate(res["grads"]):
        ratio = assert_elem_close(gr, r64["grads"][i], r32["grads"][i], K=K, what=f"{tag} grad[{i}]")
        print(f"RATIO exposure grad{i} {tag} {ratio:.4g}")
    _check_gE(res, c, tag)


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("ename", ["full", "offset"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("C,H,W,y0,y1", CASES)
def test_exposure_every_element_against_fp64(device, family, ename, dyn, C, H, W, y0, y1):
    c = _case(family, ename, C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    res = run_expo(device, c["img"], c["gt"], y0, y1, c["E"], cap=cap)
    _check_against_fp64(res, c, f"{family} {ename} {C}x{H}x{W}[{y0}:{y1}] cap{cap}")


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("C,H,W,y0,y1", CASES)
def test_identity_exposure_is_bit_equal_to_the_plain_launch(device, dyn, C, H, W, y0, y1):
    from test_gpu_loss_edges import run_loss

    c = _case("noise", "identity", C, H, W, y0, y1)
    cap = _cap_of(y1 - y0, dyn)
    res = run_expo(device, c["img"], c["gt"], y0, y1, c["E"], cap=cap)
    plain = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap)
    assert torch.equal(res["partials"].view(i32), plain["partials"].view(i32)), "partial sums differ in bits"
    assert torch.equal(res["M"].view(i32), plain["M"].view(i32)), "maps differ in bits"
    for a, b in zip(res["grads"], plain["grads"]):
        assert torch.equal(a, b), "image gradients differ"
    _check_gE(res, c, f"noise identity {C}x{H}x{W}[{y0}:{y1}] cap{cap}")


@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 33, 36, 0, 33), (3, 96, 101, 32, 64)])
def test_backward_is_reproducible(device, C, H, W, y0, y1):
    c = _case("noise", "full", C, H, W, y0, y1)
    a = run_expo(device, c["img"], c["gt"], y0, y1, c["E"])
    b = run_expo(device, c["img"], c["gt"], y0, y1, c["E"])
    for x, y in zip(a["gE"] + a["grads"], b["gE"] + b["grads"]):
        assert torch.equal(x.view(i32), y.view(i32)), "two launches on the same inputs differ in bits"


@pytest.mark.parametrize("W", [100, 101])
def test_capacity_above_the_band(device, W):
    """capacity 96 on a 43-row band: the slots above the band's tile count are zero (run_expo asserts it for the loss
    partials and the exposure rows) and every result equals the launch sized for the band, bit for bit"""
    lib = _lib()
    c = _case("noise", "full", 3, 96, W, 27, 70)
    big = run_expo(device, c["img"], c["gt"], 27, 70, c["E"], cap=96)
    own = run_expo(device, c["img"], c["gt"], 27, 70, c["E"], cap=43)
    assert big["ne"] == lib.gsr_l1_ssim_exposure_num_partials(43, W) < lib.gsr_l1_ssim_exposure_num_partials(96, W)
    assert big["ep"].shape[0] == lib.gsr_l1_ssim_exposure_num_partials(96, W)
    assert torch.equal(big["ep"][:big["ne"]].view(i32), own["ep"].view(i32))
    assert torch.equal(big["partials"].view(i32), own["partials"].view(i32))
    assert torch.equal(big["M"].view(i32), own["M"].view(i32))
    for x, y in zip(big["gE"] + big["grads"], own["gE"] + own["grads"]):
        assert torch.equal(x.view(i32), y.view(i32))


def test_argument_checks_launch_nothing(device):
    lib = _lib()
    C, H, W = 3, 33, 36
    c = _case("noise", "full", C, H, W, 0, H)
    n4 = 4 * H * W  # room for a 4-channel call
    gI, gG = Guard(n4, f32, device), Guard(n4, u8, device)
    gI.t[:C * H * W] = c["img"].reshape(-1).to(device)
    gG.t[:C * H * W] = c["gt"].reshape(-1).to(device)
    gP, gD = Guard(2 * lib.gsr_l1_ssim_num_partials(4, H, W), f32, device), Guard(n4, f32, device)
    gM = [Guard(n4, f32, device) for _ in range(3)]
    gB, g1, gE = Guard(2, i32, device), Guard(1, f32, device), Guard(12, f32, device)
    gEP, gGE = Guard(12 * lib.gsr_l1_ssim_exposure_num_partials(H, W), f32, device), Guard(12, f32, device)
    gB.t.copy_(torch.tensor([0, H], dtype=i32))
    g1.t.fill_(1.0)
    gE.t.copy_(c["E"].reshape(-1))
    every = [gI, gG, gP, gD, gB, g1, gE, gEP, gGE] + gM
    for g in every:
        g.seal()
    s = _stream()
    m = [g.ptr for g in gM]

    def fwd(ch=C, expo=gE.ptr, partials=gP.ptr, band=None):
        return lib.gsr_l1_ssim_forward_exposure(ch, H, W, gI.ptr, H * W, gG.ptr, partials, m[0], m[1], m[2], band, expo, s)

    def bwd(ch=C, expo=gE.ptr, ep=gEP.ptr, ge=gGE.ptr, band=None):
        return lib.gsr_l1_ssim_backward_exposure(ch, H, W, gI.ptr, H * W, gG.ptr, m[0], m[1], m[2], g1.ptr, g1.ptr, 1.0,
                                                 1.0, gD.ptr, H * W, band, expo, ep, ge, s)

    for band in (None, gB.ptr):
        for ch in (1, 4):
            assert fwd(ch=ch, band=band) == GSR_EINVAL and bwd(ch=ch, band=band) == GSR_EINVAL
        assert fwd(expo=None, band=band) == GSR_EINVAL and fwd(partials=None, band=band) == GSR_EINVAL
        assert bwd(expo=None, band=band) == GSR_EINVAL
        assert bwd(ep=None, band=band) == GSR_EINVAL
        assert bwd(ge=None, band=band) == GSR_EINVAL
    torch.cuda.synchronize()
    for g in every:  # outputs still hold their poison, the guards are intact
        g.check("argument checks", whole=True)


@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 96, 100, 27, 70), (3, 33, 37, 0, 33)])
@pytest.mark.parametrize("dyn", [False, True])
def test_wrapper_against_fp64(device, C, H, W, y0, y1, dyn):
    from diff_gaussian_rasterization import fused_band_loss_exposure
    from oracle.loss_oracle import band_loss

    c = _case("noise", "full", C, H, W, y0, y1)
    rows, n, lam = y1 - y0, H * W * 3, 0.2
    ref = {}
    for dt in (f64, f32):
        x = c["xb"].to(dt).clone().requires_grad_(True)
        E = c["E"].to(dt).clone().requires_grad_(True)
        loss, Ll1, ssim = band_loss(_apply(x, E), c["gt"], H, W, lam)
        loss.backward()
        ref[dt] = (loss.detach(), Ll1.detach(), ssim.detach(), x.grad, E.grad)
    xi = c["img"].to(device).requires_grad_(True)
    Ei = c["E"].to(device).requires_grad_(True)
    if dyn:
        cap = rows + 7
        gt = torch.full((C, cap, W), 0xA5, dtype=u8, device=device)
        gt[:, :rows] = c["gt"].to(device)
        out = fused_band_loss_exposure(xi, Ei, gt, 0, 0, lam, n, band_rows=torch.tensor([y0, y1], dtype=i32, device=device))
    else:
        out = fused_band_loss_exposure(xi, Ei, c["gt"].to(device), y0, y1, lam, n)
    out[0].backward()
    tag = f"{C}x{H}x{W}[{y0}:{y1}] dyn={dyn}"
    for j, name in enumerate(("loss", "Ll1", "ssim")):
        want, w32 = float(ref[f64][j]), float(ref[f32][j])
        ratio = abs(float(out[j].detach()) - want) / max(abs(w32 - want), SUM_FLOOR * abs(want))
        print(f"RATIO exposure wrapper_{name} {tag} {ratio:.4g}")
        assert ratio <= K, (name, float(out[j].detach()), want)
    assert not out[1].requires_grad and not out[2].requires_grad
    g = xi.grad.cpu()
    ratio = assert_elem_close(g[:, y0:y1], ref[f64][3], ref[f32][3], K=K, what="wrapper image gradient")
    print(f"RATIO exposure wrapper_grad {tag} {ratio:.4g}")
    outside = torch.ones(H, dtype=torch.bool)
    outside[y0:y1] = False
    assert bool((g[:, outside] == 0).all()), "the gradient outside the band must be exactly zero"
    assert tuple(Ei.grad.shape) == (3, 4)
    ratio = assert_elem_close(Ei.grad.cpu(), ref[f64][4], ref[f32][4], K=K, what="wrapper exposure gradient")
    print(f"RATIO exposure wrapper_gE {tag} {ratio:.4g}")
