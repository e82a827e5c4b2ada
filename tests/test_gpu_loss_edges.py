"""csrc/loss.hip at its edges: the three derivative maps, the image gradient and the two sums of every launch variant,
element by element against the fp64 restatement (oracle/loss_oracle.py), with guard bands around every buffer, NaN rows
around every band, and the tolerance of helpers.assert_elem_close (K times the restatement's own fp32 error, never the
kernel's).  Observed ratios are printed (`RATIO ...`); EXPERIMENTS.md, "leaf-kernel element-wise noise", keeps the maxima."""
import math

import numpy as np
import pytest
import torch

import leaf_refs as R
from helpers import assert_elem_close
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

K = 8
SUM_FLOOR = 2e-5  # relative floor of the two sums: the bound of test_fused_loss_fwd_bwd_matches_torch_restatement
GSR_EINVAL = -1
f32, u8, i32 = torch.float32, torch.uint8, torch.int32

CASES = [(3, 1, 1, 0, 1), (3, 1, 37, 0, 1), (1, 5, 4, 0, 5), (3, 11, 11, 0, 11),       # degenerate sizes
         (3, 32, 32, 0, 32), (3, 64, 64, 0, 64),                                      # exact tiles
         (3, 33, 36, 0, 33), (4, 40, 68, 0, 40),                                      # VEC, partial tiles on both axes
         (3, 33, 37, 0, 33), (3, 83, 131, 0, 83)]                                     # scalar template
CASES += [(3, 96, W, y0, y1) for W in (100, 101) for y0, y1 in ((0, 1), (95, 96), (27, 70), (32, 64))]


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


_REFS = {}


def _case(family, C, H, W, y0, y1):
    """inputs and both references of one (family, case), computed once and never modified"""
    key = (family, C, H, W, y0, y1)
    if key not in _REFS:
        x, gt, ties = R.loss_inputs(family, C, H, W)
        img = torch.full_like(x, float("nan"))  # rows outside the band are NaN: zero padding has to BE zero padding
        img[:, y0:y1] = x[:, y0:y1]
        _REFS[key] = dict(img=img, gt=gt[:, y0:y1].contiguous(), ties=ties[:, y0:y1],
                          r64=R.loss_reference(x, gt, y0, y1, torch.float64),
                          r32=R.loss_reference(x, gt, y0, y1, torch.float32))
    return _REFS[key]


def run_loss(dev, img, gt_band, y0, y1, cap=None, coefs=R.COEFS, img_off=0, gt_off=0, img_extra=0, map_off=0,
             grad_extra=0, maps=True):
    """One forward (+ one backward per entry of `coefs`) through the C ABI on guarded buffers.  cap=None: the static entry
    points with the band pointer; cap >= rows: the *_band entry points at that capacity.  *_off: misalignment of a base
    (elements), *_extra: added to the channel stride.  -> dict(partials [nb_band, 2], M [3, C, rows, W] or None, grads)"""
    lib = _lib()
    C, H, W = img.shape
    rows = y1 - y0
    cap_rows = rows if cap is None else cap
    cs, gs = H * W + img_extra, H * W + grad_extra
    gI = Guard(C * cs, f32, dev, offset=img_off)
    gI.t.view(C, cs)[:, :H * W] = img.reshape(C, H * W).to(dev)
    gG = Guard(C * cap_rows * W, u8, dev, offset=gt_off)
    gG.t.view(C, cap_rows, W)[:, :rows] = gt_band.to(dev)
    nb_cap = lib.gsr_l1_ssim_num_partials(C, cap_rows, W)
    nb = lib.gsr_l1_ssim_num_partials(C, rows, W)
    assert nb == C * math.ceil(rows / 32) * math.ceil(W / 32) and nb_cap >= nb
    gP = Guard(2 * nb_cap, f32, dev)
    gM = [Guard(C * cap_rows * W, f32, dev, offset=map_off if i == 0 else 0) for i in range(3)]
    gB = Guard(2, i32, dev)
    gB.t.copy_(torch.tensor([y0, y1], dtype=i32))
    for g in [gI, gG, gP, gB] + gM:
        g.seal()
    mp = [g.ptr if maps else None for g in gM]
    if cap is None:
        rc = lib.gsr_l1_ssim_forward(C, rows, W, gI.ptr + 4 * y0 * W, cs, gG.ptr, gP.ptr, mp[0], mp[1], mp[2], _stream())
    else:
        rc = lib.gsr_l1_ssim_forward_band(C, cap_rows, W, gI.ptr, cs, gG.ptr, gP.ptr, mp[0], mp[1], mp[2], gB.ptr,
                                          _stream())
    assert rc == 0
    torch.cuda.synchronize()
    gI.check("image", whole=True), gG.check("ground truth", whole=True), gB.check("band", whole=True)
    gP.check("partials")
    partials = gP.t.view(nb_cap, 2).cpu()
    # every slot of the capacity is written: the band's own tiles hold sums, the slots above them exactly zero
    assert bool(torch.isfinite(partials).all()), "a partial sum was not written or is not finite"
    assert bool((partials[nb:] == 0).all()), "slots above the band's tile count must be exactly zero"
    in_band = torch.zeros(C, cap_rows, W, dtype=torch.bool, device=dev)
    in_band[:, :rows] = True
    M = None
    for i, g in enumerate(gM):
        g.check(f"map {i}")
        if not maps:
            g.check(f"map {i} (no-grad launch)", whole=True)
        else:
            g.untouched(~in_band.reshape(-1), f"map {i}, rows above the band")
    if maps:
        M = torch.stack([g.t.view(C, cap_rows, W)[:, :rows] for g in gM]).cpu()
        assert bool(torch.isfinite(M).all()), "a map element of the band was not written or is not finite"
    grads = []
    band_px = torch.zeros(C, gs, dtype=torch.bool, device=dev)
    band_px[:, y0 * W:y1 * W] = True
    for g_l1, g_ssim, s_l1, s_ssim in (coefs if maps else []):
        gD = Guard(C * gs, f32, dev)
        g1, g2 = Guard(1, f32, dev), Guard(1, f32, dev)
        g1.t.fill_(g_l1), g2.t.fill_(g_ssim)
        for g in [gD, g1, g2] + gM + [gP]:
            g.seal()
        if cap is None:
            rc = lib.gsr_l1_ssim_backward(C, rows, W, gI.ptr + 4 * y0 * W, cs, gG.ptr, gM[0].ptr, gM[1].ptr, gM[2].ptr,
                                          g1.ptr, g2.ptr, s_l1, s_ssim, gD.ptr + 4 * y0 * W, gs, _stream())
        else:
            rc = lib.gsr_l1_ssim_backward_band(C, cap_rows, W, gI.ptr, cs, gG.ptr, gM[0].ptr, gM[1].ptr, gM[2].ptr,
                                               g1.ptr, g2.ptr, s_l1, s_ssim, gD.ptr, gs, gB.ptr, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        for g in [gI, gG, gB, g1, g2, gP] + gM:
            g.check("backward input", whole=True)
        gD.check("gradient")
        gD.untouched(~band_px.reshape(-1), "gradient outside the band (the launch writes the band's rows only)")
        gr = gD.t.view(C, gs)[:, y0 * W:y1 * W].reshape(C, rows, W).cpu()
        assert bool(torch.isfinite(gr).all()), "a gradient element of the band was not written or is not finite"
        grads.append(gr)
    return dict(partials=partials[:nb].clone(), M=M, grads=grads)


def _check_sums(partials, r64, r32, tag):
    for j, name in enumerate(("l1", "ssim")):
        got = float(partials[:, j].double().sum())
        want, w32 = float(r64[name]), float(r32[name])
        unit = max(abs(w32 - want), SUM_FLOOR * abs(want))
        ratio = abs(got - want) / unit if unit > 0 else (0.0 if got == want else float("inf"))  # (an exact 0 sum)
        print(f"RATIO loss sum_{name} {tag} {ratio:.4g}")
        assert ratio <= K, f"{tag}: sum {name}: got {got!r}, fp64 {want!r}, error / unit = {ratio:.3g} > {K}"


def _check_against_fp64(res, c, tag):
    r64, r32 = c["r64"], c["r32"]
    _check_sums(res["partials"], r64, r32, tag)
    for i in range(3):
        ratio = assert_elem_close(res["M"][i], r64["M"][i], r32["M"][i], K=K, what=f"{tag} M{i + 1}")
        print(f"RATIO loss map{i + 1} {tag} {ratio:.4g}")
    for i, gr in enumerate(res["grads"]):
        ratio = assert_elem_close(gr, r64["grads"][i], r32["grads"][i], K=K, what=f"{tag} grad[{i}]")
        print(f"RATIO loss grad{i} {tag} {ratio:.4g}")


def _bit_equal(a, b, what):
    assert torch.equal(a["partials"].view(i32), b["partials"].view(i32)), f"{what}: partial sums differ in bits"
    if a["M"] is not None and b["M"] is not None:
        assert torch.equal(a["M"].view(i32), b["M"].view(i32)), f"{what}: maps differ in bits"
    for x, y in zip(a["grads"], b["grads"]):
        assert torch.equal(x.view(i32), y.view(i32)), f"{what}: gradients differ in bits"


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C,H,W,y0,y1", CASES)
def test_loss_every_element_against_fp64(device, family, C, H, W, y0, y1):
    """static launch with the band pointer, then the device-band launch at three capacities: each against fp64, and the
    device-band results bit-equal to the static ones (same tiles, same arithmetic)"""
    c = _case(family, C, H, W, y0, y1)
    rows = y1 - y0
    tag = f"{family} {C}x{H}x{W}[{y0}:{y1}]"
    static = run_loss(device, c["img"], c["gt"], y0, y1)
    _check_against_fp64(static, c, tag + " static")
    for cap in (rows, rows + 7, 32 * math.ceil(rows / 32) + 32):
        dyn = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap)
        _check_against_fp64(dyn, c, tag + f" cap{cap}")
        _bit_equal(dyn, static, tag + f" cap{cap} vs static")
    if family == "ties":  # sign(0) = 0: with g_ssim's term removed the gradient at a tie is exactly the SSIM part
        only_l1 = run_loss(device, c["img"], c["gt"], y0, y1, coefs=[(1.0, 0.0, 1.0, 1.0)])["grads"][0]
        assert bool((only_l1[c["ties"]] == 0).all()) and bool((only_l1[~c["ties"]].abs() == 1).all())


FALLBACKS = {"image_base_4B": dict(img_off=1), "gt_base_1B": dict(gt_off=1), "image_cstride_odd": dict(img_extra=1),
             "map_base_4B": dict(map_off=1), "grad_cstride_differs": dict(grad_extra=4)}


@pytest.mark.parametrize("which", sorted(FALLBACKS))
@pytest.mark.parametrize("cap", [None, 40])
def test_loss_alignment_fallback_is_bit_equal_to_the_aligned_launch(device, which, cap):
    """the launcher's scalar template (taken for a misaligned base or an odd channel stride) does the vector template's
    arithmetic in the same order: same bits, and the fp64 check again"""
    C, H, W, y0, y1 = 3, 33, 36, 0, 33
    c = _case("noise", C, H, W, y0, y1)
    aligned = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap)
    other = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap, **FALLBACKS[which])
    _check_against_fp64(other, c, f"noise fallback {which} cap{cap}")
    _bit_equal(other, aligned, which)


@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 33, 36, 0, 33), (3, 33, 37, 0, 33), (3, 96, 100, 27, 70)])
def test_loss_no_grad_launch_gives_the_same_partials(device, C, H, W, y0, y1):
    c = _case("noise", C, H, W, y0, y1)
    for cap in (None, y1 - y0 + 7):
        a = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap)
        b = run_loss(device, c["img"], c["gt"], y0, y1, cap=cap, maps=False)
        _bit_equal(a, b, "null maps")


@pytest.mark.parametrize("W", [100, 101])
def test_loss_capacity_above_the_band_publishes_zero_sums(device, W):
    """(run_loss asserts it for every launch; this is the case with two whole tile rows of slack)"""
    c = _case("noise", 3, 96, W, 27, 70)
    lib = _lib()
    res = run_loss(device, c["img"], c["gt"], 27, 70, cap=96)
    assert res["partials"].shape[0] == lib.gsr_l1_ssim_num_partials(3, 43, W) < lib.gsr_l1_ssim_num_partials(3, 96, W)


def _finalize_cases():
    out = []
    for nb in (1, 2, 255, 256, 257, 2047, 2048, 2049, 6120):
        out.append((nb, "mixed"))
    out.append((2049, "cancel"))
    return out


@pytest.mark.parametrize("nb,kind", _finalize_cases())
def test_loss_finalize_alone(device, nb, kind):
    """out[1], out[2] within 2^-23 |s| + 2^-52 sum|p| of the exact sums (double accumulation, one float rounding);
    out[0] within 4 * 2^-24 (|c_l1 s1| + |c_ssim s2| + |bias|)"""
    lib = _lib()
    g = torch.Generator().manual_seed(nb)
    p = (torch.rand(nb, 2, generator=g) - 0.3) * torch.tensor([900.0, 700.0])
    if kind == "cancel":  # pairs that cancel exactly, a small remainder on top
        half = nb // 2
        p[half:2 * half] = -p[:half]
        p[-1] = torch.tensor([3.0e-3, -2.0e-3])
    gP, gO = Guard(2 * nb, f32, device), Guard(3, f32, device)
    gP.t.copy_(p.reshape(-1))
    gP.seal(), gO.seal()
    c_l1, c_ssim, bias = float(np.float32(0.8 / 1234.0)), float(np.float32(-0.2 / 1234.0)), float(np.float32(0.2))
    assert lib.gsr_l1_ssim_finalize(nb, gP.ptr, c_l1, c_ssim, bias, 1.0, gO.ptr, _stream()) == 0
    torch.cuda.synchronize()
    gP.check("partials", whole=True), gO.check("out3")
    out = gO.t.cpu().double()
    s = [math.fsum(p[:, j].double().tolist()) for j in range(2)]
    sa = [float(p[:, j].double().abs().sum()) for j in range(2)]
    for j in range(2):
        assert abs(float(out[1 + j]) - s[j]) <= 2.0 ** -23 * abs(s[j]) + 2.0 ** -52 * sa[j], (nb, kind, j, out, s)
    want = c_l1 * s[0] + c_ssim * s[1] + bias
    assert abs(float(out[0]) - want) <= 4 * 2.0 ** -24 * (abs(c_l1 * s[0]) + abs(c_ssim * s[1]) + abs(bias))


def test_loss_argument_checks_launch_nothing(device):
    lib = _lib()
    C, H, W = 3, 33, 36
    c = _case("noise", C, H, W, 0, H)
    gI, gG = Guard(C * H * W, f32, device), Guard(C * H * W, u8, device)
    gI.t.copy_(c["img"].reshape(-1)), gG.t.copy_(c["gt"].reshape(-1))
    nb = lib.gsr_l1_ssim_num_partials(C, H, W)
    gP, gD = Guard(2 * nb, f32, device), Guard(C * H * W, f32, device)
    gM = [Guard(C * H * W, f32, device) for _ in range(3)]
    gB, g1 = Guard(2, i32, device), Guard(1, f32, device)
    gB.t.copy_(torch.tensor([0, H], dtype=i32))
    g1.t.fill_(1.0)
    every = [gI, gG, gP, gD, gB, g1] + gM
    for g in every:
        g.seal()
    s = _stream()
    m = [g.ptr for g in gM]
    for nulls in ([0], [1], [2], [0, 1], [0, 2], [1, 2]):  # one or two of the three map pointers null
        q = [None if i in nulls else m[i] for i in range(3)]
        assert lib.gsr_l1_ssim_forward(C, H, W, gI.ptr, H * W, gG.ptr, gP.ptr, q[0], q[1], q[2], s) == GSR_EINVAL
        assert lib.gsr_l1_ssim_forward_band(C, H, W, gI.ptr, H * W, gG.ptr, gP.ptr, q[0], q[1], q[2], gB.ptr,
                                            s) == GSR_EINVAL
        assert lib.gsr_l1_ssim_backward(C, H, W, gI.ptr, H * W, gG.ptr, q[0], q[1], q[2], g1.ptr, g1.ptr, 1.0, 1.0,
                                        gD.ptr, H * W, s) == GSR_EINVAL
    # capacity 0 with a band; a null band at the _band entry points
    assert lib.gsr_l1_ssim_forward_band(C, 0, W, gI.ptr, H * W, gG.ptr, gP.ptr, m[0], m[1], m[2], gB.ptr, s) == GSR_EINVAL
    assert lib.gsr_l1_ssim_backward_band(C, 0, W, gI.ptr, H * W, gG.ptr, m[0], m[1], m[2], g1.ptr, g1.ptr, 1.0, 1.0,
                                         gD.ptr, H * W, gB.ptr, s) == GSR_EINVAL
    assert lib.gsr_l1_ssim_forward_band(C, H, W, gI.ptr, H * W, gG.ptr, gP.ptr, m[0], m[1], m[2], None, s) == GSR_EINVAL
    assert lib.gsr_l1_ssim_backward_band(C, H, W, gI.ptr, H * W, gG.ptr, m[0], m[1], m[2], g1.ptr, g1.ptr, 1.0, 1.0,
                                         gD.ptr, H * W, None, s) == GSR_EINVAL
    # rows = 0: success, nothing written
    assert lib.gsr_l1_ssim_forward(C, 0, W, gI.ptr, H * W, gG.ptr, gP.ptr, m[0], m[1], m[2], s) == 0
    assert lib.gsr_l1_ssim_backward(C, 0, W, gI.ptr, H * W, gG.ptr, m[0], m[1], m[2], g1.ptr, g1.ptr, 1.0, 1.0, gD.ptr,
                                    H * W, s) == 0
    assert lib.gsr_l1_ssim_num_partials(C, 0, W) == 0
    torch.cuda.synchronize()
    for g in every:
        g.check("argument checks", whole=True)


@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 96, 100, 27, 70), (3, 33, 37, 0, 33)])
@pytest.mark.parametrize("dyn", [False, True])
def test_fused_band_loss_wrapper_against_fp64(device, C, H, W, y0, y1, dyn):
    from diff_gaussian_rasterization import fused_band_loss
    from oracle.loss_oracle import band_loss

    c = _case("noise", C, H, W, y0, y1)
    rows, n, lam = y1 - y0, H * W * 3, 0.2
    ref = {}
    for dt in (torch.float64, torch.float32):
        x = c["img"][:, y0:y1].to(dt).clone().requires_grad_(True)
        loss, Ll1, ssim = band_loss(x, c["gt"], H, W, lam)
        loss.backward()
        ref[dt] = (loss.detach(), Ll1.detach(), ssim.detach(), x.grad)
    xi = c["img"].to(device).requires_grad_(True)
    if dyn:
        cap = rows + 7
        gt = torch.full((C, cap, W), 0xA5, dtype=u8, device=device)
        gt[:, :rows] = c["gt"].to(device)
        out = fused_band_loss(xi, gt, 0, 0, lam, n, band_rows=torch.tensor([y0, y1], dtype=i32, device=device))
    else:
        out = fused_band_loss(xi, c["gt"].to(device), y0, y1, lam, n)
    out[0].backward()
    for j, name in enumerate(("loss", "Ll1", "ssim")):
        want, w32 = float(ref[torch.float64][j]), float(ref[torch.float32][j])
        ratio = abs(float(out[j].detach()) - want) / max(abs(w32 - want), SUM_FLOOR * abs(want))
        print(f"RATIO loss wrapper_{name} {C}x{H}x{W}[{y0}:{y1}] dyn={dyn} {ratio:.4g}")
        assert ratio <= K, (name, float(out[j].detach()), want)
    g = xi.grad.cpu()
    ratio = assert_elem_close(g[:, y0:y1], ref[torch.float64][3], ref[torch.float32][3], K=K, what="wrapper grad")
    print(f"RATIO loss wrapper_grad {C}x{H}x{W}[{y0}:{y1}] dyn={dyn} {ratio:.4g}")
    outside = torch.ones(H, dtype=torch.bool)
    outside[y0:y1] = False
    assert bool((g[:, outside] == 0).all()), "the gradient outside the band must be exactly zero"
