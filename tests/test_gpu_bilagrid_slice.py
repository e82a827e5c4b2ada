"""The bilateral-grid slice kernels of csrc/bilagrid.hip (include/gsraster.h, N1g) through the C ABI on guarded buffers:
every element of x', of the image gradient and of the lattice gradient against the fp64 restatement
(tests/bilagrid_refs.py), tolerance helpers.assert_elem_close -- K times the restatement's own fp32 error, never the
kernel's.  Observed ratios are printed (`RATIO ...`); EXPERIMENTS.md keeps the maxima.  Then the exact properties: an
identity grid, the cut of the guide term, reproducible bits, bands that partition an image, nodes out of a band's reach,
refused arguments."""
import pytest
import torch

import bilagrid_refs as B
from helpers import assert_elem_close
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

K = 8
GSR_EINVAL = -1
f32, i32 = torch.float32, torch.int32
NAMES = [c[0] for c in B.CASES]


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def run_slice(dev, image, grid, gout, y0, y1):
    """one forward and one backward on guarded buffers; rows outside the band are NaN in the inputs and must stay
    untouched in the outputs -> (x', grad_image: the band's rows [3,rows,W]; grad_grid [12,L,GH,GW]), on the host"""
    lib = _lib()
    _, H, W = image.shape
    _, gl, gh, gw = grid.shape
    n = 3 * H * W
    band = torch.zeros(3, H, W, dtype=torch.bool)
    band[:, y0:y1] = True
    nan = torch.full_like(image, float("nan"))
    gI, gG, gO, gD, gX = (Guard(n, f32, dev), Guard(grid.numel(), f32, dev), Guard(n, f32, dev), Guard(n, f32, dev),
                          Guard(n, f32, dev))
    gI.t.copy_(torch.where(band, image, nan).reshape(-1))
    gD.t.copy_(torch.where(band, gout, nan).reshape(-1))
    gG.t.copy_(grid.reshape(-1))
    npart = lib.gsr_bilagrid_num_partials(W, H, gw, gh, gl)
    assert npart > 0 and npart % (4 * gl * 12) == 0
    gP, gGG = Guard(npart, f32, dev), Guard(grid.numel(), f32, dev)
    every = [gI, gG, gO, gD, gX, gP, gGG]
    for g in every:
        g.seal()
    rc = lib.gsr_bilagrid_slice_forward(W, H, y0, y1, gI.ptr, H * W, gG.ptr, gw, gh, gl, gO.ptr, H * W, _stream())
    assert rc == 0
    rc = lib.gsr_bilagrid_slice_backward(W, H, y0, y1, gI.ptr, H * W, gG.ptr, gw, gh, gl, gD.ptr, H * W, gX.ptr, H * W,
                                         gP.ptr, gGG.ptr, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for g in (gI, gG, gD):
        g.check("input", whole=True)
    outside = (~band).reshape(-1).to(dev)
    for g, what in ((gO, "x'"), (gX, "grad_image")):
        g.check(what)
        g.untouched(outside, f"{what}, rows outside the band")
    gP.check("partials"), gGG.check("grad_grid")
    out = gO.t.view(3, H, W)[:, y0:y1].cpu()
    gx = gX.t.view(3, H, W)[:, y0:y1].cpu()
    gg = gGG.t.view(12, gl, gh, gw).cpu()
    checked = [(out, "x'"), (gx, "grad_image"), (gg, "grad_grid")]
    if y1 > y0:  # (an empty band launches nothing: the scratch rows stay as they were)
        checked.append((gP.t.cpu(), "partials"))
    for t, what in checked:
        assert bool(torch.isfinite(t).all()), f"{what}: an element was not written or is not finite"
    return out, gx, gg


_RUNS = {}


def _run(dev, name):
    if name not in _RUNS:
        c = B.case(name)
        _RUNS[name] = run_slice(dev, c["image"], c["grid"], c["gout"], c["y0"], c["y1"])
    return _RUNS[name]


@pytest.mark.parametrize("name", NAMES)
def test_every_element_against_fp64(device, name):
    c = B.case(name)
    got = _run(device, name)
    for what, g, r64, r32 in zip(("forward", "grad_image", "grad_grid"), got, c["r64"], c["r32"]):
        ratio = assert_elem_close(g, r64, r32, K=K, what=f"{name} {what}")
        print(f"RATIO bilagrid {what} {name} {ratio:.4g}")


def test_band_equals_the_rows_of_the_whole_image(device):
    """y is the row of the full image: the band run's rows have the bits of the whole-image run's"""
    whole, band = _run(device, "33x17"), _run(device, "33x17-band")
    assert torch.equal(band[0].view(i32), whole[0][:, 5:12].contiguous().view(i32))
    assert torch.equal(band[1].view(i32), whole[1][:, 5:12].contiguous().view(i32))


@pytest.mark.parametrize("name", ["33x17", "96x64", "67x35-g5416"])
def test_identity_grid_hands_image_and_gradient_through(device, name):
    c = B.case(name)
    out, gx, gg = run_slice(device, c["image"], B.identity_grid(c["sizes"]), c["gout"], c["y0"], c["y1"])
    assert torch.equal(out, c["image"]) and torch.equal(gx, c["gout"])
    assert bool(gg.any())


@pytest.mark.parametrize("name", ["33x17", "67x35-g354"])
def test_guide_term_is_exactly_zero_on_clamped_pixels(device, name):
    """A clamped pixel (luminance <= 0 or >= 1) samples M at the end of the guide axis whatever its colour, and its
    gradient is A_M^T g' alone.  Second run: every clamped pixel's colour moved further out (the dedicated pixels leave
    the exact ends), which changes g' (x) [c, 1] -- the input of the guide term -- and nothing else: the gradients of
    those pixels keep their bits."""
    c = B.case(name)
    img = c["image"]
    lum = B.luminance(img)
    low, high = lum <= 0, lum >= 1
    black, white = B.dedicated_pixels(c["W"], c["H"])
    assert bool(low.reshape(-1)[black].all()) and bool(high.reshape(-1)[white].all())
    moved = torch.where(low, img - 0.03125, torch.where(high, img + 0.03125, img))
    lum2 = B.luminance(moved)
    assert bool((lum2[low] < 0).all()) and bool((lum2[high] > 1).all())
    _, gx, _ = _run(device, name)
    _, gx2, _ = run_slice(device, moved, c["grid"], c["gout"], c["y0"], c["y1"])
    dead = (low | high).expand(3, -1, -1)
    assert torch.equal(gx[dead].view(i32), gx2[dead].view(i32))
    # (that the value they keep is A_M^T g' is the element-wise comparison above: the restatement cuts the term, and
    # tests/test_bilagrid_refs_cpu.py shows that its gradient there is A_M^T g')


@pytest.mark.parametrize("name", ["96x64", "67x35-g5416", "33x17-band"])
def test_two_runs_give_equal_bits(device, name):
    c = B.case(name)
    a = _run(device, name)
    b = run_slice(device, c["image"], c["grid"], c["gout"], c["y0"], c["y1"])
    for x, y in zip(a, b):
        assert torch.equal(x.view(i32), y.view(i32))


@pytest.mark.parametrize("name,cut", [("33x17", 5), ("96x64", 37)])
def test_two_bands_sum_to_the_whole_image(device, name, cut):
    c = B.case(name)
    H = c["H"]
    top = run_slice(device, c["image"], c["grid"], c["gout"], 0, cut)
    bottom = run_slice(device, c["image"], c["grid"], c["gout"], cut, H)
    ratio = assert_elem_close(top[2].double() + bottom[2].double(), c["r64"][2], c["r32"][2], K=K,
                              what=f"{name} grad_grid of two bands")
    print(f"RATIO bilagrid grad_grid_two_bands {name} {ratio:.4g}")
    whole = _run(device, name)
    assert torch.equal(torch.cat([top[1], bottom[1]], dim=1).view(i32), whole[1].view(i32))


def test_nodes_out_of_a_thin_bands_reach_are_exactly_zero(device):
    c = B.case("96x64")
    gw, gh, gl = c["sizes"]
    y0, y1 = 20, 23
    _, _, gg = run_slice(device, c["image"], c["grid"], c["gout"], y0, y1)
    iy, _ = B._axis(c["H"], gh, torch.float32, y0, y1)
    lo, hi = int(iy.min()), int(iy.max()) + 1  # the node rows the band's pixels touch
    assert 0 < lo and hi < gh - 1
    assert bool(gg[:, :, lo:hi + 1].any())
    assert bool((gg[:, :, :lo] == 0).all()) and bool((gg[:, :, hi + 1:] == 0).all())
    # an empty band: nothing written but the lattice gradient, which is cleared
    out, gx, gg = run_slice(device, c["image"], c["grid"], c["gout"], 7, 7)
    assert out.numel() == 0 and gx.numel() == 0 and bool((gg == 0).all())


def test_refused_arguments_launch_nothing(device):
    lib = _lib()
    c = B.case("67x35-g354")
    W, H, (gw, gh, gl) = c["W"], c["H"], c["sizes"]
    n = 3 * H * W
    gI, gG, gO, gP = Guard(n, f32, device), Guard(c["grid"].numel(), f32, device), Guard(n, f32, device), \
        Guard(lib.gsr_bilagrid_num_partials(W, H, gw, gh, gl), f32, device)
    gI.t.copy_(c["image"].reshape(-1))
    gG.t.copy_(c["grid"].reshape(-1))
    gGG = Guard(c["grid"].numel(), f32, device)
    every = [gI, gG, gO, gP, gGG]
    for g in every:
        g.seal()
    s = _stream()

    def fwd(w=W, h=H, y0=0, y1=H, img=gI.ptr, grid=gG.ptr, sizes=(gw, gh, gl), out=gO.ptr):
        return lib.gsr_bilagrid_slice_forward(w, h, y0, y1, img, W * H, grid, *sizes, out, W * H, s)

    def bwd(w=W, h=H, y0=0, y1=H, img=gI.ptr, grid=gG.ptr, sizes=(gw, gh, gl), gout=gI.ptr, gimg=gO.ptr, part=gP.ptr,
            gg=gGG.ptr):
        return lib.gsr_bilagrid_slice_backward(w, h, y0, y1, img, W * H, grid, *sizes, gout, W * H, gimg, W * H, part, gg, s)

    for f in (fwd, bwd):
        for kw in (dict(w=0), dict(w=-3), dict(h=0), dict(y0=-1), dict(y1=H + 1), dict(y0=9, y1=8), dict(img=None),
                   dict(grid=None), dict(sizes=(1, gh, gl)), dict(sizes=(65, gh, gl)), dict(sizes=(gw, 1, gl)),
                   dict(sizes=(gw, 65, gl)), dict(sizes=(gw, gh, 1)), dict(sizes=(gw, gh, 17))):
            assert f(**kw) == GSR_EINVAL, kw
    assert fwd(out=None) == GSR_EINVAL
    for kw in (dict(gout=None), dict(gimg=None), dict(part=None), dict(gg=None)):
        assert bwd(**kw) == GSR_EINVAL, kw
    torch.cuda.synchronize()
    for g in every:
        g.check("refused arguments", whole=True)


@pytest.mark.parametrize("name", ["33x17-band", "67x35-g354"])
def test_wrapper_against_fp64(device, name):
    from diff_gaussian_rasterization import bilagrid_slice

    c = B.case(name)
    y0, y1, H = c["y0"], c["y1"], c["H"]
    x = c["image"].to(device).requires_grad_(True)
    g = c["grid"].to(device).requires_grad_(True)
    out = bilagrid_slice(x, g, y0, y1, H)
    (out * c["gout"].to(device)).sum().backward()
    outside = torch.ones(H, dtype=torch.bool)
    outside[y0:y1] = False
    assert bool((out.detach().cpu()[:, outside] == 0).all()) and bool((x.grad.cpu()[:, outside] == 0).all())
    for what, got, r64, r32 in zip(("forward", "grad_image", "grad_grid"),
                                   (out.detach().cpu()[:, y0:y1], x.grad.cpu()[:, y0:y1], g.grad.cpu()), c["r64"], c["r32"]):
        ratio = assert_elem_close(got, r64, r32, K=K, what=f"wrapper {name} {what}")
        print(f"RATIO bilagrid wrapper_{what} {name} {ratio:.4g}")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilagrid_slice(c["image"], c["grid"], y0, y1, H)
