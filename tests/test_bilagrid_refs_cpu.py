"""The restatement of the bilateral-grid slice (tests/bilagrid_refs.py) pinned on torch's own grid_sample, and the input
conditions the GPU tests rest on, verified before a GPU is involved.  Also the host-only surface of the feature: the
model's shape, the two setters' mutual refusal and the pure-host entry points of the library."""
import pytest
import torch

import bilagrid_refs as B

f32, f64 = torch.float32, torch.float64
NAMES = [c[0] for c in B.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_agrees_with_grid_sample(name):
    c = B.case(name)
    a = c["r64"]
    b = B.slice_with_grads(B.slice_gridsample, c["image"], c["grid"], c["gout"], f64, c["y0"], c["y1"])
    for what, x, y in zip(("value", "grad_image", "grad_grid"), a, b):
        err = float((x - y).abs().max())
        assert err <= 1e-12, f"{name} {what}: restatement and grid_sample differ by {err:.3g}"
    assert bool(a[2].any()) and bool(a[1].any())


@pytest.mark.parametrize("name", NAMES)
def test_input_conditions(name):
    """colours in [-0.25, 1.25] with both clamps live; pz of every unclamped pixel at least 2^-10 from an integer, in
    fp32 and in fp64, on the same set of pixels; the dedicated pixels have luminance exactly 0 and exactly 1 in both"""
    c = B.case(name)
    img, (gw, gh, gl) = c["image"], c["sizes"]
    assert float(img.min()) >= -0.25 and float(img.max()) <= 1.25
    lum32, lum64 = B.luminance(img), B.luminance(img.double())
    live32, live64 = (lum32 > 0) & (lum32 < 1), (lum64 > 0) & (lum64 < 1)
    assert torch.equal(live32, live64)
    for lum, live in ((lum32, live32), (lum64, live64)):
        pz = (lum.double() * (gl - 1))[live]
        assert bool(((pz - pz.round()).abs() >= B.MARGIN).all())
    black, white = B.dedicated_pixels(c["W"], c["H"])
    for lum in (lum32, lum64):
        flat = lum.reshape(-1)
        assert bool((flat[black] == 0).all()) and bool((flat[white] == 1).all())
    if c["W"] * c["H"] >= 16:
        assert bool((lum64 < 0).any()) and bool((lum64 > 1).any()) and bool(live64.any())
        y0, y1 = c["y0"], c["y1"]
        rows = torch.tensor(black + white) // c["W"]
        assert bool(((rows >= y0) & (rows < y1)).any()), "no dedicated pixel inside the band"


def test_guide_term_is_cut_on_clamped_pixels():
    """the image gradient of a clamped pixel (luminance <= 0 or >= 1, the exact ends included) is A_M^T g' alone"""
    c = B.case("33x17")
    img, grid, gout = c["image"].double(), c["grid"].double(), c["gout"].double()
    _, gx, _ = c["r64"]
    lum = B.luminance(img)
    dead = ~((lum > 0) & (lum < 1))
    # A_M of every pixel, rebuilt here from the lattice with the guide held at this image's luminance
    _, L, GH, GW = grid.shape
    ix, tx = B._axis(c["W"], GW, f64)
    iy, ty = B._axis(c["H"], GH, f64)
    pz = lum.clamp(0, 1) * (L - 1)
    iz = torch.floor(pz).clamp(max=L - 2)
    tz, iz = pz - iz, iz.long()

    def node(dz, dy, dx):
        return grid[:, iz + dz, (iy + dy)[:, None], (ix + dx)[None, :]]

    lo = B._lerp(B._lerp(node(0, 0, 0), node(0, 0, 1), tx[None]), B._lerp(node(0, 1, 0), node(0, 1, 1), tx[None]), ty[:, None])
    hi = B._lerp(B._lerp(node(1, 0, 0), node(1, 0, 1), tx[None]), B._lerp(node(1, 1, 0), node(1, 1, 1), tx[None]), ty[:, None])
    M = B._lerp(lo, hi, tz).reshape(3, 4, c["H"], c["W"])
    direct = torch.einsum("ckhw,chw->khw", M[:, :3], gout)
    assert bool(dead.any()) and float((gx - direct)[:, dead].abs().max()) <= 1e-12
    assert float((gx - direct)[:, ~dead].abs().max()) > 1e-3  # (and elsewhere the guide term is there)


@pytest.mark.parametrize("sizes", [B.DEFAULT, (3, 5, 4), (2, 2, 2)])
def test_identity_grid_returns_the_image(sizes):
    img = B.make_image(33, 17, sizes[2], 0)
    for dt in (f32, f64):
        out = B.slice_reference(img, B.identity_grid(sizes), dt)
        assert torch.equal(out, img.to(dt))
    out, gx, _ = B.slice_with_grads(B.slice_reference, img, B.identity_grid(sizes), B.make_gout(33, 17, 0), f64)
    assert torch.equal(gx, B.make_gout(33, 17, 0).double())


def test_band_rows_are_rows_of_the_whole_image():
    whole, band = B.case("33x17"), B.case("33x17-band")
    assert torch.equal(whole["image"], band["image"]) and torch.equal(whole["grid"], band["grid"])
    y0, y1 = band["y0"], band["y1"]
    assert (y0, y1) == (5, 12)
    assert torch.equal(band["r64"][0], whole["r64"][0][:, y0:y1])
    assert float((band["r64"][1] - whole["r64"][1][:, y0:y1]).abs().max()) <= 1e-13


@pytest.mark.parametrize("N,sizes", [(3, (3, 5, 4)), (2, B.DEFAULT)])
def test_tv_value_and_gradient_against_the_closed_form(N, sizes):
    """tv_reference by autograd against the stated closed form: dT/dG = sum_axis 2 / (N cnt_axis) ((G - prev) - (next - G))"""
    gw, gh, gl = sizes
    g = torch.Generator().manual_seed(5)
    G = torch.randn(N, 12, gl, gh, gw, generator=g, dtype=f64).requires_grad_(True)
    T = B.tv_reference(G)
    (grad,) = torch.autograd.grad(T, G)
    want_T, want = 0.0, torch.zeros_like(G)
    for dim, size in ((2, gl), (3, gh), (4, gw)):
        d = (G.narrow(dim, 1, size - 1) - G.narrow(dim, 0, size - 1)).detach()
        cnt = d[0].numel()
        assert cnt == 12 * gl * gh * gw // size * (size - 1)
        want_T += float((d * d).sum()) / cnt / N
        want.narrow(dim, 1, size - 1).add_(2.0 / (N * cnt) * d)
        want.narrow(dim, 0, size - 1).sub_(2.0 / (N * cnt) * d)
    assert abs(float(T.detach()) - want_T) <= 1e-12 * want_T
    assert float((grad - want).abs().max()) <= 1e-14


def test_apply_bilagrid_agrees_with_the_restatement():
    from bilagrid import apply_bilagrid

    c = B.case("67x35-g354")
    got = apply_bilagrid(c["image"].double(), c["grid"].double())
    assert float((got - c["r64"][0]).abs().max()) <= 1e-12


def test_model_shape_and_schedule_on_the_host():
    from bilagrid import BilateralGridModel

    m = BilateralGridModel(3, grid=(3, 5, 4), device="cpu", lr_init=2e-3, lr_final=2e-5, max_steps=100)
    assert tuple(m.grids.shape) == (3, 12, 4, 5, 3) and m.num_cameras == 3 and m.steps == 0
    assert torch.equal(m.grids.detach()[1], B.identity_grid((3, 5, 4)))
    cam = type("C", (), {"uid": 2})()
    assert m.of(cam).shape == (12, 4, 5, 3) and m.of(cam).data_ptr() == m.grids[2].data_ptr()
    with pytest.raises(IndexError):
        m.of(type("C", (), {"uid": 3})())
    assert m.lr_at(0) == 2e-3 and abs(m.lr_at(100) - 2e-5) <= 1e-18 and m.lr_at(1000) == m.lr_at(100)
    m.step()  # no gradient: nothing happens
    assert m.steps == 0
    m.grids.grad = torch.ones_like(m.grids)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.step()
    other = BilateralGridModel(3, grid=(3, 5, 4), device="cpu")
    state = m.state_dict()
    state["steps"] = 7
    other.load_state_dict(state)
    assert other.steps == 7 and torch.equal(other.grids.detach(), m.grids.detach()) and other.grids.grad is None
    with pytest.raises(ValueError):
        BilateralGridModel(3, grid=(16, 16, 8), device="cpu").load_state_dict(state)
    for bad in ((1, 16, 8), (16, 65, 8), (16, 16, 17)):
        with pytest.raises(ValueError):
            BilateralGridModel(1, grid=bad, device="cpu")


def test_exposure_and_grid_refuse_each_other():
    from bilagrid import BilateralGridModel
    from exposure import ExposureModel
    from gaussian_renderer import loss_distribution as ld

    grid, expo = BilateralGridModel(1, grid=(2, 2, 2), device="cpu"), ExposureModel(1, device="cpu")
    assert ld.get_bilateral_grid() is None
    try:
        ld.set_exposure_model(expo)
        with pytest.raises(ValueError, match="set_exposure_model.*set_bilateral_grid"):
            ld.set_bilateral_grid(grid)
        assert ld.get_bilateral_grid() is None
        ld.set_exposure_model(None)
        ld.set_bilateral_grid(grid)
        assert ld.get_bilateral_grid() is grid
        with pytest.raises(ValueError, match="set_exposure_model.*set_bilateral_grid"):
            ld.set_exposure_model(expo)
        assert ld.get_exposure_model() is None
    finally:
        ld.set_bilateral_grid(None)
        ld.set_exposure_model(None)


def test_host_entry_points_and_argument_checks():
    """everything here returns before any device work: dummy integers stand for device pointers"""
    from diff_gaussian_rasterization import _lib

    lib, d = _lib.lib, 0x1000
    # 1080p under the default grid: 15 x 15 cells of 128 x 72 pixels, 4 x 3 pieces each, 4 * 8 * 12 sums per piece
    assert lib.gsr_bilagrid_num_partials(1920, 1080, 16, 16, 8) == 225 * 12 * 384
    assert lib.gsr_bilagrid_num_partials(1, 1, 16, 16, 8) == 225 * 384
    assert lib.gsr_bilagrid_num_partials(67, 35, 2, 2, 2) == 3 * 2 * 96
    assert lib.gsr_bilagrid_num_partials(0, 35, 2, 2, 2) == 0 and lib.gsr_bilagrid_num_partials(67, 35, 1, 2, 2) == 0
    assert lib.gsr_bilagrid_tv_num_partials(2, 16, 16, 8) == 2 * 12 * 8 * 16 * 16 // 256

    def fwd(w=67, h=35, y0=0, y1=35, img=d, grid=d, sizes=(3, 5, 4), out=d):
        return lib.gsr_bilagrid_slice_forward(w, h, y0, y1, img, w * h, grid, *sizes, out, w * h, None)

    def bwd(w=67, h=35, y0=0, y1=35, img=d, grid=d, sizes=(3, 5, 4), gout=d, gimg=d, part=d, gg=d):
        return lib.gsr_bilagrid_slice_backward(w, h, y0, y1, img, w * h, grid, *sizes, gout, w * h, gimg, w * h, part, gg,
                                               None)

    for f in (fwd, bwd):
        assert f(w=0) == -1 and f(h=0) == -1 and f(y0=-1) == -1 and f(y1=36) == -1 and f(y0=9, y1=8) == -1
        assert f(img=None) == -1 and f(grid=None) == -1
        for sizes in ((1, 5, 4), (65, 5, 4), (3, 1, 4), (3, 65, 4), (3, 5, 1), (3, 5, 17)):
            assert f(sizes=sizes) == -1
    assert fwd(out=None) == -1
    assert bwd(gout=None) == -1 and bwd(gimg=None) == -1 and bwd(part=None) == -1 and bwd(gg=None) == -1
    assert fwd(y0=7, y1=7) == 0  # an empty band: nothing to do
    assert lib.gsr_bilagrid_tv(0, 3, 5, 4, d, 1.0, d, None, None, None) == -1
    assert lib.gsr_bilagrid_tv(1, 3, 5, 4, None, 1.0, d, None, None, None) == -1
    assert lib.gsr_bilagrid_tv(1, 3, 5, 4, d, 1.0, None, None, None, None) == -1
    assert lib.gsr_bilagrid_tv(1, 3, 5, 4, d, 1.0, d, d, None, None) == -1
    assert lib.gsr_bilagrid_tv(1, 3, 5, 17, d, 1.0, d, None, None, None) == -1
