"""set_antialiasing(True) through the operator surface: the rendered image and the gradients of the five inputs against
the float64 restatement (tests/antialias_refs.py -> oracle/torch_oracle.render; the switch has no reference call site),
the fused K11 + Adam step against the unfused one with the setting flipped between backward and step, a captured
iteration, and the refusal of camera gradients.  Every test leaves the setting (and the library) off."""
import pytest
import torch

import antialias_refs as A
import projection_refs as R
import synthetic_scene as S
from helpers import KEYS, elem_excess, rel_err, settings_from
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # the bar of tests/test_gpu_parity.py::test_full_chain_matches_c_oracle


@pytest.fixture
def aa():
    """-> the operator module, anti-aliasing on; off again afterwards, in the library too"""
    import diff_gaussian_rasterization as dgr

    dgr.set_antialiasing(True)
    try:
        yield dgr
    finally:
        dgr.set_antialiasing(False)
        dgr._lib_antialiasing(False)


def _scene(W, H):
    """300 rows: half `aaclamp` (far below a pixel, q on both sides of the clamp), half `plain`"""
    gen = torch.Generator().manual_seed(41)
    a, b = A._draw_aaclamp(gen, 150, W, H), R._base(gen, 150, W, H)
    g = {k: torch.cat([a[k], b[k]]).float().contiguous() for k in KEYS}
    g["opacities"] = 0.5 + 0.5 * g["opacities"]  # (the compensated sub-pixel rows are to stay above alpha = 1/255)
    return g


def _oracle(g, cam, bg, mask, wgt, deg):
    """float64: K1 with the compensated opacity, the composite, the weighted sum, autograd to the five inputs"""
    W, H = cam.image_width, cam.image_height
    leaves = [g[k].double().clone().requires_grad_() for k in KEYS]
    tx, ty = R.tanfov(cam)
    m2, rgb, co, radii, depths = O.preprocess(*leaves, viewmatrix=cam.world_view_transform,
                                              projmatrix=cam.full_proj_transform, campos=cam.camera_center, W=W, H=H,
                                              tanfovx=tx, tanfovy=ty, sh_degree=deg)
    ix = (radii > 0).nonzero().squeeze(1)
    rho = A.Rho.apply(*A.cov2d_abc(leaves[0][ix], leaves[1][ix], leaves[2][ix], cam, W, H))
    factor = torch.ones(radii.shape[0], dtype=torch.float64).index_copy(0, ix, rho)
    co = torch.cat([co[:, :3], co[:, 3:] * factor[:, None]], dim=1)
    image = O.render(m2, co, rgb, depths, radii, mask, bg=bg.double(), W=W, H=H)[0]
    grads = torch.autograd.grad((image * wgt.double()).sum(), leaves)
    return image.detach(), dict(zip(KEYS, grads)), float(((factor < 1) & (factor <= 0.005 * (1 + 1e-9))).sum())


def test_render_and_gradients_match_the_float64_restatement(device, aa):
    W, H, deg = 96, 64, 3
    g = _scene(W, H)
    cam = S.orbit_cameras(4, W, H)[0]
    bg = torch.tensor([0.1, 0.2, 0.3])
    mask = torch.ones((H + 15) // 16, (W + 15) // 16, dtype=torch.bool)
    wgt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(11))
    want_img, want, n_clamped = _oracle(g, cam, bg, mask, wgt, deg)
    assert n_clamped >= 20, "the scene has no rows on the clamp"

    def run():
        rast = aa.GaussianRasterizer(settings_from(cam, bg, sh_degree=deg))
        gg = {k: v.to(device).requires_grad_(True) for k, v in g.items()}
        ca = {"stats_collector": {}}
        m2, rgb, co, radii, depths = rast.preprocess_gaussians(*[gg[k] for k in KEYS], ca)
        img = rast.render_gaussians(means2D=m2, conic_opacity=co, rgb=rgb, depths=depths, radii=radii,
                                    compute_locally=mask.to(device), extended_compute_locally=None, cuda_args=ca)[0]
        (img * wgt.to(device)).sum().backward()
        return img.detach(), gg

    img, gg = run()
    print(f"[aa render] image rel {rel_err(img, want_img):.2e}")
    assert rel_err(img, want_img) < RTOL
    for k in KEYS:
        e, x = rel_err(gg[k].grad, want[k]), elem_excess(gg[k].grad, want[k])
        print(f"[aa render] d_{k}: rel {e:.2e}, p99 element-wise excess {x:.2f}")
        assert e < RTOL, k
        assert x <= 1.0, f"d_{k}: p99 element-wise excess {x:.2f}"
    # the switch does something: the same scene with it off
    aa.set_antialiasing(False)
    img0, _ = run()
    assert float((img0 - img).abs().max()) > 1e-3


def test_fused_step_uses_the_mode_of_its_forward(device, aa):
    """FusedAdam(fuse_backward=True) over the raw batched path == the unfused autograd path after one step, bit for bit
    (the bar of tests/test_gpu_loss_and_step.py::test_fused_backward_step_equals_k11_then_adam), under mode 1 -- with
    the setting switched OFF between backward and optimizer step: K11 still runs under the forward's mode"""
    from fused_optim import FusedAdam

    dgr = aa
    B, deg, N, W, H = 2, 3, 4099, 320, 208
    cams = S.orbit_cameras(8, W, H, device=device)[:B]
    rasts = [dgr.GaussianRasterizer(settings_from(c, torch.zeros(3), sh_degree=deg)) for c in cams]
    packed = torch.stack([dgr.pack_camera(r.raster_settings) for r in rasts])
    gen = torch.Generator().manual_seed(5)
    ws = [[torch.randn(s, generator=gen).to(device) for s in [(N, 2), (N, 3), (N, 4)]] for _ in range(B)]
    names = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")

    def run(fuse, mode, flip):
        dgr.set_antialiasing(mode)
        m = S.SyntheticGaussianModel(N, W, H, seed=2, device=device, scale_coef=0.002)
        opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=fuse, grad_scale=1.0 / B)
        try:
            raw = [getattr(m, n) for n in names]
            m2, rgb, co, radii, depths = dgr.preprocess_gaussians_raw_batched(*raw, packed, deg, 1.0, W, H)
            loss = sum((m2[k] * ws[k][0]).sum() + (rgb[k] * ws[k][1]).sum() + (co[k] * ws[k][2]).sum() for k in range(B))
            if flip:  # the unfused K11 runs inside backward(), the fused one inside step(): flip before both
                dgr.set_antialiasing(not mode)
            loss.backward()
            assert all((getattr(m, n).grad is None) == fuse for n in names)
            opt.step()
            assert opt.fused_steps == (1 if fuse else 0)
            return [getattr(m, n).detach().clone() for n in names] + \
                [opt.state[getattr(m, n)][k].clone() for n in names for k in ("exp_avg", "exp_avg_sq")]
        finally:
            opt.set_fuse_backward(False)
            dgr.set_antialiasing(True)

    unfused, fused = run(False, True, False), run(True, True, False)
    for flip_fuse in (False, True):
        flipped = run(flip_fuse, True, True)
        for j, (x, y, z) in enumerate(zip(unfused, fused, flipped)):
            assert torch.equal(x, y), f"tensor {j}: fused and unfused differ under mode 1"
            assert torch.equal(x, z), f"tensor {j}: the step after a flip did not use its forward's mode"
    off = run(True, False, False)
    assert not torch.equal(off[1], fused[1]) and not torch.equal(off[5], fused[5]), "mode 1 changed nothing"


def test_captured_iteration_keeps_its_mode_and_refuses_the_other(device, aa, monkeypatch):
    """GraphedIteration at the shape of tests/test_gpu_graphed_step.py, whose loop is reused by import: captured under
    mode 1 it replays equal to the eager mode-1 loop; a replay attempted after set_antialiasing(False) raises, and the
    run goes on unharmed once the setting is back"""
    import graphed_step
    import test_gpu_graphed_step as GS

    steps = 6
    ref = GS._train(device, steps, 1, graph=False)
    refused = []
    call = graphed_step.GraphedIteration.__call__

    def flipping_call(self, *a):
        if self.enabled and self.stats["replayed"] == 1 and not refused:
            aa.set_antialiasing(False)
            try:
                with pytest.raises(RuntimeError, match="set_antialiasing"):
                    call(self, *a)
            finally:
                aa.set_antialiasing(True)
            refused.append(dict(self.stats))
        return call(self, *a)

    monkeypatch.setattr(graphed_step.GraphedIteration, "__call__", flipping_call)
    run = GS._train(device, steps, 1, graph=True)
    st = run[3]
    assert st["disabled"] is None, st
    assert refused and refused[0]["replayed"] == 1, "no replay was attempted under the other mode"
    assert st["captured"] == 1 and st["replayed"] == steps - 2 and st["redone"] == 0, st
    GS._compare(run, ref, steps)


def test_camera_gradients_are_refused(device, aa):
    W, H = 96, 64
    g = _scene(W, H)
    cam = S.orbit_cameras(4, W, H)[1]
    rs = settings_from(cam, torch.zeros(3))
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True))
    rast = aa.GaussianRasterizer(rs)
    gg = {k: v.to(device) for k, v in g.items()}
    with pytest.raises(NotImplementedError, match="set_antialiasing"):
        rast.preprocess_gaussians(*[gg[k] for k in KEYS], {})
    raw = [t.to(device) for t in R.to_raw(g).values()]
    with pytest.raises(NotImplementedError, match="set_antialiasing"):
        rast.preprocess_gaussians_raw(*raw, {})
    packed = aa.pack_camera(rs).view(1, 40)
    assert packed.requires_grad
    with pytest.raises(NotImplementedError, match="set_antialiasing"):
        aa.preprocess_gaussians_raw_batched(*raw, packed, 3, 1.0, W, H)
    aa.set_antialiasing(False)  # ... and with the switch off the same calls go through
    m2 = rast.preprocess_gaussians(*[gg[k] for k in KEYS], {})[0]
    assert m2.shape == (300, 2)
