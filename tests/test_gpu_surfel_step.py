"""The surfel geometry pass in the training step (gaussian_renderer.set_surfel_pass), world size 1, one small synthetic
scene (2000 Gaussians, 64 x 48, two views): the fused pass against the SEPARATE passes it replaces -- render_features
under the plain normals mode, and gsr_render_distortion(_backward) through the C ABI (an autograd Function here: the
operator has no distortion op of its own).  Both sides are fp32 kernels, so the separate side is the reference and the
unit is helpers.ROW_UNIT_FLOOR.  What the pass itself emits is held per ROW, error / (floor x the row's largest value)
<= K, zero rows exactly zero: the map per pixel with composite_refs.K_FORWARD, the distortion map with its K, the
means2D gradient of normal_consistency_loss + distortion_loss with surfel_refs.K_of's d_means2D.  xyz and rotation lie
behind K11 and the rows' backward, the SAME unchanged kernels on both sides, which cancel within a row (a quaternion's
gradient is what is left of terms that cancel along it): a row's relative error there is the emitted error times that
row's condition number, which no K knows (measured on an MI355X: worst row 57 x floor for xyz, 242 for rotation, with
means2D at 37.8).  They are held norm-wise to 1e-6, the bound tests/test_gpu_normals.py sets for two fp32 paths that
round the same sums (measured 1.5e-7 and 5.2e-7).  Each figure is printed before it is asserted.  The refusals carry no
gpu mark and run with the CPU suite, as tests/test_gpu_normals.py's do: they come before any launch."""
import types

import pytest
import torch

import surfel_refs as SR
import synthetic_scene as S
import test_gpu_normals as TN
from helpers import ROW_UNIT_FLOOR, rel_err

N, WEIGHT_N, WEIGHT_D = 2000, 0.5, 100.0
STEP = types.SimpleNamespace(family="step")  # (surfel_refs.K_of asks a case for its family only)


def _batch(dev, surfels):
    """a fresh model and the two views rendered under the normals mode, with or without the pass -> (model, pkg, batch)"""
    import gaussian_renderer as gr

    model = S.SyntheticGaussianModel(N, TN.PW, TN.PH, seed=TN.SEED, sh_degree=TN.DEG, device=dev, scale_coef=TN.SCALE)
    TN._single_rank(2)
    gr.set_normal_consistency(True)
    try:
        gr.set_surfel_pass(surfels, distortion="depth" if surfels else None)
        _, pkg, batch = TN._render_batch(model, dev, True)
    finally:
        gr.set_surfel_pass(False)
        gr.set_normal_consistency(False)
    return model, pkg, batch


class _SeparateDistortion(torch.autograd.Function):
    """gsr_render_distortion and its backward on the view tuple the colour render left, m = depth"""

    @staticmethod
    def forward(ctx, means2D, conic_opacity, depths, view):
        import diff_gaussian_rasterization as dgr

        ranges, point_list, mask, band, final_T, n_contrib, W, H = view
        ctx.maps = torch.empty((4, H, W), device=means2D.device)
        ctx.keep = (ranges, point_list, means2D, conic_opacity, depths, mask, n_contrib)
        ctx.args = (means2D.shape[0], W, H, *map(dgr._ptr, ctx.keep), 0.0, 1.0, 0.0)
        ctx.tail = (band, final_T)
        dgr.check(dgr.lib.gsr_render_distortion(*ctx.args, *band, dgr._ptr(ctx.maps), dgr._stream()), "distortion")
        return ctx.maps[0]

    @staticmethod
    def backward(ctx, g):
        import diff_gaussian_rasterization as dgr

        band, final_T = ctx.tail
        rec = torch.empty((ctx.args[0], 7), device=g.device)
        acc = torch.empty((ctx.args[0], 7), dtype=torch.float64, device=g.device)
        dgr.check(dgr.lib.gsr_render_distortion_backward(*ctx.args, dgr._ptr(final_T), dgr._ptr(ctx.maps),
                                                         dgr._ptr(g.float().contiguous()), *band, dgr._ptr(rec),
                                                         dgr._ptr(acc), dgr._stream()), "distortion backward")
        return rec[:, 0:2], rec[:, 2:6], rec[:, 6], None


def _worst_row(got, want):
    """max over the rows of error / (ROW_UNIT_FLOOR x the row's largest value); inf when a zero row is not zero"""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    err, s = (g - w).abs().amax(dim=1), w.abs().amax(dim=1)
    return float(torch.where(s > 0, err / (ROW_UNIT_FLOOR * s.clamp(min=1e-300)),
                             torch.where(err == 0, 0.0, float("inf"))).max())


@pytest.mark.gpu
def test_the_fused_pass_against_the_separate_passes(device):
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer.loss_distribution import distortion_loss, normal_consistency_loss

    (fused, pkg, batch), (plain, ref, _) = _batch(device, True), _batch(device, False)
    assert not any(k in ref for k in ("batched_distortion", "batched_median_depth", "batched_median_pos", "_surfel_pass"))
    dist = []
    for k in range(2):
        f, f0 = pkg["batched_features"][k], ref["batched_features"][k]
        assert f.shape == f0.shape == (5, TN.PH, TN.PW)
        d = _SeparateDistortion.apply(ref["batched_means2D_redistributed"][k], ref["batched_conic_opacity_redistributed"][k],
                                      ref["_features_rows"][k][:, 1].contiguous(), ref["batched_cuda_args"][k][dgr._FEATURES_KEY])
        dist.append(d)
        wf, wd = _worst_row(f.reshape(5, -1).T, f0.reshape(5, -1).T), _worst_row(pkg["batched_distortion"][k].reshape(-1, 1), d.reshape(-1, 1))
        print(f"SURFELS step view {k}: worst pixel of the map {wf:.3g}, of the distortion map {wd:.3g} (x unit floor)")
        assert wf <= SR.R.K_FORWARD and wd <= SR.K_of(STEP, "Dist") and bool(d.any())
        pos, med = pkg["batched_median_pos"][k], pkg["batched_median_depth"][k]
        assert pos.dtype == torch.int32 and torch.equal(pos > 0, f[0] > 0) and torch.equal(med > 0, pos > 0)
    (normal_consistency_loss(pkg, batch, WEIGHT_N) + distortion_loss(pkg, batch, WEIGHT_D)).backward()
    (normal_consistency_loss(ref, batch, WEIGHT_N) + sum(d.sum() * (WEIGHT_D / d.numel()) for d in dist)).backward()
    torch.cuda.synchronize()
    m2 = [torch.cat([m.grad for m in p["batched_locally_preprocessed_mean2D"]]) for p in (pkg, ref)]
    worst = _worst_row(*m2)
    print(f"SURFELS step d_means2D: worst row {worst:.3g} x unit floor (K = {SR.K_of(STEP, 'd_means2D')})")
    assert worst <= SR.K_of(STEP, "d_means2D") and bool(m2[1].any())
    for name in ("_xyz", "_rotation"):
        got, want = getattr(fused, name).grad, getattr(plain, name).grad
        e = rel_err(got, want)
        print(f"SURFELS step d{name}: rel err {e:.3g} (worst row {_worst_row(got, want):.3g} x unit floor)")
        assert e < 1e-6 and bool(want.any()), name


def test_the_refusals_come_before_any_launch(monkeypatch):
    import gaussian_renderer as gr
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final as prep
    from gaussian_renderer.loss_distribution import distortion_loss

    TN._single_rank(1)
    with pytest.raises(ValueError, match="set_normal_consistency"):
        gr.set_surfel_pass(True)
    monkeypatch.setattr(gr, "_SURFELS", [True, None])  # (GSR_SURFELS=1 without GSR_NORMALS=1: the call itself refuses)
    with pytest.raises(ValueError, match="set_normal_consistency"):
        prep([], None, None, None, batched_strategies=[])
    monkeypatch.setattr(gr, "_NORMALS", [True])
    with pytest.raises(ValueError, match="distortion"):
        gr.set_surfel_pass(True, distortion="sideways")
    monkeypatch.setattr(gr, "_FEATURES", [True])  # every refusal of the normals mode is the pass's
    with pytest.raises(ValueError, match="together with set_features"):
        prep([], None, None, None, batched_strategies=[])
    with pytest.raises(RuntimeError, match="set_surfel_pass"):
        distortion_loss({}, [], 1.0)
    with pytest.raises(RuntimeError, match="without a distortion mapping"):
        distortion_loss({"batched_distortion": [None], "_surfel_pass": (None,)}, [], 1.0)
    monkeypatch.undo()
    assert not gr.get_surfel_pass() and not gr.get_normal_consistency()
