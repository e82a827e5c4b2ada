"""-m gpu: the bilateral grid through the Python layers -- bilagrid.BilateralGridModel,
loss_distribution.set_bilateral_grid, batched_loss_computation -- on the small synthetic scene of
tests/test_gpu_invdepth_pipeline.py (2 000 Gaussians at 96 x 64, one rank) and, for the gradient all-reduce, on two bands
of tests/fake_world.py."""
import types

import pytest
import torch

import bilagrid_refs as B
import synthetic_scene as S
from helpers import assert_elem_close

pytestmark = pytest.mark.gpu

N, W, H, DEG, SCALE, SEED, VIEW = 2000, 96, 64, 1, 0.01, 5, 1
ALL = ["_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest"]
SIZES = (5, 4, 6)   # (GW, GH, L): three different sizes
NCAM = 4
K = 8
SUM_FLOOR = 2e-5    # the relative floor of a loss value (tests/test_gpu_exposure_loss.py)
i32 = torch.int32


def _single_rank(**args):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True, **args))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    wd._BALANCE["mode"] = "exact"
    gr._PLANNERS.clear()


def _clear():
    from gaussian_renderer import loss_distribution as ld

    ld.set_bilateral_grid(None)
    ld.set_loss_masks(False)


def _scene_step(dev, model_or_none):
    """render view VIEW of a fresh scene, take batched_loss_computation's loss against a random ground truth, backward
    -> (loss, {name: grad}, rendered image)"""
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer import loss_distribution as ld
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    _single_rank()
    scene = S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, device=dev, scale_coef=SCALE)
    cams = S.orbit_cameras(NCAM, W, H, device=dev)
    cam = cams[VIEW]
    cam.original_image = S.make_gt_image(W, H, seed=3, device=dev)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    strategies, _ = start_strategy_final([cam], hist)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    pkg = distributed_preprocess3dgs_and_all2all_final([cam], scene, pipe, bg, batched_strategies=strategies, mode="train")
    images, _ = render_final(pkg, strategies)
    ld.set_bilateral_grid(model_or_none)
    try:
        loss, _ = ld.batched_loss_computation(images, [cam], [None], strategies, [{}])
        loss.backward()
    finally:
        ld.set_bilateral_grid(None)
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: getattr(scene, n).grad.clone() for n in ALL}, images[0].detach().clone()


def _perturb(model, seed=2):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        model.grids.add_((0.1 * torch.randn(model.grids.shape, generator=g)).to(model.grids.device))


def test_fresh_model_keeps_the_bits_and_a_perturbed_one_matches_the_restatement(device):
    from bilagrid import BilateralGridModel
    from oracle.loss_oracle import band_loss

    plain_loss, plain_grads, image = _scene_step(device, None)
    model = BilateralGridModel(NCAM, grid=SIZES, device=device)
    loss, grads, _ = _scene_step(device, model)
    assert torch.equal(loss.view(i32), plain_loss.view(i32)), "an identity grid changed the loss"
    for n in ALL:
        assert torch.equal(grads[n], plain_grads[n]), f"an identity grid changed the gradient of {n}"
    assert bool(plain_grads["_xyz"].any())
    g = model.grids.grad
    assert g is not None and bool(g[VIEW].any())
    assert bool((g[[k for k in range(NCAM) if k != VIEW]] == 0).all()), "only the camera's row may receive a gradient"
    # perturbed grids: the existing loss of the restatement's corrected image
    model.zero_grad()
    _perturb(model)
    loss2, grads2, image2 = _scene_step(device, model)
    assert torch.equal(image2, image) and not torch.equal(loss2, plain_loss)
    assert not torch.equal(grads2["_features_dc"], plain_grads["_features_dc"])
    gt = S.make_gt_image(W, H, seed=3)
    ref = {}
    for dt in (torch.float64, torch.float32):
        corrected = B.slice_reference(image.cpu(), model.grids.detach()[VIEW].cpu(), dt)
        ref[dt] = float(band_loss(corrected, gt, H, W, 0.2)[0])
    want, w32 = ref[torch.float64], ref[torch.float32]
    ratio = abs(float(loss2) - want) / max(abs(w32 - want), SUM_FLOOR * abs(want))
    print(f"RATIO bilagrid pipeline_loss {ratio:.4g} (loss {float(loss2):.9g}, fp64 {want:.9g})")
    assert ratio <= K


def test_step_counts_changes_and_round_trips(device):
    from bilagrid import BilateralGridModel

    model = BilateralGridModel(NCAM, grid=SIZES, device=device, max_steps=10)
    _perturb(model)
    before = model.grids.detach().clone()
    g = torch.Generator().manual_seed(8)
    model.grids.grad = torch.randn(model.grids.shape, generator=g).to(device)
    model.grids.grad[0] = 0.0  # a camera nobody rendered still feels the total variation
    model.step()
    torch.cuda.synchronize()
    assert model.steps == 1 and model.grids.grad is None
    moved = model.grids.detach() != before
    assert bool(moved[1:].all()) and bool(moved[0].any())
    # the first Adam step moves every element with a gradient by lr_at(1) (m / sqrt(v) = +-1 at eps = 1e-15)
    step = (model.grids.detach() - before)[1:].abs()
    assert float((step - model.lr_at(1)).abs().max()) <= 1e-3 * model.lr_at(1)
    # tv_weight = 0: rows without a gradient stay
    still = BilateralGridModel(2, grid=SIZES, device=device, tv_weight=0.0)
    _perturb(still)
    b2 = still.grids.detach().clone()
    still.grids.grad = torch.zeros_like(still.grids)
    still.grids.grad[1] = 1.0
    still.step()
    assert torch.equal(still.grids.detach()[0], b2[0]) and not torch.equal(still.grids.detach()[1], b2[1])
    other = BilateralGridModel(NCAM, grid=SIZES, device=device, max_steps=10)
    other.load_state_dict(model.state_dict())
    assert other.steps == 1 and torch.equal(other.grids.detach(), model.grids.detach())
    assert torch.equal(other.exp_avg, model.exp_avg) and torch.equal(other.exp_avg_sq, model.exp_avg_sq)
    model.grids.grad = torch.ones_like(model.grids)
    other.grids.grad = torch.ones_like(other.grids)
    model.step(), other.step()
    assert model.steps == other.steps == 2 and torch.equal(other.grids.detach(), model.grids.detach())


def _band_call(dev, rank, world_ranks, division, image, gt_full, model, mask_full=None, lam=0.2):
    """batched_loss_computation of one rank's band of a given image -> (loss, image gradient)"""
    import utils.general_utils as utils
    from gaussian_renderer import loss_distribution as ld

    y0, y1 = division[rank] * 16, min(division[rank + 1] * 16, H)
    cam = types.SimpleNamespace(uid=VIEW, original_image=gt_full[:, y0:y1].contiguous().to(dev))
    if mask_full is not None:
        cam.alpha_mask = mask_full[:, y0:y1].contiguous().to(dev)
    strategy = types.SimpleNamespace(gpu_ids=list(range(world_ranks)), division_pos=division)
    utils.set_args(utils.default_args(bsz=1, lambda_dssim=lam))
    utils.set_img_size(H, W)
    img = image.to(dev).requires_grad_(True)
    ld.set_bilateral_grid(model)
    ld.set_loss_masks(mask_full is not None)
    try:
        loss, _ = ld.batched_loss_computation([img], [cam], [None], [strategy], [{}])
        loss.backward()
    finally:
        _clear()
    return loss.detach(), img.grad, (y0, y1), cam


def test_mask_applies_to_the_corrected_image(device):
    from bilagrid import BilateralGridModel
    from diff_gaussian_rasterization import bilagrid_slice, fused_band_loss_masked

    _single_rank()
    image = B.make_image(W, H, SIZES[2], 3)
    gt = S.make_gt_image(W, H, seed=3)
    mask = torch.randint(0, 256, (1, H, W), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
    mask[:, :, :20] = 0
    model = BilateralGridModel(NCAM, grid=SIZES, device=device)
    _perturb(model)
    loss, gimg, (y0, y1), cam = _band_call(device, 0, 1, [0, 4], image, gt, model, mask_full=mask)
    x = image.to(device).requires_grad_(True)
    grid = model.grids.detach()[VIEW].clone().requires_grad_(True)
    want = fused_band_loss_masked(bilagrid_slice(x, grid, y0, y1, H), cam.original_image, cam.alpha_mask, y0, y1, 0.2,
                                  H * W * 3)
    want[0].backward()
    assert torch.equal(loss.view(i32), want[0].detach().view(i32)) and torch.equal(gimg, x.grad)
    assert torch.equal(model.grids.grad[VIEW], grid.grad) and bool(grid.grad.any())
    assert bool((gimg[:, :, :20] == 0).all()), "a pixel the mask switches off received a gradient"
    unmasked, _, _, _ = _band_call(device, 0, 1, [0, 4], image, gt, model)
    assert not torch.equal(unmasked, loss)


def test_two_ranks_gradients_sum_to_the_one_rank_gradient(device):
    """World size 2 on tests/fake_world.py, bands [0, 32) and [32, 64) of one image.  lambda_dssim = 0: the band-local
    SSIM pads every band with zeros and so is not additive over bands by design, the L1 term is.  The two partial
    lattice gradients, summed by sync_grads (one all_reduce), then equal the one-rank gradient up to the rounding of two
    fp64 sums instead of one: K * 4 half-ulps of the largest element (assert_elem_close's floor)."""
    import utils.general_utils as utils
    from bilagrid import BilateralGridModel
    from fake_world import FakeWorld

    image = B.make_image(W, H, SIZES[2], 3)
    gt = S.make_gt_image(W, H, seed=3)
    saved = (utils.GLOBAL_RANK, utils.WORLD_SIZE, utils.DEFAULT_GROUP, utils.IN_NODE_GROUP)
    fw = FakeWorld(2, device)

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, 2
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        model = BilateralGridModel(NCAM, grid=SIZES, device=device)
        _perturb(model)
        _band_call(device, rank, 2, [0, 2, 4], image, gt, model, lam=0.0)
        partial = model.grids.grad.clone()
        before = len(fw.log)
        model.sync_grads(fw.groups[rank])
        summed = model.grids.grad.clone()
        model.step()
        return dict(partial=partial, summed=summed, steps=model.steps, grids=model.grids.detach().clone(),
                    reduces=[t for _, t in fw.log[before:] if t == "all_reduce"], others=[t for _, t in fw.log[before:]
                                                                                         if not t.startswith("all_reduce")])

    try:
        res = fw.run(rank_main, timeout=120)
    finally:
        _clear()
        utils.GLOBAL_RANK, utils.WORLD_SIZE, utils.DEFAULT_GROUP, utils.IN_NODE_GROUP = saved
    assert [t for _, t in fw.log if t == "all_reduce"] == ["all_reduce"], f"not exactly one collective per step: {fw.log}"
    assert not [t for _, t in fw.log if not t.startswith("all_reduce")], fw.log
    assert bool(res[0]["partial"].any()) and bool(res[1]["partial"].any())
    assert not torch.equal(res[0]["partial"], res[1]["partial"])
    assert torch.equal(res[0]["summed"], res[1]["summed"]) and torch.equal(res[0]["grids"], res[1]["grids"])
    assert res[0]["steps"] == res[1]["steps"] == 1
    _single_rank()
    one = BilateralGridModel(NCAM, grid=SIZES, device=device)
    _perturb(one)
    _band_call(device, 0, 1, [0, 4], image, gt, one, lam=0.0)
    ratio = assert_elem_close(res[0]["summed"].cpu(), one.grids.grad.double().cpu(), one.grids.grad.cpu(), K=K,
                              what="two ranks' summed lattice gradient")
    print(f"RATIO bilagrid two_ranks_grad {ratio:.4g}")


def test_a_graph_capture_is_refused(device):
    from bilagrid import BilateralGridModel
    from fused_optim import FusedAdam
    from gaussian_renderer.loss_distribution import set_bilateral_grid
    from graphed_step import GraphedIteration

    calls = []
    m = S.SyntheticGaussianModel(64, 64, 48, seed=1, device=device)
    step = GraphedIteration(FusedAdam(m.param_groups(), lr=0.0, eps=1e-15), lambda *a: calls.append(a), warmup=1)
    set_bilateral_grid(BilateralGridModel(2, grid=(2, 2, 2), device=device))
    try:
        with pytest.raises(RuntimeError, match="bilateral-grid model is set"):
            step([], [], [])
    finally:
        set_bilateral_grid(None)
    assert not calls and not step.entries and step.stats["captured"] == 0 and step.stats["eager"] == 0


def test_both_colour_models_are_refused(device):
    from bilagrid import BilateralGridModel
    from exposure import ExposureModel
    from gaussian_renderer import loss_distribution as ld

    try:
        ld.set_bilateral_grid(BilateralGridModel(1, grid=(2, 2, 2), device=device))
        with pytest.raises(ValueError, match="set_exposure_model.*set_bilateral_grid"):
            ld.set_exposure_model(ExposureModel(1, device=device))
    finally:
        ld.set_bilateral_grid(None)
        ld.set_exposure_model(None)
