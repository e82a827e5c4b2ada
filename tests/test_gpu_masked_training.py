"""Loss masks in the training path (gaussian_renderer/loss_distribution.py, set_loss_masks), world size 1: staging ->
render -> batched_loss_computation -> backward on a small synthetic scene whose cameras carry a mask of whole tile
columns.  The loss and the image gradient are fused_band_loss_masked's, the Gaussians that only reach masked pixels receive
exactly no gradient, the switch off (or no mask on the cameras) is the unmasked path bit for bit, an exposure model's
gradient is the direct call's, and a graphed iteration refuses to capture."""
import pytest
import torch

import synthetic_scene as S

pytestmark = pytest.mark.gpu

N, W, H = 2000, 64, 48
MASKED_COLUMNS = 32  # columns [0, 32) = the tile columns 0 and 1 are masked out
u8 = torch.uint8


def _mask(shape3=False):
    m = torch.full((H, W), 255, dtype=u8)
    m[:, :MASKED_COLUMNS] = 0
    return m[None].contiguous() if shape3 else m


def _world(device):
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.WORLD_SIZE = 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=2))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    return utils


def _cameras(device, masks):
    """two cameras 15 degrees apart (what is left of the image in one is left in the other); masks: per camera None, "2d"
    or "3d" """
    cams = S.orbit_cameras(24, W, H, device=device)[:2]
    for k, c in enumerate(cams):
        c.original_image_backup = S.make_gt_image(W, H, seed=10 + k)
        if masks[k] is not None:
            c.alpha_mask_backup = _mask(masks[k] == "3d")
    return cams


def _iteration(device, masks, on, model=None, seed=4):
    """one staged, rendered and differentiated iteration -> dict(loss, parts, images, image grads, parameter grads, pkg,
    cams, strategies)"""
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.loss_distribution import (batched_loss_computation, load_camera_from_cpu_to_all_gpu,
                                                     set_loss_masks)
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    utils = _world(device)
    set_loss_masks(on)
    try:
        gm = S.SyntheticGaussianModel(N, W, H, seed=seed, device=device, scale_coef=0.012) if model is None else model
        cams = _cameras(device, masks)
        hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
        bg = torch.tensor([0.1, 0.2, 0.3], device=device)
        pipe = type("P", (), {"debug": False})()
        strategies, tasks = start_strategy_final(cams, hist)
        assert tasks == [[(0, 0, utils.TILE_Y), (1, 0, utils.TILE_Y)]]
        load_camera_from_cpu_to_all_gpu(cams, strategies, tasks)
        pkg = distributed_preprocess3dgs_and_all2all_final(cams, gm, pipe, bg, batched_strategies=strategies)
        images, cl = render_final(pkg, strategies)
        for im in images:
            im.retain_grad()
        stats = [ca["stats_collector"] for ca in pkg["batched_cuda_args"]]
        loss, parts = batched_loss_computation(images, cams, cl, strategies, stats)
        loss.backward()
        torch.cuda.synchronize()
        names = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
        return dict(loss=loss.detach(), parts=parts, images=[im.detach() for im in images],
                    image_grads=[im.grad.clone() for im in images], cams=cams, pkg=pkg, model=gm,
                    grads={n: getattr(gm, n).grad.detach().clone() for n in names})
    finally:
        set_loss_masks(False)
        utils.set_args(utils.default_args(bsz=1))


def test_masked_iteration_equals_the_direct_call_and_spares_masked_gaussians(device):
    from diff_gaussian_rasterization import fused_band_loss_masked

    r = _iteration(device, ("2d", "3d"), True)
    lam, n = 0.2, H * W * 3
    total = None
    for k, cam in enumerate(r["cams"]):
        assert tuple(cam.alpha_mask.shape) == (1, H, W) and cam.alpha_mask.dtype == u8 and cam.alpha_mask.is_cuda
        assert torch.equal(cam.alpha_mask.cpu()[0], _mask())
        x = r["images"][k].clone().requires_grad_(True)
        want = fused_band_loss_masked(x, cam.original_image, cam.alpha_mask, 0, H, lam, n)
        want[0].backward()
        assert torch.equal(r["parts"][k][0], want[1]) and torch.equal(r["parts"][k][1], want[2])
        assert torch.equal(r["image_grads"][k], x.grad), "the image gradient is not the direct call's"
        assert bool((r["image_grads"][k][:, :, :MASKED_COLUMNS] == 0).all())
        assert bool((r["image_grads"][k][:, :, MASKED_COLUMNS:] != 0).any())
        total = want[0].detach() if total is None else total + want[0].detach()
    assert torch.equal(r["loss"], total), "the loss is not the sum of the direct calls"
    # Gaussians whose tile rectangle, in every camera that sees them, lies wholly in the masked tile columns: the
    # rectangle of 16-pixel tiles a Gaussian is binned into ends before column 32 iff x + radius + 15 < 48
    pkg = r["pkg"]
    seen_any = torch.zeros(N, dtype=torch.bool, device=device)
    outside_any = torch.zeros(N, dtype=torch.bool, device=device)
    for k in range(2):
        m2, radii = pkg["batched_locally_preprocessed_mean2D"][k].detach(), pkg["batched_locally_preprocessed_radii"][k]
        seen = radii > 0
        inside = m2[:, 0] + radii.float() + 15.0 < float(MASKED_COLUMNS + 16) - 0.5
        seen_any |= seen
        outside_any |= seen & ~inside
    spared = seen_any & ~outside_any
    reached = outside_any
    assert int(spared.sum()) > 0 and int(reached.sum()) > 0, (int(spared.sum()), int(reached.sum()))
    print(f"INFO masked training: {int(spared.sum())} Gaussians only reach masked pixels, {int(reached.sum())} reach others")
    for name, g in r["grads"].items():
        assert bool(torch.isfinite(g).all()), name
        assert bool((g[spared] == 0).all()), f"{name}: a Gaussian that only reaches masked pixels received a gradient"
        assert bool((g[reached] != 0).any()), f"{name}: nobody received a gradient"


@pytest.mark.parametrize("masks,on", [(("2d", "3d"), False), ((None, None), True)])
def test_switch_off_or_no_mask_is_the_unmasked_path(device, masks, on):
    a = _iteration(device, masks, on)
    b = _iteration(device, (None, None), False)
    assert torch.equal(a["loss"], b["loss"])
    for x, y in zip(a["image_grads"], b["image_grads"]):
        assert torch.equal(x, y)
    for name in a["grads"]:
        assert torch.equal(a["grads"][name], b["grads"][name]), name
    for cam in a["cams"]:
        assert getattr(cam, "alpha_mask", None) is None
    # (and a mask does change the loss)
    c = _iteration(device, ("2d", None), True)
    assert not torch.equal(c["loss"], b["loss"])
    assert c["cams"][0].alpha_mask is not None and getattr(c["cams"][1], "alpha_mask", None) is None
    assert torch.equal(c["image_grads"][1], b["image_grads"][1])  # the camera without a mask: the unmasked path


def test_masked_iteration_with_an_exposure_model(device):
    from diff_gaussian_rasterization import fused_band_loss_masked
    from exposure import ExposureModel
    from gaussian_renderer.loss_distribution import set_exposure_model

    E = [[1.10, 0.15, -0.20, 0.05], [-0.10, 0.90, 0.20, -0.10], [0.20, -0.15, 1.05, 0.08]]
    model = ExposureModel(4, device=device)
    with torch.no_grad():
        for uid in range(4):
            model.exposure[uid].copy_(torch.tensor(E, device=device) * (1.0 + 0.05 * uid))
    set_exposure_model(model)
    try:
        r = _iteration(device, ("2d", "2d"), True)
    finally:
        set_exposure_model(None)
    g = model.exposure.grad
    assert g is not None
    lam, n = 0.2, H * W * 3
    total = None
    want_g = torch.zeros_like(g)
    for k, cam in enumerate(r["cams"]):
        x = r["images"][k].clone().requires_grad_(True)
        Ek = model.exposure[cam.uid].detach().clone().requires_grad_(True)
        want = fused_band_loss_masked(x, cam.original_image, cam.alpha_mask, 0, H, lam, n, exposure=Ek)
        want[0].backward()
        assert torch.equal(r["image_grads"][k], x.grad)
        assert bool((r["image_grads"][k][:, :, :MASKED_COLUMNS] == 0).all())
        want_g[cam.uid] += Ek.grad
        total = want[0].detach() if total is None else total + want[0].detach()
    assert torch.equal(r["loss"], total)
    assert torch.equal(g, want_g) and bool((g != 0).any()), "the model's gradient is not the direct call's"


def test_graphed_iteration_refuses_masked_cameras(device):
    from fused_optim import FusedAdam
    from gaussian_renderer.loss_distribution import set_loss_masks
    from graphed_step import GraphedIteration

    calls = []
    m = S.SyntheticGaussianModel(64, W, H, seed=1, device=device)
    step = GraphedIteration(FusedAdam(m.param_groups(), lr=0.0, eps=1e-15), lambda *a: calls.append(a), warmup=1)
    cams = _cameras(device, ("2d", None))
    set_loss_masks(True)
    try:
        with pytest.raises(RuntimeError, match="loss masks are on"):
            step(cams, [], [])
    finally:
        set_loss_masks(False)
    assert not calls and not step.entries and step.stats["captured"] == 0 and step.stats["eager"] == 0
