"""Exposure compensation in the training path: gaussian_renderer.loss_distribution with an ExposureModel set, the model's
Adam step on the device, and the refusal of a graphed iteration."""
import types

import pytest
import torch

import leaf_refs as R
from helpers import assert_elem_close

pytestmark = pytest.mark.gpu

K = 8
f32, u8, i32 = torch.float32, torch.uint8, torch.int32
E_TEST = [[1.10, 0.15, -0.20, 0.05], [-0.10, 0.90, 0.20, -0.10], [0.20, -0.15, 1.05, 0.08]]


def _setup(rank):
    import utils.general_utils as utils

    saved = (utils.GLOBAL_RANK, utils.WORLD_SIZE, utils.DEFAULT_GROUP, utils.IN_NODE_GROUP)
    utils.GLOBAL_RANK, utils.WORLD_SIZE = rank, 2
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()  # (no collective runs; no timing consumer)
    utils.set_args(utils.default_args(bsz=1))
    utils.set_img_size(48, 64)
    return saved


def _restore(saved):
    import utils.general_utils as utils
    from gaussian_renderer.loss_distribution import set_exposure_model

    set_exposure_model(None)
    utils.GLOBAL_RANK, utils.WORLD_SIZE, utils.DEFAULT_GROUP, utils.IN_NODE_GROUP = saved
    utils.set_args(utils.default_args(bsz=1))


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("rank", [0, 1])
def test_batched_loss_with_a_model_set(device, rank, dyn):
    """a 64x48 image (three tile rows) cut into the bands [0, 32) and [32, 48) of two ranks: with a model set the loss of
    this rank's band is fused_band_loss_exposure's with the camera's row, bit for bit, and only that row of the model
    receives a gradient; with the model taken away the call is the plain path again"""
    from diff_gaussian_rasterization import fused_band_loss, fused_band_loss_exposure
    from exposure import ExposureModel
    from gaussian_renderer.loss_distribution import batched_loss_computation, set_exposure_model

    H, W, uid, lam = 48, 64, 2, 0.2
    y0, y1 = (0, 32) if rank == 0 else (32, 48)
    rows = y1 - y0
    x, gt_full, _ = R.loss_inputs("noise", 3, H, W)
    cap = rows + 16
    band_rows = torch.tensor([y0, y1], dtype=i32, device=device) if dyn else None
    gt = gt_full[:, y0:y1].contiguous().to(device)
    if dyn:  # a capacity-sized buffer that carries the band in its first rows (graphed_step.py)
        buf = torch.full((3, cap, W), 0xA5, dtype=u8, device=device)
        buf[:, :rows] = gt
        gt = buf
    strategy = types.SimpleNamespace(gpu_ids=[0, 1], division_pos=[0, 2, 3])
    if dyn:
        strategy._gsr_dyn_band = band_rows
    camera = types.SimpleNamespace(uid=uid, original_image=gt)
    saved = _setup(rank)
    try:
        model = ExposureModel(4, device=device)
        with torch.no_grad():
            model.exposure[uid].copy_(torch.tensor(E_TEST, device=device))
        set_exposure_model(model)
        img = x.to(device).requires_grad_(True)
        loss, parts = batched_loss_computation([img], [camera], [None], [strategy], [{}])
        loss.backward()
        ref_img = x.to(device).requires_grad_(True)
        ref_E = torch.tensor(E_TEST, device=device).requires_grad_(True)
        want = fused_band_loss_exposure(ref_img, ref_E, gt, y0 if not dyn else 0, y1 if not dyn else 0, lam, H * W * 3,
                                        band_rows)
        want[0].backward()
        assert torch.equal(loss.detach(), want[0].detach()) and torch.equal(img.grad, ref_img.grad)
        assert torch.equal(parts[0][0], want[1]) and torch.equal(parts[0][1], want[2])
        g = model.exposure.grad
        assert g is not None and torch.equal(g[uid], ref_E.grad) and bool((g[uid] != 0).any())
        others = [k for k in range(4) if k != uid]
        assert bool((g[others] == 0).all()), "only the camera's row may receive a gradient"
        # the model taken away: the present path, bit for bit
        set_exposure_model(None)
        img2 = x.to(device).requires_grad_(True)
        loss2, _ = batched_loss_computation([img2], [camera], [None], [strategy], [{}])
        loss2.backward()
        ref2 = x.to(device).requires_grad_(True)
        want2 = fused_band_loss(ref2, gt, y0 if not dyn else 0, y1 if not dyn else 0, lam, H * W * 3, band_rows)
        want2[0].backward()
        assert torch.equal(loss2.detach(), want2[0].detach()) and torch.equal(img2.grad, ref2.grad)
        assert not torch.equal(loss2.detach(), loss.detach())  # (the exposure did change the loss)
    finally:
        _restore(saved)


def test_exposure_model_step_on_the_device(device):
    """three updates against leaf_refs.adam_reference in fp64 (the rule of test_gpu_adam_edges.py: K times the error of
    torch.optim.Adam in fp32), each at the learning rate of the stated schedule"""
    from exposure import ExposureModel

    n, lr0, lr1, T = 7, 0.01, 0.001, 10
    model = ExposureModel(n, lr_init=lr0, lr_final=lr1, max_steps=T, device=device)
    gen = torch.Generator().manual_seed(11)
    p0 = model.exposure.detach().cpu().reshape(-1).clone()
    s64 = (p0.double(), torch.zeros(n * 12, dtype=torch.float64), torch.zeros(n * 12, dtype=torch.float64))
    s32 = (p0.clone(), torch.zeros(n * 12), torch.zeros(n * 12))
    for k in (1, 2, 3):
        g = torch.randn(n * 12, generator=gen) * 0.3
        g[::5] = 0.0
        lr = lr0 * (lr1 / lr0) ** (k / T)
        assert abs(model.lr_at(k) - lr) <= 1e-15
        model.exposure.grad = g.reshape(n, 3, 4).to(device)
        model.step()
        torch.cuda.synchronize()
        assert model.steps == k and model.exposure.grad is None
        hp = dict(lr=lr, b1=0.9, b2=0.999, eps=1e-8, step=k, grad_scale=1.0)
        s64 = R.adam_reference(s64[0], g, s64[1], s64[2], **hp)
        s32 = R.adam_torch32(s32[0], g, s32[1], s32[2], **hp)
        got = [t.detach().cpu().reshape(-1) for t in (model.exposure, model.exp_avg, model.exp_avg_sq)]
        for name, a, b, c in zip("pmv", got, s64, s32):
            ratio = assert_elem_close(a, b, c, K=K, what=f"exposure adam step {k} {name}")
            print(f"RATIO exposure adam_{name} step={k} {ratio:.4g}")
    assert model.lr_at(0) == lr0 and abs(model.lr_at(T) - lr1) <= 1e-15 and model.lr_at(5 * T) == model.lr_at(T)
    # the state survives a checkpoint round trip on the device
    other = ExposureModel(n, lr_init=lr0, lr_final=lr1, max_steps=T, device=device)
    other.load_state_dict(model.state_dict())
    assert other.steps == 3 and torch.equal(other.exposure.detach(), model.exposure.detach())
    assert torch.equal(other.exp_avg, model.exp_avg) and torch.equal(other.exp_avg_sq, model.exp_avg_sq)


def test_graphed_iteration_refuses_an_exposure_model(device):
    import synthetic_scene as S
    from exposure import ExposureModel
    from fused_optim import FusedAdam
    from gaussian_renderer.loss_distribution import set_exposure_model
    from graphed_step import GraphedIteration

    calls = []
    m = S.SyntheticGaussianModel(64, 64, 48, seed=1, device=device)
    step = GraphedIteration(FusedAdam(m.param_groups(), lr=0.0, eps=1e-15), lambda *a: calls.append(a), warmup=1)
    set_exposure_model(ExposureModel(2, device=device))
    try:
        with pytest.raises(RuntimeError, match="exposure model is set"):
            step([], [], [])
    finally:
        set_exposure_model(None)
    assert not calls and not step.entries and step.stats["captured"] == 0 and step.stats["eager"] == 0
