"""Deferred rounding in the training iteration (diff_gaussian_rasterization: _DEFERRED): three steps through the
gaussian_renderer mirror with the rounding of K10's record left to the fused K11 + Adam launch equal three steps with
the switch off -- parameters and both moments, torch.equal -- at one camera (the one-camera kernel) and at two (the
camera-batched one).  In the second step the per-iteration densification statistics read `means2D.grad` between
backward and step, which has the record rounded after all; a run with fuse_backward=False (never armed: K11 and Adam as
two kernels) must land on the same bits too.  The counters say which path each step took."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")
N, W, H = 20000, 320, 208


def _three_steps(device, bsz, fuse, switch):
    import densification_ops as D
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    import synthetic_scene as S
    import utils.general_utils as utils
    from fused_optim import FusedAdam
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.loss_distribution import batched_loss_computation, load_camera_from_cpu_to_all_gpu
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=bsz))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    gr.set_exchange_forced(False)
    cams = S.orbit_cameras(8, W, H, device=device)[:4]
    for k, cam in enumerate(cams):
        cam.original_image_backup = S.make_gt_image(W, H, seed=1 + k, device=device)
    bg = torch.zeros(3, device=device)
    pipe = type("P", (), {"debug": False})()
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    m = S.SyntheticGaussianModel(N, W, H, seed=3, device=device, scale_coef=0.012)
    m.xyz_gradient_accum = torch.zeros((N, 1), device=device)
    m.denom = torch.zeros((N, 1), device=device)
    m.max_radii2D = torch.zeros((N,), device=device)
    initial = [getattr(m, n).detach().clone() for n in NAMES]
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=fuse, grad_scale=1.0 / bsz)
    dgr.set_deferred_rounding(switch)
    before = dict(dgr.deferred_rounding_stats)
    per_step = []
    try:
        for it in range(3):
            batch = [cams[(it * bsz + j) % len(cams)] for j in range(bsz)]
            utils.set_cur_iter(utils.get_cur_iter() + bsz)
            st, tasks = start_strategy_final(batch, hist)
            load_camera_from_cpu_to_all_gpu(batch, st, tasks)
            pkg = distributed_preprocess3dgs_and_all2all_final(batch, m, pipe, bg, batched_strategies=st, mode="train")
            images, masks = render_final(pkg, st)
            stats = [ca["stats_collector"] for ca in pkg["batched_cuda_args"]]
            loss, _ = batched_loss_computation(images, batch, masks, st, stats)
            loss.backward()
            assert all(v.grad is not None for v in pkg["batched_locally_preprocessed_mean2D"])
            if it == 1:  # densification.py:13-25 of the reference, between backward and step
                with torch.no_grad():
                    for k in range(bsz):
                        D.update_densification_stats(m, pkg["batched_locally_preprocessed_mean2D"][k],
                                                     pkg["batched_locally_preprocessed_radii"][k])
            opt.step()
            opt.zero_grad(set_to_none=True)
            now = dict(dgr.deferred_rounding_stats)
            per_step.append({k: now[k] - before[k] for k in now})
            before = now
        torch.cuda.synchronize()
        assert opt.fused_steps == (3 if fuse else 0) and opt.materialized_steps == 0
        state = [getattr(m, n).detach().clone() for n in NAMES] + \
                [opt.state[getattr(m, n)][k].clone() for n in NAMES for k in ("exp_avg", "exp_avg_sq")] + \
                [m.xyz_gradient_accum.clone(), m.denom.clone(), m.max_radii2D.clone()]
    finally:
        opt.set_fuse_backward(False)
        dgr.set_deferred_rounding("env")
    return state, per_step, initial


@pytest.mark.parametrize("bsz", [1, 2])
def test_three_training_steps_equal_with_and_without_deferred_rounding(device, bsz):
    ref, ref_steps, initial = _three_steps(device, bsz, fuse=True, switch=False)
    assert all(s == {"deferred": 0, "materialized": 0, "fused_from_sums": 0} for s in ref_steps)  # today's path
    got, steps, _ = _three_steps(device, bsz, fuse=True, switch=True)
    # every view's rounding was left out; the statistics of step 1 had each of its records rounded, and that step's
    # fused launch read the sums all the same (they hold what the record holds)
    assert steps == [{"deferred": bsz, "materialized": 0, "fused_from_sums": bsz},
                     {"deferred": bsz, "materialized": bsz, "fused_from_sums": bsz},
                     {"deferred": bsz, "materialized": 0, "fused_from_sums": bsz}], steps
    unfused, unfused_steps, _ = _three_steps(device, bsz, fuse=False, switch=True)
    assert all(s == {"deferred": 0, "materialized": 0, "fused_from_sums": 0} for s in unfused_steps)  # never armed
    for what, other in (("deferred", got), ("fuse_backward=False", unfused)):
        for j, (a, b) in enumerate(zip(ref, other)):
            assert torch.equal(a, b), f"bsz {bsz}, {what}: tensor {j}: {int((a != b).sum())} of {a.numel()} differ"
    # not vacuous: the three steps moved every one of the six parameters away from its initial value through first
    # moments that are not zero, and the statistics of step 1 accumulated a gradient norm
    for j, n in enumerate(NAMES):
        assert not torch.equal(ref[j], initial[j]), f"{n} did not move"
        assert int((ref[6 + 2 * j] != 0).sum()) > 0 and int((ref[7 + 2 * j] != 0).sum()) > 0, f"{n}: zero moments"
    # (many rows, not a stray one: the 260 tiles of the image each blend at least one row)
    assert int(((ref[0] != initial[0]).any(dim=1)).sum()) >= 260
    assert float(ref[-3].abs().sum()) > 0 and float(ref[-2].sum()) > 0
