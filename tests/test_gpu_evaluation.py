"""evaluation.py on the GPU: training_report on one rank (the two log lines against the fp64 restatement of
tests/metric_refs.py on the very images render_final returned), and evaluate_batch on W fake ranks (tests/fake_world.py)
with SSIM on: bit-identical on every rank, inside the tolerance of the fp64 restatement on the one-rank image, with one
all_reduce per batch, at most one strip all_gather per split camera and nothing of image size on the wire.

Tolerance, carried from the sums (tests/test_gpu_metrics_edges.py: K = 8 units per sum, a unit = max(|fp32 torch
restatement - fp64|, 2e-5 |fp64|)) through metrics_from_sums:
  L1   = sum_c S_l1[c] / (C H W)            -> sum_c K unit[c, 0] / (C H W)
  PSNR = mean_c -10 log10(S_sse[c] / (H W)) -> a relative error r of S_sse[c] moves a channel by 10 |log10(1 - r)| dB, so
         10 |log10(1 - max_c K unit[c, 1] / S_sse[c])| dB; with the floor alone r = 8 * 2e-5 = 1.6e-4, i.e. 6.9e-4 dB
  (means over the cameras of a set: the mean of the per-camera bounds)."""
import io
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

N, WD, H = 20_000, 640, 360  # 23 tile rows, the last one partial (8 pixel rows)
f32, f64 = torch.float32, torch.float64


class _Scene:
    def __init__(self, gaussians, train, test):
        self.gaussians, self._train, self._test = gaussians, train, test

    def getTrainCameras(self):
        return self._train

    def getTestCameras(self):
        return self._test


def _cameras(dev, n, first_uid, seed):
    import synthetic_scene as S

    cams = S.orbit_cameras(n, WD, H, device=dev)
    for k, c in enumerate(cams):
        c.uid = first_uid + k
        c.original_image_backup = S.make_gt_image(WD, H, seed=seed + k, device=dev)
    return cams


def _one_rank_globals(bsz=1):
    import gaussian_renderer as gr
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=bsz))
    utils.set_img_size(H, WD)
    utils.set_cur_iter(1)
    gr._PLANNERS.clear()


def _bounds(image, gt, ssim):
    """-> (l1, psnr, ssim) of the fp64 restatement and the bounds (l1, dB, ssim) the docstring derives"""
    import metric_refs as M

    r64 = M.metric_sums(image, gt, 0, H, f64, ssim=ssim)
    r32 = M.metric_sums(image, gt, 0, H, f32, ssim=ssim)
    unit = M.sum_units(r64, r32)
    n = 3.0 * H * WD
    tol = (float(M.K * unit[:, 0].sum() / n), M.psnr_tolerance_db(float((M.K * unit[:, 1] / r64[:, 1]).max())),
           float(M.K * unit[:, 2].sum() / n))
    return M.metrics_of(r64, H, WD), tol, (r64, r32)


def test_training_report_one_rank(device, monkeypatch, capsys):
    import evaluation
    import synthetic_scene as S
    import utils.general_utils as utils

    _one_rank_globals()
    model = S.SyntheticGaussianModel(N, WD, H, seed=5, device=device, scale_coef=0.006)
    test_cams, train_cams = _cameras(device, 4, 100, 20), _cameras(device, 8, 200, 40)
    gts = {c.uid: c.original_image_backup.cpu() for c in test_cams + train_cams}
    scene = _Scene(model, train_cams, test_cams)
    bg = torch.tensor([0.1, 0.2, 0.3], device=device)
    pipe = type("P", (), {"debug": False})()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    log = io.StringIO()
    utils.set_log_file(log)
    seen = []
    real_render = evaluation.render_final

    def recording_render(pkg, strategies, *a, **k):
        images, masks = real_render(pkg, strategies, *a, **k)
        seen.append((pkg["batched_cuda_args"][0]["mode"], [im.detach().clone() for im in images]))
        return images, masks

    monkeypatch.setattr(evaluation, "render_final", recording_render)
    iterations = [1]
    try:
        report = evaluation.training_report(1, iterations, scene, pipe, bg)
        lines = log.getvalue().splitlines()
        again = evaluation.training_report(1, iterations, scene, pipe, bg)
        assert again == {} and iterations == [] and log.getvalue().splitlines() == lines, "a second call must do nothing"
    finally:
        utils.set_log_file(None)
    printed = capsys.readouterr().out
    assert [ln.split(":")[0] for ln in lines] == ["[ITER 1] Evaluating test", "[ITER 1] Evaluating train"]
    assert all(ln in printed for ln in lines) and "[ITER 1] Start Testing" in printed
    assert all(mode == "test" for mode, _ in seen) and len(seen) == 4 + 1
    assert report["test"]["num_cameras"] == 4 and sorted(report["test"]["cameras"]) == [100, 101, 102, 103]
    assert report["train"]["num_cameras"] == 1 and report["train"]["cameras"][0] in range(200, 208)  # max(8 // 8, bsz)
    assert report["test"]["ssim"] is None
    images = [im[0].cpu() for _, im in seen]
    at = 0
    for ln, name in zip(lines, ("test", "train")):
        l1 = float(ln.split("L1 ")[1].split(" PSNR")[0])  # examples/mip360/analyze_results.py:59-64 of the reference
        psnr = float(ln.split("PSNR ")[1])
        assert l1 == report[name]["l1"] and psnr == report[name]["psnr"]
        uids = report[name]["cameras"]
        want = [_bounds(images[at + k], gts[uid], ssim=False) for k, uid in enumerate(uids)]
        at += len(uids)
        w_l1, w_psnr = (sum(w[0][j] for w in want) / len(want) for j in (0, 1))
        t_l1, t_db = (sum(w[1][j] for w in want) / len(want) for j in (0, 1))
        print(f"training_report {name}: L1 {l1!r} (fp64 {w_l1!r}, bound {t_l1:.3g}), PSNR {psnr!r} dB (fp64 {w_psnr!r}, "
              f"bound {t_db:.3g} dB)")
        assert abs(l1 - w_l1) <= t_l1 and abs(psnr - w_psnr) <= t_db
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]) and p.grad is None, f"{n} was touched by the evaluation"
    for c in test_cams + train_cams:  # the staged ground truth is released, as the reference does
        if c.uid in report["test"]["cameras"] + report["train"]["cameras"]:
            assert c.original_image is None


def _single_rank_images(dev, cams_idx, n_views):
    """the whole scene on one rank: the full image of each camera, rendered in mode="test" """
    import synthetic_scene as S
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    _one_rank_globals()
    model = S.SyntheticGaussianModel(N, WD, H, seed=5, device=dev, scale_coef=0.006)
    cams = _cameras(dev, n_views, 100, 20)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    out = []
    with torch.no_grad():
        for i in cams_idx:
            st, _ = start_strategy_final([cams[i]], hist)
            pkg = distributed_preprocess3dgs_and_all2all_final([cams[i]], model, pipe, bg, batched_strategies=st,
                                                               mode="test")
            out.append(render_final(pkg, st)[0][0].detach().clone())
    return out, [cams[i].original_image_backup for i in cams_idx]


def _run_world(dev, world, bsz, stand_in_rank=None):
    import torch.distributed as dist

    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import synthetic_scene as S
    import utils.general_utils as utils
    from evaluation import evaluate_batch
    from fake_world import FakeWorld
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.loss_distribution import load_camera_from_cpu_to_all_gpu_for_eval
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    fw = FakeWorld(world, dev)
    gr._PLANNERS.clear()
    wire = []  # (collective, bytes rank 0 hands to it) during evaluate_batch

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, world
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        utils.set_args(utils.default_args(bsz=bsz, no_heuristics_update=True))
        utils.set_img_size(H, WD)
        utils.set_cur_iter(1)
        wd._BALANCE["mode"] = "exact"
        for k in gr.exchange_stats:
            gr.exchange_stats[k] = 0
        model = S.SyntheticGaussianModel(N, WD, H, seed=5, rank=rank, world_size=world, device=dev, scale_coef=0.006)
        cams = _cameras(dev, 4, 100, 20)
        hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), world, rank)
        bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
        pipe = type("P", (), {"debug": False})()
        batch = cams[:bsz]
        with torch.no_grad():
            strategies, tasks = start_strategy_final(batch, hist)
            load_camera_from_cpu_to_all_gpu_for_eval(batch, strategies, tasks)
            pkg = distributed_preprocess3dgs_and_all2all_final(batch, model, pipe, bg, batched_strategies=strategies,
                                                               mode="test")
            images, _ = render_final(pkg, strategies)
            rendered = [None if (im is None or im.dim() != 3) else im.detach().clone() for im in images]
            if rank == stand_in_rank:
                images = [None if im is None else torch.zeros((), device=dev) for im in images]
            first = len(fw.log)
            if rank == 0:  # what the stand-in collectives are handed while rank 0 is inside evaluate_batch
                real = {n: getattr(dist, n) for n in ("all_reduce", "all_gather_into_tensor")}

                def note(name):
                    def f(*a, **k):
                        if fw.current == 0:
                            t = a[0] if name == "all_reduce" else a[1]
                            wire.append((name, t.numel() * t.element_size()))
                        return real[name](*a, **k)
                    return f

                for n in real:
                    setattr(dist, n, note(n))
            try:
                sums = evaluate_batch(images, batch, strategies, ssim=True)
            finally:
                if rank == 0:
                    for n, fn in real.items():
                        setattr(dist, n, fn)
            mine = [tag for _, tag in fw.log[first:]] if rank == 0 else None
        return dict(sums=sums.clone(), rendered=rendered, log=mine,
                    partitions=[(list(s.gpu_ids), list(s.division_pos)) for s in strategies])

    return fw.run(rank_main, timeout=120), wire


@pytest.mark.parametrize("world,bsz,stand_in", [(2, 1, None), (3, 1, None), (4, 1, None), (2, 2, None), (2, 1, 1)])
def test_evaluate_batch_on_fake_ranks(device, world, bsz, stand_in):
    import metric_refs as M

    res, wire = _run_world(device, world, bsz, stand_in_rank=stand_in)
    partitions = res[0]["partitions"]
    assert all(r["partitions"] == partitions for r in res)
    for r in res[1:]:
        assert torch.equal(r["sums"].view(torch.int64), res[0]["sums"].view(torch.int64)), "the ranks disagree in bits"
    full, gts = _single_rank_images(device, list(range(bsz)), 4)
    split = sum(1 for gpu_ids, _ in partitions if len(gpu_ids) > 1)
    assert split == (bsz if bsz < world else 0)
    for k, (gpu_ids, div) in enumerate(partitions):
        image = full[k].clone()
        for j, g in enumerate(gpu_ids):  # the band renders assemble to the one-rank image bitwise
            y0, y1 = div[j] * 16, min(div[j + 1] * 16, H)
            assert torch.equal(res[g]["rendered"][k][:, y0:y1], full[k][:, y0:y1]), f"camera {k}, band of rank {g}"
            if g == stand_in:
                image[:, y0:y1] = 0.0  # the 0-dim stand-in: that band is scored as zeros, as in the reference's sum
        r64 = M.metric_sums(image.cpu(), gts[k].cpu(), 0, H, f64)
        r32 = M.metric_sums(image.cpu(), gts[k].cpu(), 0, H, f32)
        M.check_sums(res[0]["sums"][k], r64, r32, f"fake world W={world} bsz={bsz} stand_in={stand_in} camera {k}")
    # the wire: one all_reduce of the [B, C, 3] doubles per batch, one strip gather per split camera, no image
    tags = [t for t in res[0]["log"] if not t.endswith("/read")]
    assert tags.count("all_reduce") == 1 and tags.count("all_gather_into_tensor") == split
    assert set(tags) <= {"all_reduce", "all_gather_into_tensor"}, tags
    image_bytes = 3 * H * WD * 4
    assert sorted(wire) == sorted([("all_reduce", bsz * 3 * 3 * 8)] + [("all_gather_into_tensor", 2 * 3 * 5 * WD * 4)] * split)
    assert all(b * world < image_bytes / 4 for _, b in wire)
