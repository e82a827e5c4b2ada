"""absolute-gradient A/B: what the AbsGS densification signal adds to a training step, and what its kernel costs beside
K10, in one process, the legs taking turns after a warm-up, device events around windows of a few hundred ms.
    python tools/absgrad_ab.py [OUT.json] [--P 1000000] [--rounds 9] [--views 4] [--kernels-only]
The c1 shape: 10^6 Gaussians of the synthetic scene (seed 0), 1920 x 1080, SH degree 3, orbit cameras, one rank.

Training step (the product's calls: projection, render_final, fused L1 + SSIM loss, backward,
densification_ops.update_densification_stats, FusedAdam(fuse_backward=True) -- learning rates 0 so that every window
sees the same scene), the views in rotation:
    step                      gaussian_renderer.set_absgrad(False), update_densification_stats(model, means2D, radii)
    step + absgrad            set_absgrad(True), update_densification_stats(..., absgrad=collect_absgrad(...)[0])
    step, again               the first leg twice in the rotation: the noise floor of this very method
Kernels alone, per view on its own lists (K1, K3-K7, K8 once), whole grid:
    K10      gsr_render_backward (fill + walk + rounding pass)
    absgrad  gsr_render_absgrad (fill + walk + rounding pass)
    invdepth gsr_render_invdepth_backward: the kernel this one has the shape of
The last line printed is the whole result as one JSON object (also written to OUT.json when given).
Kernel names for a later trace: composite_absgrad_kernel, absgrad_round_kernel."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import synthetic_scene as S  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402

W, H, DEG = 1920, 1080, 3
WINDOW_MS = 200.0
dev = torch.device("cuda:0")  # (a name only: nothing touches the device before main())


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class View:
    """one camera's lists and K8 outputs, and the launches on them"""

    def __init__(self, g, cam):
        rs = dgr.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2),
            bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev),
            projmatrix=cam.full_proj_transform.to(dev), sh_degree=DEG, campos=cam.camera_center.to(dev),
            prefiltered=False, debug=False)
        rast = dgr.GaussianRasterizer(rs)
        with torch.no_grad():
            m2, rgb, co, radii, depths = rast.preprocess_gaussians(g["means3D"], g["scales"], g["rotations"], g["shs"],
                                                                   g["opacities"], {})
        self.P = P = m2.shape[0]
        gx, gy = (W + 15) // 16, (H + 15) // 16
        self.mask = torch.ones(gx * gy, dtype=torch.uint8, device=dev)
        self.m2, self.co, self.rgb, self.depths = m2.contiguous(), co.contiguous(), rgb.contiguous(), depths.contiguous()
        self.point_list, self.ranges, self.D = dgr.bin_gaussians(self.m2, self.depths, radii.contiguous(), self.co,
                                                                 self.mask, W, H)
        self.bg = torch.zeros(3, device=dev)
        self.img = torch.empty((3, H, W), device=dev)
        self.fT = torch.empty((H, W), device=dev)
        self.nc = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.inv = torch.empty((H, W), device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        self.g3 = torch.rand((3, H, W), device=dev, generator=gen)
        self.rec9, self.acc9 = torch.empty((P, 9), device=dev), torch.empty((P, 9), dtype=torch.float64, device=dev)
        self.rec7, self.acc7 = torch.empty((P, 7), device=dev), torch.empty((P, 7), dtype=torch.float64, device=dev)
        self.abs2, self.acc2 = torch.empty((P, 2), device=dev), torch.empty((P, 2), dtype=torch.float64, device=dev)

    def k8(self):
        return _lib.lib.gsr_render_forward(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2), ptr(self.co),
                                           ptr(self.rgb), ptr(self.mask), ptr(self.bg), ptr(self.img), ptr(self.fT),
                                           ptr(self.nc), None, 0, 0, 0, None, 0, dgr._stream())

    def k10(self):
        return _lib.lib.gsr_render_backward(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2),
                                            ptr(self.co), ptr(self.rgb), ptr(self.mask), ptr(self.bg), ptr(self.fT),
                                            ptr(self.nc), ptr(self.g3), ptr(self.rec9), None, None, 0, 0, 0, 0,
                                            ptr(self.acc9), None, dgr._stream())

    def map(self):
        return _lib.lib.gsr_render_invdepth(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2),
                                            ptr(self.co), ptr(self.depths), ptr(self.mask), ptr(self.nc), 0, 0,
                                            ptr(self.inv), dgr._stream())

    def absgrad(self):
        return _lib.lib.gsr_render_absgrad(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2),
                                           ptr(self.co), ptr(self.rgb), ptr(self.mask), ptr(self.bg), ptr(self.fT),
                                           ptr(self.nc), ptr(self.g3), 0, 0, ptr(self.abs2), ptr(self.acc2),
                                           dgr._stream())

    def map_bwd(self):
        return _lib.lib.gsr_render_invdepth_backward(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2),
                                                     ptr(self.co), ptr(self.depths), ptr(self.mask), ptr(self.nc),
                                                     ptr(self.fT), ptr(self.inv), ptr(self.g3), 0, 0, ptr(self.rec7),
                                                     ptr(self.acc7), dgr._stream())


def window(fns, n):
    """-> ms per pass over `fns`, n passes between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    code = 0
    for _ in range(n):
        for fn in fns:
            code |= fn() or 0
    e1.record()
    e1.synchronize()
    assert code == 0, code
    return e0.elapsed_time(e1) / n


def alternate(legs, rounds):
    ns = []
    for fns in legs:
        window(fns, 3)
        ns.append(max(3, min(4000, int(math.ceil(WINDOW_MS / max(window(fns, 5), 1e-3))))))
    out = [[] for _ in legs]
    for _ in range(rounds):
        for k, fns in enumerate(legs):
            out[k].append(window(fns, ns[k]))
    return out


def stats(ts, views):
    s = sorted(t / views for t in ts)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5),
            "spread_ms": round(s[-1] - s[0], 5)}


class Trainer:
    """the product's training step on one rank, one camera per step"""

    def __init__(self, P, n_views):
        import gaussian_renderer as gr
        import utils.general_utils as utils
        from fused_optim import FusedAdam
        from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal

        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
        utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        self.gr, self.utils = gr, utils
        self.model = S.SyntheticGaussianModel(P, W, H, seed=0, sh_degree=DEG, device=dev)
        self.cams = S.orbit_cameras(n_views, W, H, device=dev)
        for k, c in enumerate(self.cams):
            c.original_image_backup = S.make_gt_image(W, H, seed=20 + k, device=dev)
        self.hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(self.cams), 1, 0)
        groups = self.model.param_groups()
        for g in groups:
            g["lr"] = 0.0
        self.opt = FusedAdam(groups, lr=0.0, eps=1e-15, fuse_backward=True)
        n = self.model._xyz.shape[0]
        self.model.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.model.denom = torch.zeros((n, 1), device=dev)
        self.model.max_radii2D = torch.zeros((n,), device=dev)
        self.bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
        self.pipe = type("P", (), {"debug": False})()
        self.turn = 0

    def step(self, with_absgrad):
        import densification_ops as D
        from gaussian_renderer import collect_absgrad, distributed_preprocess3dgs_and_all2all_final, render_final
        from gaussian_renderer.loss_distribution import batched_loss_computation, load_camera_from_cpu_to_all_gpu
        from gaussian_renderer.workload_division import start_strategy_final

        self.gr.set_absgrad(with_absgrad)
        batch = [self.cams[self.turn % len(self.cams)]]
        self.turn += 1
        strategies, tasks = start_strategy_final(batch, self.hist)
        load_camera_from_cpu_to_all_gpu(batch, strategies, tasks)
        pkg = distributed_preprocess3dgs_and_all2all_final(batch, self.model, self.pipe, self.bg,
                                                           batched_strategies=strategies, mode="train")
        images, masks = render_final(pkg, strategies)
        loss, _ = batched_loss_computation(images, batch, masks, strategies,
                                           [ca["stats_collector"] for ca in pkg["batched_cuda_args"]])
        loss.backward()
        with torch.no_grad():
            D.update_densification_stats(self.model, pkg["batched_locally_preprocessed_mean2D"][0],
                                         pkg["batched_locally_preprocessed_radii"][0],
                                         absgrad=collect_absgrad(pkg, strategies)[0] if with_absgrad else None)
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true", help="skip the training-step legs")
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    g = {k: v.to(dev) for k, v in S.make_gaussians(a.P, W, H, seed=0).items()}
    views = [View(g, cam) for cam in S.orbit_cameras(a.views, W, H)]
    for v in views:
        assert v.k8() == 0 and v.k10() == 0 and v.map() == 0 and v.map_bwd() == 0 and v.absgrad() == 0
    torch.cuda.synchronize()
    res = {"P": a.P, "width": W, "height": H, "sh_degree": DEG, "views": a.views, "window_ms": WINDOW_MS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "pairs_per_view": [int(v.D) for v in views],
           "rows_with_absgrad": [int((v.abs2 != 0).any(dim=1).sum()) for v in views],
           "sum_absgrad_over_sum_abs_signed": [round(float(v.abs2.double().sum() / v.rec9[:, :2].double().abs().sum()), 3)
                                               for v in views],
           "mean_n_contrib": [round(float(v.nc.float().mean()), 2) for v in views]}
    legs = [[v.k10 for v in views], [v.absgrad for v in views], [v.map_bwd for v in views], [v.k10 for v in views]]
    t = alternate(legs, a.rounds)
    for name, ts in zip(("k10", "absgrad", "invdepth_backward", "k10_again"), t):
        res[name] = stats(ts, a.views)
    res["ratio_absgrad_over_k10"] = round(res["absgrad"]["median_ms"] / res["k10"]["median_ms"], 4)
    res["ratio_absgrad_over_invdepth_backward"] = round(res["absgrad"]["median_ms"] /
                                                        res["invdepth_backward"]["median_ms"], 4)
    res["kernel_noise_floor_ms"] = round(max(abs(res["k10_again"]["median_ms"] - res["k10"]["median_ms"]),
                                             res["k10"]["spread_ms"], res["k10_again"]["spread_ms"]), 5)
    res["library"] = os.path.basename(_lib.LIB_PATH)
    if a.kernels_only:  # (an ablation build named by GSRASTER_LIB: the step's legs say nothing there)
        if a.out:
            with open(a.out, "w") as fo:
                json.dump(res, fo, indent=1)
        print(json.dumps(res))
        return
    del views, g
    torch.cuda.empty_cache()
    tr = Trainer(a.P, a.views)
    off, on = [lambda: tr.step(False)], [lambda: tr.step(True)]
    t_off, t_on, t_again = alternate([off, on, off], a.rounds)
    tr.gr.set_absgrad(False)
    tr.opt.set_fuse_backward(False)
    res["step"] = stats(t_off, 1)
    res["step_with_absgrad"] = stats(t_on, 1)
    res["step_again"] = stats(t_again, 1)
    res["ratio_step_with_absgrad_over_step"] = round(res["step_with_absgrad"]["median_ms"] / res["step"]["median_ms"], 4)
    res["step_noise_floor_ms"] = round(max(abs(res["step_again"]["median_ms"] - res["step"]["median_ms"]),
                                           res["step"]["spread_ms"], res["step_again"]["spread_ms"]), 5)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
