"""bilateral-grid A/B: what the per-image colour correction (include/gsraster.h, N1g) costs, measured in one
process, legs interleaved, warmed up, device events around windows of launches.
    python tools/bilagrid_ab.py OUT.json [--variant-lib PATH/libgsraster.so] [--window-ms 100] [--repeats 7]
                                         [--gaussians 1000000] [--step-rounds 12]
Legs, each its own window (1080p, the default 16 x 16 x 8 grid):
  slice_forward                      gsr_bilagrid_slice_forward of the whole image
  slice_backward                     gsr_bilagrid_slice_backward (pieces + finalize)
  variant_slice_backward             the same entry point of --variant-lib: a build with
                                     GSR_DEFINES=-DGSR_ABL_BILAGRID_FIXEDPOINT (integer LDS atomics; EXPERIMENTS.md)
  tv_adam_100 / tv_adam_1000         gsr_bilagrid_tv + gsr_adam_step over 100 / 1 000 cameras' grids
  step_plain / step_grid             the training step (ground-truth staging .. optimizer step; bsz 1, 8 views,
                                     fused K11 + Adam) without and with a BilateralGridModel set, the model's
                                     sync_grads + step included; the plain step runs the parent commit's code
  *_again                            the first legs once more: their ratio to the first visit is the noise floor
The host's enqueue time of every window is recorded: a window whose host time is not well below its device time measures
the launch path, not the kernels."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

from diff_gaussian_rasterization import _lib  # noqa: E402

W, H = 1920, 1080
GW, GH, GL = 16, 16, 8


def load_variant(path):
    lib = ctypes.CDLL(path)
    for name in ("gsr_bilagrid_slice_backward", "gsr_bilagrid_num_partials"):
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Slice:
    def __init__(self, dev):
        g = torch.Generator(device=dev).manual_seed(3)
        self.img = torch.rand((3, H, W), device=dev, generator=g)
        self.gout = torch.randn((3, H, W), device=dev, generator=g) * 1e-6
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12, 1, 1, 1)
        self.grid = (eye + 0.1 * torch.randn((12, GL, GH, GW), generator=torch.Generator().manual_seed(4))).to(dev)
        self.out, self.gimg, self.ggrid = torch.empty_like(self.img), torch.empty_like(self.img), torch.empty_like(self.grid)
        self.partials = torch.empty((_lib.lib.gsr_bilagrid_num_partials(W, H, GW, GH, GL),), device=dev)
        self.s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, lib):
        return lib.gsr_bilagrid_slice_forward(W, H, 0, H, self.img.data_ptr(), H * W, self.grid.data_ptr(), GW, GH, GL,
                                              self.out.data_ptr(), H * W, self.s)

    def backward(self, lib):
        return lib.gsr_bilagrid_slice_backward(W, H, 0, H, self.img.data_ptr(), H * W, self.grid.data_ptr(), GW, GH, GL,
                                               self.gout.data_ptr(), H * W, self.gimg.data_ptr(), H * W,
                                               self.partials.data_ptr(), self.ggrid.data_ptr(), self.s)


class TvAdam:
    def __init__(self, dev, cameras):
        from bilagrid import BilateralGridModel

        self.model = BilateralGridModel(cameras, device=dev)
        self.grad = torch.randn(self.model.grids.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def __call__(self):
        self.model.grids.grad = self.grad  # (step() adds the TV term into it and drops the reference)
        self.model.step()
        return 0


class Step:
    """the eager training step of bench.py's headline workload (same calls in the same order), on one rank"""

    def __init__(self, dev, gaussians):
        import synthetic_scene as S
        import utils.general_utils as utils
        from bilagrid import BilateralGridModel
        from fused_optim import FusedAdam
        from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal

        utils.init_distributed(backend=None)  # one rank: bench.py's start-up
        utils.set_args(utils.default_args(bsz=1))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        self.utils, self.dev = utils, dev
        self.model = S.SyntheticGaussianModel(gaussians, W, H, seed=0, device=dev)
        self.cameras = S.orbit_cameras(8, W, H, device=dev)
        for k, cam in enumerate(self.cameras):
            cam.original_image_backup = S.make_gt_image(W, H, seed=1 + k, device=dev)
        self.history = DivisionStrategyHistoryFinal(S.SyntheticDataset(self.cameras), 1, 0)
        self.bg = torch.zeros(3, dtype=torch.float32, device=dev)
        self.pipe = type("Pipe", (), {"debug": False})()
        self.opt = FusedAdam(self.model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, grad_scale=1.0)
        self.grid = BilateralGridModel(100, device=dev)
        self.it = 0

    def __call__(self, with_grid):
        from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
        from gaussian_renderer import loss_distribution as ld
        from gaussian_renderer.workload_division import finish_strategy_final, start_strategy_final

        utils = self.utils
        cams = [self.cameras[self.it % len(self.cameras)]]
        self.it += 1
        utils.set_cur_iter(utils.get_cur_iter() + 1)
        ld.set_bilateral_grid(self.grid if with_grid else None)
        try:
            strategies, tasks = start_strategy_final(cams, self.history)
            ld.load_camera_from_cpu_to_all_gpu(cams, strategies, tasks)
            pkg = distributed_preprocess3dgs_and_all2all_final(cams, self.model, self.pipe, self.bg,
                                                               batched_strategies=strategies, mode="train")
            images, masks = render_final(pkg, strategies)
            stats = [ca["stats_collector"] for ca in pkg["batched_cuda_args"]]
            loss, _ = ld.batched_loss_computation(images, cams, masks, strategies, stats)
            loss.backward()
            finish_strategy_final(cams, self.history, strategies, stats)
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)
            if with_grid:
                self.grid.sync_grads(utils.DEFAULT_GROUP)
                self.grid.step()
            for cam in cams:
                cam.original_image = None
        finally:
            ld.set_bilateral_grid(None)
        return 0


def window(fns, n):
    """n rounds of the launches in `fns` between two events -> (device ms per round, host ms per round)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        for f in fns:
            if f() != 0:
                raise RuntimeError("a launch was refused")
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, host / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--step-rounds", type=int, default=12, help="training steps per window of the step legs")
    ap.add_argument("--no-step", action="store_true", help="kernel legs only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_ab: no GPU (this measurement has no CPU form)")
    dev = torch.device("cuda:0")
    lib = _lib.lib
    variant = load_variant(a.variant_lib) if a.variant_lib else None
    c = Slice(dev)
    tv100, tv1000 = TvAdam(dev, 100), TvAdam(dev, 1000)
    legs = {
        "slice_forward": [lambda: c.forward(lib)],
        "slice_backward": [lambda: c.backward(lib)],
        "tv_adam_100": [tv100],
        "tv_adam_1000": [tv1000],
        "slice_forward_again": [lambda: c.forward(lib)],
        "slice_backward_again": [lambda: c.backward(lib)],
    }
    if variant is not None:
        assert variant.gsr_bilagrid_num_partials(W, H, GW, GH, GL) == c.partials.numel()
        legs["variant_slice_backward"] = [lambda: c.backward(variant)]
    fixed = {}
    if not a.no_step:
        step = Step(dev, a.gaussians)
        for name, on in (("step_plain", False), ("step_grid", True), ("step_plain_again", False)):
            legs[name] = [lambda on=on: step(on)]
            fixed[name] = a.step_rounds
    counts = {}
    for k, fns in legs.items():  # warm-up (code objects, allocator, first sight of every view) and the rounds of a window
        if k in fixed:
            window(fns, 10)
            counts[k] = fixed[k]
            continue
        window(fns, 20)
        ms, _ = window(fns, 50)
        counts[k] = max(50, int(a.window_ms / max(ms, 1e-4)))
    samples, hosts = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(a.repeats):  # interleaved: every repeat visits every leg once
        for k, fns in legs.items():
            ms, host = window(fns, counts[k])
            samples[k].append(ms)
            hosts[k].append(host)
    rec = {"window_ms": a.window_ms, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "height": H, "width": W,
           "grid": [GW, GH, GL], "gaussians": a.gaussians, "legs": {}}
    for k in legs:
        v = sorted(samples[k])
        rec["legs"][k] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "samples_ms": samples[k],
                          "host_ms_per_round": sorted(hosts[k])[len(v) // 2], "rounds_per_window": counts[k]}
    med = {k: rec["legs"][k]["median_ms"] for k in legs}
    px = H * W
    rec["slice"] = {
        # 3 floats in and 3 out per pixel forward; 6 in and 3 out backward, plus the partial rows written and read once
        "forward_GBps": 24.0 * px / med["slice_forward"] / 1e6,
        "backward_GBps": (36.0 * px + 8.0 * c.partials.numel()) / med["slice_backward"] / 1e6,
        "partials_MB": 4.0 * c.partials.numel() / 1e6,
    }
    rec["noise_floor"] = {"slice_forward_again_over_first": med["slice_forward_again"] / med["slice_forward"],
                          "slice_backward_again_over_first": med["slice_backward_again"] / med["slice_backward"]}
    if variant is not None:
        rec["variant_slice_backward_over_slice_backward"] = med["variant_slice_backward"] / med["slice_backward"]
    if not a.no_step:
        rec["step"] = {"plain_ms": med["step_plain"], "grid_ms": med["step_grid"],
                       "grid_over_plain": med["step_grid"] / med["step_plain"],
                       "added_ms": med["step_grid"] - med["step_plain"],
                       "kernels_ms": med["slice_forward"] + med["slice_backward"] + med["tv_adam_100"]}
        rec["noise_floor"]["step_plain_again_over_first"] = med["step_plain_again"] / med["step_plain"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("legs", json.dumps({k: round(v, 5) for k, v in med.items()}), flush=True)
    print("BILAGRID_AB " + json.dumps({k: rec[k] for k in ("slice", "step", "noise_floor",
                                                           "variant_slice_backward_over_slice_backward") if k in rec}))


if __name__ == "__main__":
    main()
