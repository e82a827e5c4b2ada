"""depth distortion A/B: what its two kernels cost beside K8 / K10 and beside the inverse-depth pair, in one process, the
legs taking turns after a warm-up, device events around windows of a few hundred ms (tools/invdepth_ab.py's method and
shape: 10^6 Gaussians of the synthetic scene, 1920 x 1080, one rank).
    python tools/distortion_ab.py [OUT.json] [--P 1000000] [--rounds 9] [--views 4]

Kernels alone, per view on its own lists (K1, K3-K7, K8 once), whole grid:
    K8, K10                             gsr_render_forward / gsr_render_backward
    invdepth forward / backward         gsr_render_invdepth (fill + walk) / _backward (fill + walk + rounding pass)
    distortion forward / backward       gsr_render_distortion / _backward, the default "ndc" mapping
The last line printed is the whole result as one JSON object (also written to OUT.json when given).
Kernel names for a later trace: composite_distortion_kernel, composite_distortion_backward_kernel,
distortion_record_kernel."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import invdepth_ab as AB  # noqa: E402  (puts the package and tests/ on the path)
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import synthetic_scene as S  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402

W, H, dev, ptr = AB.W, AB.H, AB.dev, AB.ptr
NEAR, FAR = 0.2, 1000.0
COEF = (FAR / (FAR - NEAR), 0.0, -FAR * NEAR / (FAR - NEAR))  # 2DGS's NDC mapping (include/gsraster.h)


class View(AB.View):
    def __init__(self, g, cam):
        super().__init__(g, cam)
        self.maps = torch.empty((4, H, W), device=dev)

    def _args(self):
        return [self.P, W, H] + [ptr(t) for t in (self.ranges, self.point_list, self.m2, self.co, self.depths, self.mask,
                                                   self.nc)] + list(COEF)

    def dist(self):
        return _lib.lib.gsr_render_distortion(*self._args(), 0, 0, ptr(self.maps), dgr._stream())

    def dist_bwd(self):
        return _lib.lib.gsr_render_distortion_backward(*self._args(), ptr(self.fT), ptr(self.maps), ptr(self.g3), 0, 0,
                                                       ptr(self.rec7), ptr(self.acc7), dgr._stream())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--views", type=int, default=4)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    g = {k: v.to(dev) for k, v in S.make_gaussians(a.P, W, H, seed=0).items()}
    views = [View(g, cam) for cam in S.orbit_cameras(a.views, W, H)]
    names = ("k8", "invdepth_forward", "distortion_forward", "k10", "invdepth_backward", "distortion_backward", "k8_again")
    fns = ("k8", "map", "dist", "k10", "map_bwd", "dist_bwd", "k8")
    for v in views:
        assert all(getattr(v, f)() == 0 for f in fns)
    torch.cuda.synchronize()
    res = {"P": a.P, "width": W, "height": H, "views": a.views, "window_ms": AB.WINDOW_MS, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "pairs_per_view": [int(v.D) for v in views],
           "mean_n_contrib": [round(float(v.nc.float().mean()), 2) for v in views]}
    for name, ts in zip(names, AB.alternate([[getattr(v, f) for v in views] for f in fns], a.rounds)):
        res[name] = AB.stats(ts, a.views)
    for k, base in (("forward", "k8"), ("backward", "k10")):
        res[f"ratio_distortion_{k}_over_invdepth_{k}"] = round(res[f"distortion_{k}"]["median_ms"] /
                                                               res[f"invdepth_{k}"]["median_ms"], 4)
        res[f"ratio_distortion_{k}_over_{base}"] = round(res[f"distortion_{k}"]["median_ms"] / res[base]["median_ms"], 4)
    res["kernel_noise_floor_ms"] = round(max(abs(res["k8_again"]["median_ms"] - res["k8"]["median_ms"]),
                                             res["k8"]["spread_ms"], res["k8_again"]["spread_ms"]), 5)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
