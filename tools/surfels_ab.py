"""surfel geometry pass A/B: the fused forward / backward against the two pairs it replaces, in one process, the legs
taking turns after a warm-up, device events around windows of a few hundred ms (tools/distortion_ab.py's method and
shape: 10^6 Gaussians of the synthetic scene, 1920 x 1080, one rank).
    python tools/surfels_ab.py [OUT.json] [--P 1000000] [--rounds 9] [--views 4]

Kernels alone, per view on its own lists (K1, K3-K7, K8 once), whole grid:
    surfels forward / backward          gsr_render_surfels / _backward, every upstream map given, the "ndc" mapping
    features forward / backward         gsr_render_features / _backward at C = 5 with the feature gradient, on the same rows
    distortion forward / backward       gsr_render_distortion / _backward, the "ndc" mapping, on the rows' depths
The rows are (1, K1's depth, a seeded unit normal): the kernels' time does not depend on the normals' values.
`separate_*` is the sum of the two separate legs' medians and `separate_*_spread_ms` the sum of their spreads; the fused
pair is below the separate pairs by more than the separate legs' own spread when `fused_*_saving_ms` exceeds it.
The last line printed is the whole result as one JSON object (also written to OUT.json when given).
Kernel names for a later trace: composite_surfels_kernel, composite_surfels_backward_kernel, surfels_record_kernel."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distortion_ab as DAB  # noqa: E402  (puts the package and tests/ on the path)
import invdepth_ab as AB  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import synthetic_scene as S  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402

W, H, dev, ptr, COEF = AB.W, AB.H, AB.dev, AB.ptr, DAB.COEF


class View(DAB.View):
    def __init__(self, g, cam):
        super().__init__(g, cam)
        P = self.P
        gen = torch.Generator(device=dev).manual_seed(3)
        n = torch.nn.functional.normalize(torch.rand((P, 3), device=dev, generator=gen) - 0.5, dim=1)
        self.rows = torch.cat([torch.ones((P, 1), device=dev), self.depths.reshape(-1, 1), n], dim=1).contiguous()
        self.surfel, self.aux = torch.empty((5, H, W), device=dev), torch.empty((4, H, W), device=dev)
        self.mpos = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.fmap = torch.empty((5, H, W), device=dev)
        self.g5 = torch.rand((5, H, W), device=dev, generator=gen)
        self.rec6, self.drows = torch.empty((P, 6), device=dev), torch.empty((P, 5), device=dev)
        self.acc10 = torch.empty((P, 10), dtype=torch.float64, device=dev)
        self.acc11 = torch.empty((P, 11), dtype=torch.float64, device=dev)

    def _lists(self, per_row):
        return [ptr(t) for t in (self.ranges, self.point_list, self.m2, self.co, per_row, self.mask, self.nc)]

    def surf(self):
        return _lib.lib.gsr_render_surfels(self.P, W, H, *self._lists(self.rows), *COEF, 0, 0, ptr(self.surfel),
                                           ptr(self.aux), ptr(self.mpos), dgr._stream())

    def surf_bwd(self):
        return _lib.lib.gsr_render_surfels_backward(self.P, W, H, *self._lists(self.rows), *COEF, ptr(self.fT),
                                                    ptr(self.surfel), ptr(self.aux), ptr(self.mpos), ptr(self.g5),
                                                    ptr(self.g3[0]), ptr(self.g3[1]), 0, 0, ptr(self.rec6),
                                                    ptr(self.drows), ptr(self.acc10), dgr._stream())

    def feat(self):
        return _lib.lib.gsr_render_features(self.P, 5, W, H, *self._lists(self.rows), 0, 0, ptr(self.fmap), dgr._stream())

    def feat_bwd(self):
        return _lib.lib.gsr_render_features_backward(self.P, 5, W, H, *self._lists(self.rows), ptr(self.fT), ptr(self.g5),
                                                     0, 0, ptr(self.rec6), ptr(self.drows), ptr(self.acc11),
                                                     dgr._stream())


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
    names = ("k8", "surfels_forward", "features5_forward", "distortion_forward", "surfels_backward",
             "features5_backward", "distortion_backward", "k8_again")
    fns = ("k8", "surf", "feat", "dist", "surf_bwd", "feat_bwd", "dist_bwd", "k8")
    for v in views:
        assert all(getattr(v, f)() == 0 for f in fns)
    torch.cuda.synchronize()
    res = {"P": a.P, "width": W, "height": H, "views": a.views, "window_ms": AB.WINDOW_MS, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "pairs_per_view": [int(v.D) for v in views],
           "mean_n_contrib": [round(float(v.nc.float().mean()), 2) for v in views]}
    for name, ts in zip(names, AB.alternate([[getattr(v, f) for v in views] for f in fns], a.rounds)):
        res[name] = AB.stats(ts, a.views)
    for k in ("forward", "backward"):
        sep = res[f"features5_{k}"]["median_ms"] + res[f"distortion_{k}"]["median_ms"]
        res[f"separate_{k}_ms"] = round(sep, 5)
        res[f"separate_{k}_spread_ms"] = round(res[f"features5_{k}"]["spread_ms"] + res[f"distortion_{k}"]["spread_ms"], 5)
        res[f"fused_{k}_saving_ms"] = round(sep - res[f"surfels_{k}"]["median_ms"], 5)
        res[f"ratio_surfels_{k}_over_separate"] = round(res[f"surfels_{k}"]["median_ms"] / sep, 4)
    res["kernel_noise_floor_ms"] = round(max(abs(res["k8_again"]["median_ms"] - res["k8"]["median_ms"]),
                                             res["k8"]["spread_ms"], res["k8_again"]["spread_ms"]), 5)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
