"""contribution statistics A/B: what gsr_render_contrib adds to a view, on the same lists, in one process, the launches
taking turns after a warm-up, device events around windows of a few hundred ms of launches.
    python tools/contribution_ab.py [OUT.json] [--P 1000000] [--rounds 9] [--views 4]
The c1 shape: 10^6 Gaussians of the synthetic scene (seed 0), 1920 x 1080, SH degree 3, orbit cameras.  Per view the
lists are built once (K1, K3-K7, K8 for n_contrib); then three launches are timed, interleaved, the median of `rounds`
(>= 7) windows each:
    K8 alone                  gsr_render_forward, whole grid, no segments
    K8 + contribution         the two launches back to back on one stream (what cuda_args["contributions"] costs a view)
    K8 alone, again           the same launch twice in the rotation: the noise floor of this very method
The accumulators are zeroed once and then accumulated into by every timed launch (the atomics' cost does not depend on
the values).  The last line printed is the whole result as one JSON object (also written to OUT.json when given).
Kernel names for a later trace: composite_forward_kernel<false, false>, composite_contrib_kernel."""
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
    """one camera's lists and K8 outputs, and the two launches on them"""

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
        self.P = m2.shape[0]
        gx, gy = (W + 15) // 16, (H + 15) // 16
        self.mask = torch.ones(gx * gy, dtype=torch.uint8, device=dev)
        self.m2, self.co, self.rgb = m2.contiguous(), co.contiguous(), rgb.contiguous()
        self.point_list, self.ranges, self.D = dgr.bin_gaussians(self.m2, depths.contiguous(), radii.contiguous(), self.co,
                                                                 self.mask, W, H)
        self.bg = torch.zeros(3, device=dev)
        self.img = torch.empty((3, H, W), device=dev)
        self.fT = torch.empty((H, W), device=dev)
        self.nc = torch.empty((H, W), dtype=torch.int32, device=dev)
        self.stats = dgr.ContributionStats(self.P, dev)
        self.radii = radii

    def k8(self):
        return _lib.lib.gsr_render_forward(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2), ptr(self.co),
                                           ptr(self.rgb), ptr(self.mask), ptr(self.bg), ptr(self.img), ptr(self.fT),
                                           ptr(self.nc), None, 0, 0, 0, None, 0, dgr._stream())

    def contrib(self):
        s = self.stats
        return _lib.lib.gsr_render_contrib(self.P, W, H, ptr(self.ranges), ptr(self.point_list), ptr(self.m2), ptr(self.co),
                                           ptr(self.mask), ptr(self.nc), 0, 0, ptr(s.hits), ptr(s.wmax), ptr(s.wsum),
                                           dgr._stream())


def window(fns, n):
    """-> ms per pass over the views' launches `fns`, n passes between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    code = 0
    for _ in range(n):
        for fn in fns:
            code |= fn()
    e1.record()
    e1.synchronize()
    assert code == 0, code
    return e0.elapsed_time(e1) / n


def alternate(legs, rounds):
    ns = []
    for fns in legs:
        window(fns, 3)
        ns.append(max(10, min(4000, int(math.ceil(WINDOW_MS / max(window(fns, 5), 1e-3))))))
    out = [[] for _ in legs]
    for _ in range(rounds):
        for k, fns in enumerate(legs):
            out[k].append(window(fns, ns[k]))
    return out


def stats(ts, views):
    s = sorted(t / views for t in ts)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5),
            "spread_ms": round(s[-1] - s[0], 5)}


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
    for v in views:
        assert v.k8() == 0 and v.contrib() == 0
    torch.cuda.synchronize()
    res = {"P": a.P, "width": W, "height": H, "sh_degree": DEG, "views": a.views, "window_ms": WINDOW_MS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "pairs_per_view": [int(v.D) for v in views],
           "rows_with_radii": [int((v.radii > 0).sum()) for v in views],
           "rows_blended": [int((v.stats.hits > 0).sum()) for v in views],
           "mean_n_contrib": [round(float(v.nc.float().mean()), 2) for v in views]}
    for v in views:
        v.stats.zero_()
    k8 = [v.k8 for v in views]
    both = [fn for v in views for fn in (v.k8, v.contrib)]
    only = [v.contrib for v in views]
    t_k8, t_both, t_again, t_only = alternate([k8, both, k8, only], a.rounds)
    res["k8"] = stats(t_k8, a.views)
    res["k8_plus_contrib"] = stats(t_both, a.views)
    res["k8_again"] = stats(t_again, a.views)
    res["contrib_alone"] = stats(t_only, a.views)
    res["ratio_k8_plus_contrib_over_k8"] = round(res["k8_plus_contrib"]["median_ms"] / res["k8"]["median_ms"], 4)
    res["noise_floor_ms"] = round(max(abs(res["k8_again"]["median_ms"] - res["k8"]["median_ms"]), res["k8"]["spread_ms"],
                                      res["k8_again"]["spread_ms"]), 5)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
