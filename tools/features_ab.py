"""N-channel feature map A/B: what gsr_render_features and gsr_render_features_backward cost beside K8 and K10 and beside
the inverse-depth pair, in one process, the legs taking turns after a warm-up, device events around windows of a few
hundred ms (tools/invdepth_ab.py's method, whose View, windows and statistics are reused).
    python tools/features_ab.py [OUT.json] [--P 1000000] [--rounds 7] [--views 4] [--channels 1,3,16,64]
The c1 shape: 10^6 Gaussians of the synthetic scene (seed 0), 1920 x 1080, SH degree 3, orbit cameras, one rank.
Kernels alone, per view on its own lists (K1, K3-K7, K8 once), whole grid:
    K8   gsr_render_forward          invdepth      gsr_render_invdepth            features C      gsr_render_features
    K10  gsr_render_backward         invdepth bwd  gsr_render_invdepth_backward   features C bwd  gsr_render_features_backward
                                                                                 (with dL_dfeatures, and with NULL)
K8 runs twice in the rotation: the noise floor of this very method.  No gate: the figures are written down.
The last line printed is the whole result as one JSON object (also written to OUT.json when given; the project keeps
profiles/features_ab.json).  Kernel names for a later trace: composite_features_kernel<1|4>,
composite_features_backward_kernel<1|4, true|false>, features_record_kernel."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import synthetic_scene as S  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from invdepth_ab import H, W, DEG, WINDOW_MS, View, alternate, dev, ptr, stats  # noqa: E402


class Channels:
    """the feature rows, dL/dout and the outputs of one channel count, shared by the views (they run in turn)"""

    def __init__(self, P, C):
        gen = torch.Generator(device=dev).manual_seed(3 + C)
        self.C = C
        self.feat = torch.rand((P, C), device=dev, generator=gen)
        self.g = torch.rand((C, H, W), device=dev, generator=gen)
        self.out = torch.empty((C, H, W), device=dev)
        self.rec = torch.empty((P, 6), device=dev)
        self.dfeat = torch.empty((P, C), device=dev)
        self.acc = torch.empty((P, 6 + C), dtype=torch.float64, device=dev)

    def forward(self, v):
        return _lib.lib.gsr_render_features(v.P, self.C, W, H, ptr(v.ranges), ptr(v.point_list), ptr(v.m2), ptr(v.co),
                                            ptr(self.feat), ptr(v.mask), ptr(v.nc), 0, 0, ptr(self.out), dgr._stream())

    def backward(self, v, feature_grad):
        return _lib.lib.gsr_render_features_backward(v.P, self.C, W, H, ptr(v.ranges), ptr(v.point_list), ptr(v.m2),
                                                     ptr(v.co), ptr(self.feat), ptr(v.mask), ptr(v.nc), ptr(v.fT),
                                                     ptr(self.g), 0, 0, ptr(self.rec),
                                                     ptr(self.dfeat) if feature_grad else None, ptr(self.acc),
                                                     dgr._stream())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--channels", default="1,3,16,64")
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    chans = [int(c) for c in a.channels.split(",")]
    g = {k: v.to(dev) for k, v in S.make_gaussians(a.P, W, H, seed=0).items()}
    views = [View(g, cam) for cam in S.orbit_cameras(a.views, W, H)]
    sets = [Channels(views[0].P, C) for C in chans]
    for v in views:
        assert v.k8() == 0 and v.k10() == 0 and v.map() == 0 and v.map_bwd() == 0
        for s in sets:
            assert s.forward(v) == 0 and s.backward(v, True) == 0 and s.backward(v, False) == 0
    torch.cuda.synchronize()
    res = {"P": a.P, "width": W, "height": H, "sh_degree": DEG, "views": a.views, "window_ms": WINDOW_MS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "channels": chans,
           "chunk": 16, "pairs_per_view": [int(v.D) for v in views],
           "mean_n_contrib": [round(float(v.nc.float().mean()), 2) for v in views]}
    names = ["k8", "invdepth_forward"] + [f"features_forward_C{s.C}" for s in sets] + ["k10", "invdepth_backward"] + \
        [f"features_backward_C{s.C}" for s in sets] + [f"features_backward_nograd_C{s.C}" for s in sets] + ["k8_again"]
    legs = [[v.k8 for v in views], [v.map for v in views]] + \
        [[(lambda v=v, s=s: s.forward(v)) for v in views] for s in sets] + \
        [[v.k10 for v in views], [v.map_bwd for v in views]] + \
        [[(lambda v=v, s=s: s.backward(v, True)) for v in views] for s in sets] + \
        [[(lambda v=v, s=s: s.backward(v, False)) for v in views] for s in sets] + [[v.k8 for v in views]]
    t = alternate(legs, a.rounds)
    for name, ts in zip(names, t):
        res[name] = stats(ts, a.views)
    k8, k10 = res["k8"]["median_ms"], res["k10"]["median_ms"]
    res["ratio_invdepth_forward_over_k8"] = round(res["invdepth_forward"]["median_ms"] / k8, 4)
    res["ratio_invdepth_backward_over_k10"] = round(res["invdepth_backward"]["median_ms"] / k10, 4)
    for s in sets:
        res[f"ratio_features_forward_C{s.C}_over_k8"] = round(res[f"features_forward_C{s.C}"]["median_ms"] / k8, 4)
        res[f"ratio_features_backward_C{s.C}_over_k10"] = round(res[f"features_backward_C{s.C}"]["median_ms"] / k10, 4)
        res[f"ratio_features_backward_nograd_C{s.C}_over_k10"] = \
            round(res[f"features_backward_nograd_C{s.C}"]["median_ms"] / k10, 4)
    res["kernel_noise_floor_ms"] = round(max(abs(res["k8_again"]["median_ms"] - k8), res["k8"]["spread_ms"],
                                             res["k8_again"]["spread_ms"]), 5)
    res["library"] = os.path.basename(_lib.LIB_PATH)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
