"""anti-aliasing A/B: what gsr_set_antialiasing(1) costs in K1 and in the fused K11 + Adam launch, on the same inputs, in one
process, the launches taking turns after a warm-up, device events around windows of a few hundred ms of launches.
    python tools/antialias_ab.py [OUT.json] [--P 1000000] [--rounds 9] [--log-scale MEAN SPREAD]
                                 [--parent-lib PATH/libgsraster.so]
The c1 shape: 10^6 Gaussians, 1920 x 1080, SH degree 3, one camera.  K1 is gsr_preprocess_forward_raw_batched with B = 1,
K11 + Adam gsr_preprocess_backward_adam_raw_batched with the host tangents (the one-camera kernel), learning rate 0.
Three comparisons, each interleaved, the median of `rounds` (>= 7) windows per launch:
    mode 0 against mode 1            the cost of the switch
    mode 0 against mode 0            the same launch twice in the rotation: the noise floor of this very method
    --parent-lib against mode 0      a libgsraster.so built from the parent commit: "mode 0 is the parent's code", timed
The last line printed is the whole result as one JSON object (also written to OUT.json when given).
Kernel names for a later trace: preprocess_forward_batched_kernel<3, AA>, preprocess_backward_adam_kernel<3, AA>."""
import argparse
import ctypes
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
VP, D6, I64 = ctypes.c_void_p * 6, ctypes.c_double * 6, ctypes.c_int64 * 6
dev = torch.device("cuda:0")  # (a name only: nothing touches the device before main())


def ptr(t):
    return t.data_ptr() if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Scene:
    def __init__(self, P, log_scale):
        g = torch.Generator(device=dev).manual_seed(1)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        xyz = r(P, 3) * torch.tensor([0.8, 0.45, 0.5], device=dev) + torch.tensor([0.0, 0.0, 6.0], device=dev)
        # xyz, scaling, rotation, features_dc, features_rest, opacity.  Log-scales: the default, -8 +- 1.2, is ~0.1 px at
        # depth 6, and the clamp of q = det0 / det sets in near 0.04 px: several per cent of the rows sit on the clamp, mixed
        # into every wave, so mode 1 takes both of its paths (the result records the share).  --log-scale -6.5 1.0 is
        # ~0.4 px: no row on the clamp, every row pays the covariance term
        self.params = [xyz, r(P, 3) * log_scale[1] + log_scale[0], r(P, 4), r(P, 1, 3), r(P, 15, 3) * 0.1, r(P, 1)]
        self.ms = [torch.randn_like(p) * 1e-3 for p in self.params]
        self.vs = [torch.rand_like(p) * 1e-6 + 1e-12 for p in self.params]
        self.P = P
        c = S.orbit_cameras(8, W, H, device=dev)[0]
        rs = dgr.GaussianRasterizationSettings(
            image_height=c.image_height, image_width=c.image_width, tanfovx=math.tan(c.FoVx / 2),
            tanfovy=math.tan(c.FoVy / 2), bg=torch.zeros(3, device=dev), scale_modifier=1.0,
            viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev), sh_degree=DEG,
            campos=c.camera_center.to(dev), prefiltered=False, debug=False)
        self.tanfov0 = (ctypes.c_float * 2)(float(rs.tanfovx), float(rs.tanfovy))
        self.cams = dgr.pack_camera(rs).view(1, 40).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        self.m2, self.depths, self.co, self.rgb = (torch.empty(s, **f32) for s in ((1, P, 2), (1, P), (1, P, 4), (1, P, 3)))
        self.radii = torch.empty((1, P), dtype=torch.int32, device=dev)
        self.cov3D = torch.empty((P, 6), **f32)
        self.clamped = torch.empty((1, P, 3), dtype=torch.uint8, device=dev)
        self.rec = torch.randn((P, 9), device=dev, generator=g) * 1e-3
        self.tabs = (VP(*[ptr(t) for t in self.ms]), VP(*[ptr(t) for t in self.vs]), D6(*[0.0] * 6), D6(*[0.9] * 6),
                     D6(*[0.999] * 6), D6(*[1e-15] * 6), I64(*[1000] * 6))

    def k1(self, lib):
        q = self.params
        args = [self.P, 1, DEG, 16, ptr(q[0]), ptr(q[1]), 1.0, ptr(q[2]), ptr(q[3]), ptr(q[4]), ptr(q[5]), ptr(self.cams),
                W, H, ptr(self.m2), ptr(self.depths), ptr(self.radii), ptr(self.cov3D), ptr(self.co), ptr(self.rgb),
                ptr(self.clamped), stream()]
        return lambda: lib.gsr_preprocess_forward_raw_batched(*args)

    def k11_adam(self, lib):
        q, rec = self.params, self.rec
        args = [self.P, 1, DEG, 16, ptr(q[0]), ptr(q[1]), 1.0, ptr(q[2]), ptr(q[3]), ptr(q[4]), ptr(q[5]), ptr(self.cams),
                W, H, ptr(self.radii), ptr(self.cov3D), ptr(self.clamped), rec.data_ptr(), rec.data_ptr() + 20,
                rec.data_ptr() + 8, 9, *self.tabs, 1.0, self.tanfov0, stream()]
        return lambda: lib.gsr_preprocess_backward_adam_raw_batched(*args)


def window(fn, mode, n):
    """-> ms per launch over n launches between two device events; mode: what this tree's library is switched to first
    (a launch keeps the mode it was enqueued under; the parent's library has no switch and is not touched)"""
    assert _lib.lib.gsr_set_antialiasing(mode) >= 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        code = fn()
    e1.record()
    e1.synchronize()
    assert code == 0, code
    return e0.elapsed_time(e1) / n


def alternate(pairs, rounds):
    """pairs: [(launch, mode)].  Warm up, size the windows to WINDOW_MS, then `rounds` rounds over the launches in turn
    -> [[ms per launch] per pair]"""
    ns = []
    for fn, mode in pairs:
        window(fn, mode, 3)
        ns.append(max(20, min(4000, int(math.ceil(WINDOW_MS / max(window(fn, mode, 10), 1e-3))))))
    out = [[] for _ in pairs]
    for _ in range(rounds):
        for k, (fn, mode) in enumerate(pairs):
            out[k].append(window(fn, mode, ns[k]))
    return out


def stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5),
            "spread_ms": round(s[-1] - s[0], 5)}


def compare(name, a, b, rounds):
    ta, tb = alternate([a, b], rounds)
    sa, sb = stats(ta), stats(tb)
    return {"what": name, "a": sa, "b": sb, "b_minus_a_ms": round(sb["median_ms"] - sa["median_ms"], 5),
            "b_over_a": round(sb["median_ms"] / sa["median_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log-scale", type=float, nargs=2, default=[-8.0, 1.2], metavar=("MEAN", "SPREAD"))
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    lib = _lib.lib
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        assert not hasattr(parent, "gsr_set_antialiasing"), "--parent-lib has the switch: not the parent's library"
        for name in ("gsr_preprocess_forward_raw_batched", "gsr_preprocess_backward_adam_raw_batched"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    sc = Scene(a.P, a.log_scale)
    res = {"P": a.P, "log_scale": a.log_scale, "width": W, "height": H, "sh_degree": DEG, "cameras": 1, "window_ms": WINDOW_MS, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "K1": {}, "K11_adam": {}}
    try:
        assert lib.gsr_set_antialiasing(1) >= 0 and sc.k1(lib)() == 0
        torch.cuda.synchronize()
        vis = sc.radii[0] > 0
        rho = sc.co[0, :, 3][vis] / torch.sigmoid(sc.params[5].view(-1)[vis])
        res["visible_fraction"] = round(float(vis.float().mean()), 4)
        res["clamped_fraction_of_visible"] = round(float((rho <= 0.005 * (1 + 1e-5)).float().mean()), 4)
        for key, make in (("K1", sc.k1), ("K11_adam", sc.k11_adam)):
            fn = make(lib)
            res[key]["mode0_vs_mode1"] = compare("a: mode 0, b: mode 1", (fn, 0), (fn, 1), a.rounds)
            res[key]["noise_floor"] = compare("a: mode 0, b: mode 0 again", (fn, 0), (fn, 0), a.rounds)
            if parent is not None:
                res[key]["parent_vs_mode0"] = compare("a: parent commit's library, b: mode 0", (make(parent), 0), (fn, 0),
                                                      a.rounds)
            floor = max(abs(res[key]["noise_floor"]["b_minus_a_ms"]), res[key]["noise_floor"]["a"]["spread_ms"],
                        res[key]["noise_floor"]["b"]["spread_ms"])
            res[key]["noise_floor_ms"] = round(floor, 5)
            res[key]["mode1_cost_above_floor"] = res[key]["mode0_vs_mode1"]["b_minus_a_ms"] > floor
            if parent is not None:
                res[key]["mode0_within_floor_of_parent"] = abs(res[key]["parent_vs_mode0"]["b_minus_a_ms"]) <= floor
    finally:
        lib.gsr_set_antialiasing(0)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
