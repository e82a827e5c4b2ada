"""sparse Adam A/B: the sparse (lazy) fused K11 + Adam launch against the dense fused launch on the same inputs, same
process, alternating, warmed up, device events around windows of a few hundred ms of launches.
    python tools/sparse_adam_ab.py OUT.json [--P 1000000 6000000] [--B 1 4] [--parent-lib PATH/libgsraster.so]
SH degree 3; active fractions 1.0, 0.5, 0.25, 0.1, 0.03; the active rows once drawn at random and once as contiguous
runs.  Every row of the scene is in front of every camera, so the active fraction is the share of rows with a non-zero
gradient record (the count the launch itself reports is written next to it).  --parent-lib: a libgsraster.so built from
the parent commit; its dense launch is timed against this tree's, alternating, for "dense launch unchanged".
Kernel names for a later trace: sparse_adam_reset_kernel, sparse_adam_classify_kernel, sparse_adam_update_kernel;
dense: preprocess_backward_adam_kernel (one camera) / preprocess_backward_adam_batched_kernel."""
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
FRACTIONS = (1.0, 0.5, 0.25, 0.1, 0.03)
RUN = 4096  # rows per contiguous run of the "runs" layout
WINDOW_MS, REPEATS = 250.0, 5
VP, D6, I64 = ctypes.c_void_p * 6, ctypes.c_double * 6, ctypes.c_int64 * 6
dev = torch.device("cuda:0")  # (a name only: nothing touches the device before main())


def ptr(t):
    return t.data_ptr() if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dense_bytes(P, B):
    """bench.py's algorithmic bytes of the dense fused launch: K11's reads, moments read, parameters / moments written"""
    return P * (236 + 80 * B + 5 * 236)


def sparse_bytes(P, B, visible_pairs, active):
    """radii of every (camera, row), the record row of every visible pair; per active row the list word, 236 B of
    parameters and 24 B of cov3D read, 43 B per camera (radius, record row, clamp flags), 236 B written, both moments
    read and written"""
    return 4 * P * B + 36 * visible_pairs + active * (4 + 236 + 24 + 43 * B + 236 + 4 * 236)


class Scene:
    def __init__(self, P, B):
        g = torch.Generator(device=dev).manual_seed(1)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        xyz = r(P, 3) * torch.tensor([0.8, 0.45, 0.5], device=dev) + torch.tensor([0.0, 0.0, 6.0], device=dev)
        # xyz, scaling, rotation, features_dc, features_rest, opacity
        self.params = [xyz, r(P, 3) * 0.3 - 4.5, r(P, 4), r(P, 1, 3), r(P, 15, 3) * 0.1, r(P, 1)]
        self.ms = [torch.randn_like(p) * 1e-3 for p in self.params]
        self.vs = [torch.rand_like(p) * 1e-6 + 1e-12 for p in self.params]
        self.P, self.B = P, B
        cams = S.orbit_cameras(8, W, H, device=dev)[:B]
        rs = [dgr.GaussianRasterizationSettings(
            image_height=c.image_height, image_width=c.image_width, tanfovx=math.tan(c.FoVx / 2),
            tanfovy=math.tan(c.FoVy / 2), bg=torch.zeros(3, device=dev), scale_modifier=1.0,
            viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev), sh_degree=DEG,
            campos=c.camera_center.to(dev), prefiltered=False, debug=False) for c in cams]
        self.tanfov0 = (ctypes.c_float * 2)(float(rs[0].tanfovx), float(rs[0].tanfovy))
        self.cams = torch.stack([dgr.pack_camera(s) for s in rs]).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        m2, depths, co, rgb = (torch.empty(s, **f32) for s in ((B, P, 2), (B, P), (B, P, 4), (B, P, 3)))
        self.radii = torch.empty((B, P), dtype=torch.int32, device=dev)
        self.cov3D = torch.empty((P, 6), **f32)
        self.clamped = torch.empty((B, P, 3), dtype=torch.uint8, device=dev)
        q = self.params
        _lib.check(_lib.lib.gsr_preprocess_forward_raw_batched(
            P, B, DEG, 16, ptr(q[0]), ptr(q[1]), 1.0, ptr(q[2]), ptr(q[3]), ptr(q[4]), ptr(q[5]), ptr(self.cams), W, H,
            ptr(m2), ptr(depths), ptr(self.radii), ptr(self.cov3D), ptr(co), ptr(rgb), ptr(self.clamped), stream()),
            "forward")
        self.visible = self.radii > 0
        self.full = torch.randn((B, P, 9), device=dev, generator=g) * 1e-3
        self.rec = torch.empty((B * P, 9), **f32)
        need = int(_lib.lib.gsr_sparse_step_workspace_bytes(P))
        self.ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        self.num = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tabs = (VP(*[ptr(t) for t in self.ms]), VP(*[ptr(t) for t in self.vs]), D6(*[0.0] * 6), D6(*[0.9] * 6),
                     D6(*[0.999] * 6), D6(*[1e-15] * 6), I64(*[1000] * 6))

    def set_active(self, fraction, layout):
        """-> (rows with a non-zero record, visible pairs)"""
        P, g = self.P, torch.Generator(device=dev).manual_seed(7)
        if fraction >= 1.0:
            keep = torch.ones(P, dtype=torch.bool, device=dev)
        elif layout == "random":
            keep = torch.rand(P, device=dev, generator=g) < fraction
        else:  # contiguous runs of RUN rows, a share `fraction` of the runs
            nrun = (P + RUN - 1) // RUN
            runs = torch.rand(nrun, device=dev, generator=g) < fraction
            keep = runs.repeat_interleave(RUN)[:P]
        self.rec.view(self.B, P, 9).copy_(self.full * keep.view(1, P, 1))
        return int((keep & self.visible.any(0)).sum()), int(self.visible.sum())

    def common(self):
        q, rec = self.params, self.rec
        return [self.P, self.B, DEG, 16, ptr(q[0]), ptr(q[1]), 1.0, ptr(q[2]), ptr(q[3]), ptr(q[4]), ptr(q[5]),
                ptr(self.cams), W, H, ptr(self.radii), ptr(self.cov3D), ptr(self.clamped), rec.data_ptr(),
                rec.data_ptr() + 20, rec.data_ptr() + 8, 9, *self.tabs, 1.0]

    def dense(self, lib):
        args = self.common() + [self.tanfov0 if self.B == 1 else None, stream()]
        return lambda: lib.gsr_preprocess_backward_adam_raw_batched(*args)

    def sparse(self, lib):
        args = self.common() + [None, None, ptr(self.ws), self.ws.numel() * 8, None, ptr(self.num), stream()]
        return lambda: lib.gsr_preprocess_backward_adam_raw_batched_sparse(*args)


def window(fn, n):
    """-> ms per launch over n launches between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        code = fn()
    e1.record()
    e1.synchronize()
    assert code == 0, code
    return e0.elapsed_time(e1) / n


def alternate(fns):
    """warm up, size the windows to WINDOW_MS, then REPEATS rounds over the launches in turn -> [[ms per launch] per fn]"""
    ns = []
    for fn in fns:
        window(fn, 3)
        ns.append(max(20, min(4000, int(math.ceil(WINDOW_MS / max(window(fn, 10), 1e-3))))))
    out = [[] for _ in fns]
    for _ in range(REPEATS):
        for k, fn in enumerate(fns):
            out[k].append(window(fn, ns[k]))
    return out


def stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5),
            "spread_ms": round(s[-1] - s[0], 5)}


def break_even(points):
    """points: [(active fraction, sparse ms, dense ms)] -> the fraction at which the sparse launch costs what the dense
    one does (linear between the two measured fractions that bracket it), None when they do not cross"""
    pts = sorted(points)
    for (f0, s0, d0), (f1, s1, d1) in zip(pts, pts[1:]):
        a, b = s0 - d0, s1 - d1
        if a <= 0 < b:
            return round(f0 + (f1 - f0) * (-a) / (b - a), 4)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--P", type=int, nargs="+", default=[1_000_000, 6_000_000])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    lib = _lib.lib
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        res, argt = _lib.SIGNATURES["gsr_preprocess_backward_adam_raw_batched"]
        parent.gsr_preprocess_backward_adam_raw_batched.restype = res
        parent.gsr_preprocess_backward_adam_raw_batched.argtypes = argt
        assert not hasattr(parent, "gsr_preprocess_backward_adam_raw_batched_sparse"), "--parent-lib has the sparse entry"
    res = {"width": W, "height": H, "sh_degree": DEG, "window_ms": WINDOW_MS, "repeats": REPEATS, "run_rows": RUN,
           "device": torch.cuda.get_device_name(0), "configs": [], "dense_parent_vs_this_tree": [], "summary": []}
    for P in a.P:
        for B in a.B:
            sc = Scene(P, B)
            if parent is not None:
                sc.set_active(1.0, "random")
                tp, tt = alternate([sc.dense(parent), sc.dense(lib)])
                sp, st = stats(tp), stats(tt)
                spread = max(sp["spread_ms"], st["spread_ms"])
                res["dense_parent_vs_this_tree"].append(
                    {"P": P, "B": B, "parent": sp, "this_tree": st,
                     "agree_within_spread": abs(sp["median_ms"] - st["median_ms"]) <= spread})
                print(json.dumps(res["dense_parent_vs_this_tree"][-1]), flush=True)
            for layout in ("random", "runs"):
                points = []
                for f in FRACTIONS:
                    nonzero, vis_pairs = sc.set_active(f, layout)
                    td, ts = alternate([sc.dense(lib), sc.sparse(lib)])
                    torch.cuda.synchronize()
                    active = int(sc.num)
                    assert active == nonzero, (active, nonzero)
                    d, s = stats(td), stats(ts)
                    db, sb = dense_bytes(P, B), sparse_bytes(P, B, vis_pairs, active)
                    rec = {"P": P, "B": B, "layout": layout, "fraction": f, "active_rows": active,
                           "active_fraction": round(active / P, 5), "dense": d, "sparse": s,
                           "dense_bytes": db, "sparse_bytes": sb,
                           "dense_GBps": round(db / d["median_ms"] / 1e6, 1),
                           "sparse_GBps": round(sb / s["median_ms"] / 1e6, 1),
                           "sparse_faster_by_ms": round(d["median_ms"] - s["median_ms"], 5),
                           "faster_beyond_dense_spread": d["median_ms"] - s["median_ms"] > d["spread_ms"]}
                    res["configs"].append(rec)
                    points.append((active / P, s["median_ms"], d["median_ms"]))
                    print(json.dumps(rec), flush=True)
                top = max(points)
                res["summary"].append({"P": P, "B": B, "layout": layout, "break_even_fraction": break_even(points),
                                       "cost_at_all_active_sparse_over_dense": round(top[1] / top[2], 3)})
                print(json.dumps(res["summary"][-1]), flush=True)
                with open(a.out, "w") as fo:  # (after every layout: a run that is cut short leaves what it measured)
                    json.dump(res, fo, indent=1)
            del sc
            torch.cuda.empty_cache()
    res["bar_sparse_faster_at_0.25_and_below"] = all(c["faster_beyond_dense_spread"] for c in res["configs"]
                                                     if c["fraction"] <= 0.25)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print(json.dumps({k: res[k] for k in ("summary", "dense_parent_vs_this_tree", "bar_sparse_faster_at_0.25_and_below")}))


if __name__ == "__main__":
    main()
