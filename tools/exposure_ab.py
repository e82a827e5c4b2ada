"""exposure A/B: the loss forward + backward pair with and without per-camera exposure compensation on the same inputs,
same process, alternating, warmed up, device events around windows of ~200 ms of launches.
    python tools/exposure_ab.py OUT.json [--parent-lib PATH/libgsraster.so] [--window-ms 200] [--repeats 5]
Shapes: the full 1080p image (3 x 1080 x 1920) and a 1/8 row band of it (135 rows, rows [472, 607)).  Timed per shape:
  plain    gsr_l1_ssim_forward + gsr_l1_ssim_backward                      (kernels l1_ssim_forward_kernel<.., false>,
           l1_ssim_backward_kernel)
  exposure gsr_l1_ssim_forward_exposure + gsr_l1_ssim_backward_exposure   (l1_ssim_forward_kernel<.., true>,
           l1_ssim_backward_exposure_kernel, exposure_finalize_kernel)
each also forward only and backward only, so that the pair's cost can be placed.  --parent-lib: a libgsraster.so built
from the parent commit; its plain pair is timed in the same alternation ("the plain instantiations did not change").
The loss finalize (gsr_l1_ssim_finalize) is the same launch in both and is left out.  One streaming pass over the band --
what torch glue around the loss would add at least once per direction -- is 36 bytes per pixel; the JSON carries its
time at the measured copy bandwidth of the chip for comparison.  The host's enqueue time of every window is recorded
too: a window whose host time is not well below its device time measures the launch path, not the kernels."""
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
SHAPES = {"full_1080p": (0, 1080), "band_135": (472, 607)}
COPY_BW = 6.29e12  # measured float4 copy bandwidth of the chip, bytes / s
E = [[1.10, 0.15, -0.20, 0.05], [-0.10, 0.90, 0.20, -0.10], [0.20, -0.15, 1.05, 0.08]]


def load_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("gsr_l1_ssim_forward", "gsr_l1_ssim_backward"):
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Case:
    def __init__(self, dev, y0, y1):
        g = torch.Generator(device=dev).manual_seed(3)
        self.y0, self.y1, self.rows = y0, y1, y1 - y0
        self.img = torch.rand((3, H, W), device=dev, generator=g)
        self.gt = torch.randint(0, 256, (3, self.rows, W), device=dev, generator=g, dtype=torch.uint8)
        self.maps = torch.empty((3, 3, self.rows, W), device=dev)
        self.grad = torch.zeros((3, H, W), device=dev)
        lib = _lib.lib
        self.partials = torch.empty((lib.gsr_l1_ssim_num_partials(3, self.rows, W), 2), device=dev)
        self.ep = torch.empty((lib.gsr_l1_ssim_exposure_num_partials(self.rows, W), 12), device=dev)
        self.E = torch.tensor(E, device=dev)
        self.gE = torch.empty((3, 4), device=dev)
        self.g = torch.ones((1,), device=dev)
        self.s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        off = 4 * y0 * W
        self.ip, self.gp = self.img.data_ptr() + off, self.grad.data_ptr() + off
        self.m = [self.maps[i].data_ptr() for i in range(3)]

    def plain_fwd(self, lib):
        return lib.gsr_l1_ssim_forward(3, self.rows, W, self.ip, H * W, self.gt.data_ptr(), self.partials.data_ptr(),
                                       self.m[0], self.m[1], self.m[2], self.s)

    def plain_bwd(self, lib):
        return lib.gsr_l1_ssim_backward(3, self.rows, W, self.ip, H * W, self.gt.data_ptr(), self.m[0], self.m[1],
                                        self.m[2], self.g.data_ptr(), self.g.data_ptr(), 1e-6, -1e-6, self.gp, H * W,
                                        self.s)

    def expo_fwd(self, lib):
        return lib.gsr_l1_ssim_forward_exposure(3, self.rows, W, self.ip, H * W, self.gt.data_ptr(),
                                                self.partials.data_ptr(), self.m[0], self.m[1], self.m[2], None,
                                                self.E.data_ptr(), self.s)

    def expo_bwd(self, lib):
        return lib.gsr_l1_ssim_backward_exposure(3, self.rows, W, self.ip, H * W, self.gt.data_ptr(), self.m[0],
                                                 self.m[1], self.m[2], self.g.data_ptr(), self.g.data_ptr(), 1e-6, -1e-6,
                                                 self.gp, H * W, None, self.E.data_ptr(), self.ep.data_ptr(),
                                                 self.gE.data_ptr(), self.s)


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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exposure_ab: no GPU (this measurement has no CPU form)")
    dev = torch.device("cuda:0")
    lib = _lib.lib
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    result = {"window_ms": a.window_ms, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, (y0, y1) in SHAPES.items():
        c = Case(dev, y0, y1)
        variants = {
            "plain_pair": [lambda: c.plain_fwd(lib), lambda: c.plain_bwd(lib)],
            "exposure_pair": [lambda: c.expo_fwd(lib), lambda: c.expo_bwd(lib)],
            "plain_forward": [lambda: c.plain_fwd(lib)],
            "exposure_forward": [lambda: c.expo_fwd(lib)],
            "plain_backward": [lambda: c.plain_bwd(lib)],
            "exposure_backward": [lambda: c.expo_bwd(lib)],
        }
        if parent is not None:
            variants["parent_plain_pair"] = [lambda: c.plain_fwd(parent), lambda: c.plain_bwd(parent)]
        counts = {}
        for k, fns in variants.items():  # warm-up (code objects, maps written once) and the round count of a window
            window(fns, 20)
            ms, _ = window(fns, 50)
            counts[k] = max(50, int(a.window_ms / max(ms, 1e-4)))
        samples = {k: [] for k in variants}
        hosts = {k: [] for k in variants}
        for _ in range(a.repeats):  # alternating: every repeat visits every variant once
            for k, fns in variants.items():
                ms, host = window(fns, counts[k])
                samples[k].append(ms)
                hosts[k].append(host)
        px = c.rows * W
        rec = {"rows": c.rows, "pixels": px, "streaming_pass_ms": 36.0 * px / COPY_BW * 1e3, "variants": {}}
        for k in variants:
            v = sorted(samples[k])
            rec["variants"][k] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "samples_ms": samples[k],
                                  "host_ms_per_round": sorted(hosts[k])[len(v) // 2], "rounds_per_window": counts[k]}
        med = {k: rec["variants"][k]["median_ms"] for k in variants}
        rec["exposure_over_plain"] = med["exposure_pair"] / med["plain_pair"]
        if parent is not None:
            rec["plain_over_parent_plain"] = med["plain_pair"] / med["parent_plain_pair"]
            rec["exposure_over_parent_plain"] = med["exposure_pair"] / med["parent_plain_pair"]
        result["shapes"][name] = rec
        print(name, json.dumps({k: round(v, 5) for k, v in med.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("EXPOSURE_AB " + json.dumps({n: {"exposure_over_plain": r["exposure_over_plain"],
                                           "plain_over_parent_plain": r.get("plain_over_parent_plain")}
                                       for n, r in result["shapes"].items()}))


if __name__ == "__main__":
    main()
