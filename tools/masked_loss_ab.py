"""masked-loss A/B: the L1 + SSIM loss launches with and without a per-pixel mask (include/gsraster.h, N1m) on the same
inputs, same process, legs interleaved, warmed up, device events around windows of ~100 ms of launches.
    python tools/masked_loss_ab.py OUT.json [--parent-lib PATH/libgsraster.so] [--window-ms 100] [--repeats 7]
Shape: the full 1080p image (3 x 1080 x 1920), static form.  Legs, each its own window:
  plain_forward / masked_forward                      gsr_l1_ssim_forward            / gsr_l1_ssim_forward_masked
  plain_backward / masked_backward                    gsr_l1_ssim_backward           / gsr_l1_ssim_backward_masked
  exposure_forward / masked_exposure_forward          gsr_l1_ssim_forward_exposure   / ..._masked with an exposure
  exposure_backward / masked_exposure_backward        gsr_l1_ssim_backward_exposure  / ..._masked with an exposure
  plain_forward_again, plain_backward_again           the first legs once more: their ratio to the first visit is the
                                                      noise floor of this run -- a masked / plain ratio inside it says
                                                      nothing
The mask is random bytes (every pixel a different weight; an all-255 mask runs the same instructions).  The unmasked
kernels of this build are the parent commit's instruction streams (compared in the disassembly), so the
plain legs ARE the parent's kernels in the same run; --parent-lib adds the parent's own library as one more pair of legs.
The loss finalize is the same launch everywhere and is left out.  The host's enqueue time of every window is recorded: a
window whose host time is not well below its device time measures the launch path, not the kernels."""
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
E = [[1.10, 0.15, -0.20, 0.05], [-0.10, 0.90, 0.20, -0.10], [0.20, -0.15, 1.05, 0.08]]


def load_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("gsr_l1_ssim_forward", "gsr_l1_ssim_backward"):
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Case:
    def __init__(self, dev):
        g = torch.Generator(device=dev).manual_seed(3)
        self.rows = H
        self.img = torch.rand((3, H, W), device=dev, generator=g)
        self.gt = torch.randint(0, 256, (3, H, W), device=dev, generator=g, dtype=torch.uint8)
        self.mask = torch.randint(0, 256, (H, W), device=dev, generator=g, dtype=torch.uint8)
        self.maps = torch.empty((3, 3, H, W), device=dev)
        self.grad = torch.zeros((3, H, W), device=dev)
        lib = _lib.lib
        self.partials = torch.empty((lib.gsr_l1_ssim_num_partials(3, H, W), 2), device=dev)
        self.ep = torch.empty((lib.gsr_l1_ssim_exposure_num_partials(H, W), 12), device=dev)
        self.E = torch.tensor(E, device=dev)
        self.gE = torch.empty((3, 4), device=dev)
        self.g = torch.ones((1,), device=dev)
        self.s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ip, self.gp = self.img.data_ptr(), self.grad.data_ptr()
        self.m = [self.maps[i].data_ptr() for i in range(3)]

    def plain_fwd(self, lib):
        return lib.gsr_l1_ssim_forward(3, H, W, self.ip, H * W, self.gt.data_ptr(), self.partials.data_ptr(), self.m[0],
                                       self.m[1], self.m[2], self.s)

    def plain_bwd(self, lib):
        return lib.gsr_l1_ssim_backward(3, H, W, self.ip, H * W, self.gt.data_ptr(), self.m[0], self.m[1], self.m[2],
                                        self.g.data_ptr(), self.g.data_ptr(), 1e-6, -1e-6, self.gp, H * W, self.s)

    def expo_fwd(self, lib):
        return lib.gsr_l1_ssim_forward_exposure(3, H, W, self.ip, H * W, self.gt.data_ptr(), self.partials.data_ptr(),
                                                self.m[0], self.m[1], self.m[2], None, self.E.data_ptr(), self.s)

    def expo_bwd(self, lib):
        return lib.gsr_l1_ssim_backward_exposure(3, H, W, self.ip, H * W, self.gt.data_ptr(), self.m[0], self.m[1],
                                                 self.m[2], self.g.data_ptr(), self.g.data_ptr(), 1e-6, -1e-6, self.gp,
                                                 H * W, None, self.E.data_ptr(), self.ep.data_ptr(), self.gE.data_ptr(),
                                                 self.s)

    def masked_fwd(self, lib, expo):
        return lib.gsr_l1_ssim_forward_masked(3, H, W, self.ip, H * W, self.gt.data_ptr(), self.mask.data_ptr(),
                                              self.partials.data_ptr(), self.m[0], self.m[1], self.m[2], None,
                                              self.E.data_ptr() if expo else None, self.s)

    def masked_bwd(self, lib, expo):
        return lib.gsr_l1_ssim_backward_masked(3, H, W, self.ip, H * W, self.gt.data_ptr(), self.mask.data_ptr(),
                                               self.m[0], self.m[1], self.m[2], self.g.data_ptr(), self.g.data_ptr(), 1e-6,
                                               -1e-6, self.gp, H * W, None, self.E.data_ptr() if expo else None,
                                               self.ep.data_ptr() if expo else None, self.gE.data_ptr() if expo else None,
                                               self.s)


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


PAIRS = [("masked_forward", "plain_forward"), ("masked_backward", "plain_backward"),
         ("masked_exposure_forward", "exposure_forward"), ("masked_exposure_backward", "exposure_backward")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_loss_ab: no GPU (this measurement has no CPU form)")
    dev = torch.device("cuda:0")
    lib = _lib.lib
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    c = Case(dev)
    # the backward legs read the maps of whichever forward ran last: their values differ, their traffic does not
    legs = {
        "plain_forward": [lambda: c.plain_fwd(lib)],
        "masked_forward": [lambda: c.masked_fwd(lib, False)],
        "plain_backward": [lambda: c.plain_bwd(lib)],
        "masked_backward": [lambda: c.masked_bwd(lib, False)],
        "exposure_forward": [lambda: c.expo_fwd(lib)],
        "masked_exposure_forward": [lambda: c.masked_fwd(lib, True)],
        "exposure_backward": [lambda: c.expo_bwd(lib)],
        "masked_exposure_backward": [lambda: c.masked_bwd(lib, True)],
        "plain_forward_again": [lambda: c.plain_fwd(lib)],
        "plain_backward_again": [lambda: c.plain_bwd(lib)],
    }
    if parent is not None:
        legs["parent_plain_forward"] = [lambda: c.plain_fwd(parent)]
        legs["parent_plain_backward"] = [lambda: c.plain_bwd(parent)]
    counts = {}
    for k, fns in legs.items():  # warm-up (code objects, maps written once) and the round count of a window
        window(fns, 20)
        ms, _ = window(fns, 50)
        counts[k] = max(50, int(a.window_ms / max(ms, 1e-4)))
    samples = {k: [] for k in legs}
    hosts = {k: [] for k in legs}
    for _ in range(a.repeats):  # interleaved: every repeat visits every leg once
        for k, fns in legs.items():
            ms, host = window(fns, counts[k])
            samples[k].append(ms)
            hosts[k].append(host)
    rec = {"window_ms": a.window_ms, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rows": H, "width": W,
           "legs": {}}
    for k in legs:
        v = sorted(samples[k])
        rec["legs"][k] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "samples_ms": samples[k],
                          "host_ms_per_round": sorted(hosts[k])[len(v) // 2], "rounds_per_window": counts[k]}
    med = {k: rec["legs"][k]["median_ms"] for k in legs}
    rec["ratios"] = {f"{m}_over_{p}": med[m] / med[p] for m, p in PAIRS}
    rec["noise_floor"] = {
        "plain_forward_again_over_first": med["plain_forward_again"] / med["plain_forward"],
        "plain_backward_again_over_first": med["plain_backward_again"] / med["plain_backward"],
        "worst_window_spread": max((rec["legs"][k]["max_ms"] - rec["legs"][k]["min_ms"]) / med[k] for k in legs),
    }
    if parent is not None:
        rec["ratios"]["plain_forward_over_parent"] = med["plain_forward"] / med["parent_plain_forward"]
        rec["ratios"]["plain_backward_over_parent"] = med["plain_backward"] / med["parent_plain_backward"]
    # what the mask adds to the traffic: one byte per pixel per launch, against the launch's own bytes per pixel
    # (forward: 3 x (4 + 1) in, 3 x 3 x 4 maps out; backward: 3 x (3 x 4 + 4 + 1) in, 3 x 4 out)
    rec["mask_bytes_over_launch_bytes"] = {"forward": 1.0 / 51.0, "backward": 1.0 / 63.0}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("legs", json.dumps({k: round(v, 5) for k, v in med.items()}), flush=True)
    print("MASKED_LOSS_AB " + json.dumps({"ratios": rec["ratios"], "noise_floor": rec["noise_floor"]}))


if __name__ == "__main__":
    main()
