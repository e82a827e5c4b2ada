"""Time the per-camera evaluation metrics on one GPU: the stock-PyTorch sequence of the reference's training_report
(train_internal.py:471-478: two clamps, L1 mean, per-channel PSNR) against the fused launch of csrc/metrics.hip without
and with SSIM, at 1920x1080 and 4946x3286.  HIP events around batches of launches, the three routes alternating round by
round; prints one JSON line and (with --out) writes it to a file.  Needs a GPU: there is no CPU timing.

    python tools/eval_bench.py [--sizes 1920x1080,4946x3286] [--rounds 9] [--inner 20] [--out profiles/eval_bench.json]

Bytes (algorithmic, per camera of W x H, 3 channels):
  fused            : 15 B / pixel (fp32 image + uint8 ground truth, read once); the SSIM form re-reads a halo of 10 rows and
                     24 columns per 32x32 tile, which the L2 serves
  torch            : per element  gt / 255 (1 + 4), clamp (4 + 4), clamp (4 + 4), sub (8 + 4), abs (4 + 4), mean (4),
                     sub (8 + 4), square (4 + 4), mean (4) = 69 B, i.e. 207 B / pixel
  reference, W > 1 : the all-reduce of the fp32 image in front of it, 12 B / pixel on every rank's link (ring: ~2x that);
                     the band route sends 72 B per camera (+ 120 W B of strips per neighbour pair with SSIM)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_route(image, gt):
    import torch

    x = torch.clamp(image, 0.0, 1.0)
    y = torch.clamp(gt / 255.0, 0.0, 1.0)
    l1 = torch.abs(x - y).mean()
    mse = ((x - y) ** 2).view(x.shape[0], -1).mean(1, keepdim=True)
    return l1.double(), (20 * torch.log10(1.0 / torch.sqrt(mse))).mean().double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,4946x3286")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU (a CPU timing would say nothing about the MI355X)")
    from diff_gaussian_rasterization import image_metrics, metrics_from_sums

    dev = torch.device("cuda:0")
    result = {"tool": "eval_bench", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner,
              "sizes": {}}
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(W + H)
        gt = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8, device=dev)
        image = (gt.float() / 255.0 + 0.05 * torch.randn((3, H, W), generator=g, device=dev)).contiguous()
        routes = {"torch_l1_psnr": lambda: torch_route(image, gt),
                  "fused_no_ssim": lambda: image_metrics(image, gt, ssim=False),
                  "fused_ssim": lambda: image_metrics(image, gt, ssim=True)}
        # the routes agree (and this warms every shape up)
        for _ in range(3):
            l1_t, psnr_t = torch_route(image, gt)
            l1_f, psnr_f, _ = metrics_from_sums(routes["fused_no_ssim"](), H, W)
            l1_s, psnr_s, ssim_s = metrics_from_sums(routes["fused_ssim"](), H, W)
        torch.cuda.synchronize()
        agree = {"l1_rel": abs(float(l1_f) - float(l1_t)) / float(l1_t), "psnr_db": abs(float(psnr_f) - float(psnr_t)),
                 "l1_rel_ssim_form": abs(float(l1_s) - float(l1_t)) / float(l1_t), "ssim": float(ssim_s)}
        assert agree["l1_rel"] < 1e-4 and agree["psnr_db"] < 1e-3 and agree["l1_rel_ssim_form"] < 1e-4, agree
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for name, fn in routes.items():  # alternate the routes inside every round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.inner)
        px = W * H
        bytes_ = {"torch_l1_psnr": 207 * px, "fused_no_ssim": 15 * px, "fused_ssim": 15 * px}
        entry = {"agreement": agree, "reference_allreduce_bytes_per_rank": 12 * px, "band_route_wire_bytes": 72}
        for name, ts in times.items():
            med = statistics.median(ts)
            entry[name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "algorithmic_bytes": bytes_[name],
                           "GBps_at_median": bytes_[name] / med / 1e6}
        result["sizes"][size] = entry
        del image, gt
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
