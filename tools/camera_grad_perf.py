"""Camera-gradient kernel next to the unfused K11 on the same inputs: one forward, then `--reps` backward passes of the
camera-batched projection with `cams.requires_grad_()`, so that every backward launches K11 AND the camera kernel.

Meant to run under the profiler, which gives the per-kernel times:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/camera_grad_perf.py --B 4

Without a profiler it prints the HIP-event times of the two ranges (launch overhead included) and the algorithmic
bytes of the camera kernel: per Gaussian 4 B radius per camera, and per VISIBLE (Gaussian, camera) 36 B gradient row +
3 B clamp flags, plus 12 + 24 + 180 B position / covariance / SH above DC once per Gaussian visible anywhere."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, N, B = a.width, a.height, a.P, a.B
    m = S.SyntheticGaussianModel(N, W, H, seed=0, device=dev, on_device=True)
    names = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")
    rss = [dgr.GaussianRasterizationSettings(H, W, math.tan(c.FoVx / 2), math.tan(c.FoVy / 2), torch.zeros(3, device=dev),
                                             1.0, c.world_view_transform, c.full_proj_transform, 3, c.camera_center,
                                             False, False) for c in S.orbit_cameras(8, W, H, device=dev)[:B]]
    rec = torch.stack([dgr.pack_camera(rs) for rs in rss]).requires_grad_()
    gen = torch.Generator(device=dev).manual_seed(1)
    ws = [[torch.randn(s, generator=gen, device=dev) for s in [(N, 2), (N, 3), (N, 4)]] for _ in range(B)]
    dgr.kernel_timer.enabled = True
    visible = None
    for it in range(a.reps + 3):
        if it == 3:
            dgr.kernel_timer.reset()
        m2, rgb, co, radii, depths = dgr.preprocess_gaussians_raw_batched(
            *[getattr(m, n) for n in names], rec, 3, 1.0, W, H, tanfov0=(rss[0].tanfovx, rss[0].tanfovy))
        loss = sum((m2[k] * ws[k][0]).sum() + (rgb[k] * ws[k][1]).sum() + (co[k] * ws[k][2]).sum() for k in range(B))
        loss.backward()
        if visible is None:
            r = torch.stack(list(radii)) > 0
            visible = (int(r.sum()), int(r.any(dim=0).sum()))
        for n in names:
            getattr(m, n).grad = None
        rec.grad = None
    torch.cuda.synchronize()
    ms = {k: v[1] for k, v in dgr.kernel_timer.summary_ms().items()}
    pairs, rows = visible
    nbytes = 4 * N * B + 39 * pairs + 216 * rows
    print(json.dumps({"P": N, "B": B, "visible_pairs": pairs, "visible_rows": rows,
                      "camera_kernel_bytes": nbytes,
                      "event_ms": {k: round(v, 4) for k, v in ms.items() if k.startswith("preprocess_backward")}}))


if __name__ == "__main__":
    main()
