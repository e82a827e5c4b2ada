"""codebook compression A/B: one k-means assignment and one Lloyd update on the HIP kernels of vq.hip beside the only thing
the code offered before them -- chunked torch `matmul + argmin` and `index_add_` -- in one process, the legs taking turns
after a warm-up, device events around windows of a few hundred ms (tools/invdepth_ab.py's windows and statistics).
    python tools/vq_ab.py [OUT.json] [--P 1000000] [--D 45] [--K 4096,65536] [--rounds 7] [--scene-P 1000000]
Rows: N(0, 0.1^2) like the synthetic scene's SH coefficients; the codebook: K of the rows; the indices of the update: the
assignment's.  Per K: both times, their ratio, and the assignment's share of the fp32 matrix peak (2 P K D useful flops over
the time over 157.3 TFLOP/s; the kernel itself issues D rounded up to 16 columns).  No gate: the figures are written down.
Then the synthetic scene (seed 0, --scene-P Gaussians, 1920 x 1080): `compress` with K = 4096 and 5 iterations, the sizes
before and after, and the PSNR of the decoded model's render against the uncompressed model's render of the same camera.
The scene's SH values are random, so that PSNR says little about real scenes.
The last line printed is the whole result as one JSON object (also written to OUT.json when given; the project keeps
profiles/vq_ab.json).  Kernel names for a later trace: vq_assign_kernel<1..4>, vq_dist2_kernel, vq_keys_kernel,
vq_chunk_kernel<true|false>, vq_finalize_kernel<true|false>, vq_decode_kernel."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import compression  # noqa: E402
import diff_gaussian_rasterization as dgr  # noqa: E402
import synthetic_scene as S  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from invdepth_ab import H, W, WINDOW_MS, alternate, dev, stats  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12  # MI355X, dense fp32 MFMA
CHUNK_BYTES = 4 << 30        # the [rows, K] score matrix of the torch leg


def torch_assign(rows, cb):
    out = torch.empty(rows.shape[0], dtype=torch.int64, device=rows.device)
    step = max(1, CHUNK_BYTES // (4 * cb.shape[0]))
    norms = (cb * cb).sum(1)
    for i in range(0, rows.shape[0], step):
        out[i:i + step] = torch.addmm(norms[None, :], rows[i:i + step], cb.t(), alpha=-2.0).argmin(dim=1)
    return out


def torch_update(rows, idx, cb):
    sums = torch.zeros_like(cb).index_add_(0, idx, rows)
    count = torch.bincount(idx, minlength=cb.shape[0])
    cb.copy_(torch.where(count[:, None] > 0, sums / count.clamp_min(1)[:, None], cb))


def render(pc, cam):
    rs = dgr.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                                           torch.zeros(3, device=dev), 1.0, cam.world_view_transform.to(dev),
                                           cam.full_proj_transform.to(dev), 3, cam.camera_center.to(dev), False, False)
    rast = dgr.GaussianRasterizer(rs)
    mask = torch.ones((H + 15) // 16, (W + 15) // 16, dtype=torch.bool, device=dev)
    with torch.no_grad():
        a, b, c, d, e = rast.preprocess_gaussians(pc.get_xyz, pc.get_scaling, pc.get_rotation, pc.get_features,
                                                  pc.get_opacity, {})
        return rast.render_gaussians(a, c, b, e, d, mask, None, {"stats_collector": {}})[0].clamp(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--D", type=int, default=45)
    ap.add_argument("--K", default="4096,65536")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scene-P", type=int, default=1_000_000)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = 0.1 * torch.randn((a.P, a.D), device=dev, generator=gen)
    res = {"P": a.P, "D": a.D, "window_ms": WINDOW_MS, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.LIB_PATH), "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK / 1e12, "per_K": {}}
    for K in (int(k) for k in a.K.split(",")):
        cb = rows[torch.randperm(a.P, generator=torch.Generator().manual_seed(1))[:K].to(dev)].clone()
        idx = dgr.vq_assign(rows, cb)
        idx64, cb_hip, cb_torch = idx.long(), cb.clone(), cb.clone()
        same = float((torch_assign(rows, cb) == idx64).float().mean())
        legs = [[lambda: dgr.vq_assign(rows, cb) is None], [lambda: torch_assign(rows, cb) is None],
                [lambda: dgr.vq_update(rows, idx, cb_hip) is None], [lambda: torch_update(rows, idx64, cb_torch)],
                [lambda: dgr.vq_assign(rows, cb) is None]]
        t = alternate(legs, a.rounds)
        r = {n: stats(ts, 1) for n, ts in zip(("assign_hip", "assign_torch", "update_hip", "update_torch",
                                               "assign_hip_again"), t)}
        r["rows_assigned_like_torch"] = round(same, 6)
        r["ratio_assign_torch_over_hip"] = round(r["assign_torch"]["median_ms"] / r["assign_hip"]["median_ms"], 3)
        r["ratio_update_torch_over_hip"] = round(r["update_torch"]["median_ms"] / r["update_hip"]["median_ms"], 3)
        r["assign_useful_tflops"] = round(2.0 * a.P * K * a.D / (r["assign_hip"]["median_ms"] * 1e-3) / 1e12, 2)
        r["assign_frac_fp32_matrix_peak"] = round(r["assign_useful_tflops"] * 1e12 / FP32_MATRIX_PEAK, 4)
        r["noise_floor_ms"] = round(max(abs(r["assign_hip_again"]["median_ms"] - r["assign_hip"]["median_ms"]),
                                        r["assign_hip"]["spread_ms"], r["assign_hip_again"]["spread_ms"]), 5)
        res["per_K"][str(K)] = r
        del cb, idx, idx64, cb_hip, cb_torch
    del rows
    torch.cuda.empty_cache()
    pc = S.SyntheticGaussianModel(a.scene_P, W, H, seed=0, device=dev)
    cam = S.orbit_cameras(4, W, H)[1]
    ref = render(pc, cam)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cm = compression.compress(pc, groups={"f_rest": 4096}, iters=5, seed=0)
    torch.cuda.synchronize()
    compress_s = time.perf_counter() - t0
    before, after = cm.nbytes()
    cm.apply(pc)
    mse = float(((render(pc, cam) - ref) ** 2).mean())
    res["scene"] = {"P": a.scene_P, "K": 4096, "iters": 5, "compress_s": round(compress_s, 3),
                    "bytes_before": before, "bytes_after": after, "size_ratio": round(after / before, 4),
                    "psnr_decoded_vs_uncompressed_render_db": round(10.0 * math.log10(1.0 / max(mse, 1e-20)), 2),
                    "note": "random SH values: the PSNR says little about real scenes"}
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
