"""Freeze what the REFERENCE's own metric functions give on the leaf-test inputs, and its evaluation schedule
-> tests/golden/reference_eval_metrics.json.

Runs in the build container (host-only code): imports utils.image_utils.psnr, utils.loss_utils.l1_loss / ssim and
utils.general_utils.check_update_at_this_iter from /root/reference (grendel-gs_amd/b1_graft on the module path stands in
for the rasterizer package the reference's utils import) and records

  metrics : for leaf_refs.loss_inputs(family, C, H, W), every family x SHAPES: l1_loss(x, y).mean(), psnr(x, y).mean(),
            ssim(x, y) of x = clamp(image, 0, 1), y = clamp(gt / 255, 0, 1) in float32, exactly as train_internal.py:471-478
            forms the two images -- plus an fp64 checksum of the inputs, so that a drifting generator is caught.  Only the
            values are stored, not the images;
  schedule: check_update_at_this_iter(iteration, bsz, interval, 0) over a few hundred tuples.

tests/test_metrics_cpu.py holds the fp64 restatement (tests/metric_refs.py) and the mirror's schedule function to it."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
SHAPES = [(1, 5, 4), (3, 33, 37), (3, 83, 131), (3, 96, 100)]


def schedule_tuples():
    out = []
    for bsz in (1, 2, 4, 8):
        for interval in (1, 7, 100, 1000):
            for it in list(range(1, 26)) + [interval - bsz, interval - 1, interval, interval + 1, 2 * interval - bsz + 1,
                                            7000 - bsz + 1, 7000, 30000]:
                if it >= 0:
                    out.append((it, bsz, interval, 0))
    return out


def main():
    sys.path[:0] = [REF, os.path.join(ROOT, "grendel-gs_amd", "b1_graft"), os.path.join(ROOT, "tests"), ROOT]
    import utils.general_utils as utils
    from utils.image_utils import psnr
    from utils.loss_utils import l1_loss, ssim

    import leaf_refs as R

    assert utils.__file__.startswith(REF)
    metrics = []
    for family in R.FAMILIES:
        for C, H, W in SHAPES:
            image, gt, _ = R.loss_inputs(family, C, H, W)
            x = torch.clamp(image, 0.0, 1.0)
            y = torch.clamp(gt / 255.0, 0.0, 1.0)
            metrics.append({"family": family, "C": C, "H": H, "W": W,
                            "checksum": [float(image.double().sum()), float(image.double().abs().sum()),
                                         float(gt.double().sum())],
                            "l1": float(l1_loss(x, y).mean().double()), "psnr": float(psnr(x, y).mean().double()),
                            "ssim": float(ssim(x, y).double())})
    schedule = [[it, bsz, iv, res, bool(utils.check_update_at_this_iter(it, bsz, iv, res))]
                for it, bsz, iv, res in schedule_tuples()]
    path = os.path.join(ROOT, "tests", "golden", "reference_eval_metrics.json")
    with open(path, "w") as f:
        json.dump({"metrics": metrics, "schedule": schedule}, f, allow_nan=True)
    print("wrote", path, len(metrics), "metric cases,", len(schedule), "schedule tuples")


if __name__ == "__main__":
    main()
