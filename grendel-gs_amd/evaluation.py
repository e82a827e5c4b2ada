"""Evaluation of the model being trained: the `[ITER n] Evaluating test: L1 ... PSNR ...` line, MI355X build.

From-scratch mirror of the reference's training_report (train_internal.py:355-493) on top of one fused HIP launch per
camera (include/gsraster.h: gsr_image_metrics).  The reference all-reduces every rendered fp32 image over all ranks
(3 H W floats per test camera) and then runs about ten element-wise launches over it on every rank.  Everything it
prints is a sum over pixels, and sums are additive over the row bands the ranks already own:

* each rank scores ITS rows of every camera of the batch against the full ground truth it holds anyway
  (load_camera_from_cpu_to_all_gpu_for_eval);
* one all_reduce of [B, C, 3] doubles ends the batch -- nine doubles per camera cross the wire, never the image;
* SSIM (off in the training report, which prints L1 and PSNR) is the one metric whose window reaches five rows into the
  neighbouring bands: the ranks of a split camera first exchange their first and last five rendered rows (one
  all_gather_into_tensor of [2, C, 5, W] floats per split camera) and the kernel finds them in place.

Evaluation is eager (no hipGraph capture) and runs under torch.no_grad().
"""
import torch
import torch.distributed as dist

import utils.general_utils as utils
from diff_gaussian_rasterization import image_metrics, metrics_from_sums
from gaussian_renderer import (distributed_preprocess3dgs_and_all2all_final, get_invdepth, render_final,
                               set_invdepth)
from gaussian_renderer.loss_distribution import get_coverage_y_min_max, load_camera_from_cpu_to_all_gpu_for_eval
from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

HALO = 5  # rows the 11x11 SSIM window reaches beyond a band


def _band_of(strategy, rank):
    """pixel rows [y0, y1) of `rank`'s band of the strategy's camera (the rows final_system_loss_computation scores)"""
    j = strategy.gpu_ids.index(rank)
    return get_coverage_y_min_max(strategy.division_pos[j], strategy.division_pos[j + 1])


def _exchange_halo(image, strategy, group):
    """A camera split over ranks: every rank of the group contributes the first and last HALO rows of its band (zeros when
    it renders no part of the camera -- a collective needs everybody) and copies the rows of the OTHER bands that lie
    within HALO rows of its own into the zero rows of `image` (in place), where the SSIM window looks for them."""
    me = utils.GLOBAL_RANK
    mine = me in strategy.gpu_ids
    C, H, W = (image.shape if mine else (3, utils.IMG_H, utils.IMG_W))
    dev = image.device if mine else torch.device("cuda", torch.cuda.current_device())
    send = torch.zeros((2, C, HALO, W), dtype=torch.float32, device=dev)
    if mine:
        y0, y1 = _band_of(strategy, me)
        n = min(HALO, y1 - y0)
        send[0, :, :n] = image[:, y0:y0 + n]
        send[1, :, HALO - n:] = image[:, y1 - n:y1]
    recv = torch.empty((group.size(), 2, C, HALO, W), dtype=torch.float32, device=dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    if not mine:
        return
    want = ((max(0, y0 - HALO), y0), (y1, min(H, y1 + HALO)))
    for g in strategy.gpu_ids:
        if g == me:
            continue
        a, b = _band_of(strategy, g)
        n = min(HALO, b - a)
        # the peer's two strips as (first image row, strip index, first strip row)
        for lo, s, r0 in ((a, 0, 0), (b - n, 1, HALO - n)):
            for w0, w1 in want:
                u0, u1 = max(lo, w0), min(lo + n, w1)
                if u0 < u1:
                    image[:, u0:u1] = recv[g, s, :, r0 + (u0 - lo):r0 + (u1 - lo)]


def evaluate_batch(batched_image, batched_cameras, batched_strategies, *, ssim=False, quantize=False):
    """-> float64 [B, C, 3] on the device, identical on every rank: per camera and channel (sum |x - y|, sum (x - y)^2,
    sum ssim_map) over the WHOLE image, x = clamp(render, 0, 1), y = ground truth / 255 (diff_gaussian_rasterization.
    image_metrics; metrics_from_sums turns a camera's [C, 3] into L1 / PSNR / SSIM).  batched_image is render_final's
    list: an entry that is None (camera not rendered here) contributes nothing, a 0-dim stand-in (< 10 Gaussians arrived,
    train_internal.py:457-464) scores its band as an all-zero image -- the reference's sum of images.  camera.original_image
    is the FULL uint8 ground truth (load_camera_from_cpu_to_all_gpu_for_eval).  With `ssim`, the images of cameras split
    over ranks receive their neighbours' halo rows IN PLACE."""
    group = utils.DEFAULT_GROUP
    me = utils.GLOBAL_RANK
    dev = torch.device("cuda", torch.cuda.current_device())
    gts = [c.original_image for c in batched_cameras]
    C = next((g.shape[0] for g in gts if g is not None), 3)
    out = torch.zeros((len(batched_cameras), C, 3), dtype=torch.float64, device=dev)
    for k, (image, camera, strategy) in enumerate(zip(batched_image, batched_cameras, batched_strategies)):
        mine = image is not None and me in strategy.gpu_ids
        if mine:
            gt = camera.original_image
            if not gt.is_cuda:
                raise RuntimeError("evaluate_batch: the ground truth must live on the gfx950 device (no CPU fallback)")
            if image.dim() == 0:
                image = torch.zeros(gt.shape, dtype=torch.float32, device=gt.device)
        if ssim and len(strategy.gpu_ids) > 1 and group.size() > 1:
            _exchange_halo(image if mine else None, strategy, group)
        if mine:
            y0, y1 = _band_of(strategy, me)
            out[k] = image_metrics(image, gt, y0, y1, ssim=ssim, quantize=quantize)
    if group.size() > 1:
        dist.all_reduce(out, op=dist.ReduceOp.SUM, group=group)
    return out


class EvalDataset:
    """the sampling of the reference's SceneDataset (scene/__init__.py:203-279) that evaluation uses: cameras are drawn
    without replacement from a shuffled epoch, a batch never holds a camera twice"""

    def __init__(self, cameras):
        self.cameras = cameras
        self.camera_size = len(cameras)
        self.sample_camera_idx = [i for i, c in enumerate(cameras) if c.original_image_backup is not None]
        self.cur_epoch_cameras = []

    def _next(self, taken_uids):
        if not self.cur_epoch_cameras:
            pool = self.sample_camera_idx if utils.get_args().local_sampling else list(range(self.camera_size))
            self.cur_epoch_cameras = [pool[i] for i in torch.randperm(len(pool)).tolist()]
        at = 0
        while self.cameras[self.cur_epoch_cameras[at]].uid in taken_uids:
            at += 1
        return self.cur_epoch_cameras.pop(at)

    def get_batched_cameras_idx(self, batch_size):
        assert batch_size <= self.camera_size, "Batch size is larger than the number of cameras in the scene."
        idx, uids = [], []
        for _ in range(batch_size):
            i = self._next(uids)
            idx.append(i)
            uids.append(self.cameras[i].uid)
        return idx

    def get_batched_cameras(self, batch_size):
        return [self.cameras[i] for i in self.get_batched_cameras_idx(batch_size)]

    def get_batched_cameras_from_idx(self, idx_list):
        return [self.cameras[i] for i in idx_list]


def report_line(iteration, name, l1, psnr):
    """the line examples/mip360/analyze_results.py:59-64 of the reference parses (`line.split("L1 ")[1].split(" PSNR")[0]`,
    `line.split("PSNR ")[1]`): plain numbers that float() reads back exactly"""
    return "[ITER {}] Evaluating {}: L1 {} PSNR {}".format(iteration, name, repr(float(l1)), repr(float(psnr)))


def _say(text):
    if utils.GLOBAL_RANK == 0:
        print(text, flush=True)


@torch.no_grad()
def training_report(iteration, testing_iterations, scene, pipe_args, background, *, ssim=False, quantize=False,
                    invdepth=False):
    """Mirror of train_internal.py:355-493.  When the batch [iteration, iteration + bsz) reaches testing_iterations[0]
    (popped; passed entries are dropped first): render the test cameras and a subset of the train cameras in batches of
    bsz and write, per set, `[ITER n] Evaluating <name>: L1 <l1> PSNR <psnr>` -- rank 0 prints it, every rank writes it to
    utils.get_log_file().  The means over the cameras are accumulated in fp64 on the device; one host read per set.
    -> {name: {"l1", "psnr", "ssim" (None unless asked for), "num_cameras", "cameras" (uids, in the order scored)}}, empty
    when nothing was due (the reference returns nothing; a caller here wants the numbers).
    `invdepth` (extension of this build): also render every scored camera's inverse-depth map (gaussian_renderer
    .set_invdepth, switched on for the duration of the call), assembled across the bands by a SUM all-reduce like the
    image, and return them as report[name]["invdepth"]: one [H,W] device tensor per entry of "cameras", 4 H W bytes each."""
    args = utils.get_args()
    log_file = utils.get_log_file()
    while len(testing_iterations) > 0 and iteration > testing_iterations[0]:
        testing_iterations.pop(0)
    if not (len(testing_iterations) > 0 and
            utils.check_update_at_this_iter(iteration, args.bsz, testing_iterations[0], 0)):
        return {}
    testing_iterations.pop(0)
    _say("\n[ITER {}] Start Testing".format(iteration))
    group = utils.DEFAULT_GROUP
    dev = torch.device("cuda", torch.cuda.current_device())
    train_cameras, test_cameras = scene.getTrainCameras(), scene.getTestCameras()
    configs = (("test", test_cameras, len(test_cameras) if test_cameras else 0),
               ("train", train_cameras,
                max(len(train_cameras) // getattr(args, "llffhold", 8), args.bsz) if train_cameras else 0))
    report = {}
    for name, cameras, wanted in configs:
        if not cameras or len(cameras) == 0:
            continue
        num_cameras = wanted // args.bsz * args.bsz  # (the reference's truncation to whole batches)
        dataset = EvalDataset(cameras)
        history = DivisionStrategyHistoryFinal(dataset, group.size(), group.rank())
        acc = torch.zeros(3, dtype=torch.float64, device=dev)  # sums over the cameras of (l1, psnr, ssim)
        uids, maps = [], []
        for idx in range(1, num_cameras + 1, args.bsz):
            to_load = min(args.bsz, num_cameras - idx + 1)
            if args.local_sampling:
                mine = torch.tensor(dataset.get_batched_cameras_idx(args.bsz // utils.WORLD_SIZE), device=dev,
                                    dtype=torch.int64)
                everybody = torch.zeros((utils.WORLD_SIZE, mine.numel()), device=dev, dtype=torch.int64)
                dist.all_gather_into_tensor(everybody, mine, group=group)
                batched_cameras = dataset.get_batched_cameras_from_idx(everybody.cpu().reshape(-1).tolist())
            else:
                batched_cameras = dataset.get_batched_cameras(to_load)
            strategies, gpuid2tasks = start_strategy_final(batched_cameras, history)
            load_camera_from_cpu_to_all_gpu_for_eval(batched_cameras, strategies, gpuid2tasks)
            was = get_invdepth()
            set_invdepth(was or invdepth)
            try:
                pkg = distributed_preprocess3dgs_and_all2all_final(batched_cameras, scene.gaussians, pipe_args,
                                                                   background, batched_strategies=strategies, mode="test")
                batched_image, _ = render_final(pkg, strategies)
            finally:
                set_invdepth(was)
            sums = evaluate_batch(batched_image, batched_cameras, strategies, ssim=ssim, quantize=quantize)
            l1, psnr, ss = metrics_from_sums(sums, utils.IMG_H, utils.IMG_W)
            keep = [k for k in range(len(batched_cameras)) if idx + k < num_cameras + 1]
            acc += torch.stack([l1[keep].sum(), psnr[keep].sum(), ss[keep].sum()])
            for k, camera in enumerate(batched_cameras):
                if k in keep:
                    uids.append(camera.uid)
                    if invdepth:
                        inv = pkg["batched_invdepth"][k]
                        inv = torch.zeros((utils.IMG_H, utils.IMG_W), device=dev) if inv is None else inv[0].clone()
                        if group.size() > 1:
                            dist.all_reduce(inv, op=dist.ReduceOp.SUM, group=group)
                        maps.append(inv)
                camera.original_image = None
        if num_cameras == 0:
            continue
        l1_mean, psnr_mean, ssim_mean = (acc / num_cameras).tolist()  # the one host read of this set
        line = report_line(iteration, name, l1_mean, psnr_mean)
        _say("\n" + line)
        if log_file is not None:
            log_file.write(line + "\n")
        report[name] = {"l1": l1_mean, "psnr": psnr_mean, "ssim": ssim_mean if ssim else None,
                        "num_cameras": num_cameras, "cameras": uids}
        if invdepth:
            report[name]["invdepth"] = maps
    torch.cuda.empty_cache()
    return report
