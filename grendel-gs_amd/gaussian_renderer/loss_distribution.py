"""Ground-truth staging and band-local loss of the hot path (host side), MI355X build.

From-scratch mirror of the live functions of the reference's gaussian_renderer/loss_distribution.py
(the eight legacy loss modes at :127-2318 are unreachable, SURVEY.md F4, and are not provided):

  load_camera_from_cpu_to_all_gpu            loss_distribution.py:2395-2533
  load_camera_from_cpu_to_all_gpu_for_eval   loss_distribution.py:2333-2392
  final_system_loss_computation              loss_distribution.py:2536-2585
  batched_loss_computation                   loss_distribution.py:2588-2637

Each rank evaluates L1 and SSIM on ITS row band only, zero-padded at the band edges (no halo), both
normalised by the FULL image's pixel count, so that the per-rank partial losses of a camera add up to
the full-image loss up to the band-border SSIM term.
"""
import math
import os

import torch
import torch.distributed as dist

import utils.general_utils as utils

# The fused HIP loss lives in this package's operator module.  A missing / unbuilt libgsraster.so makes this import
# raise; there is no torch / conv2d restatement of the loss in the product (oracle/loss_oracle.py holds one for the
# tests, pinned on the reference's own pixelwise_l1_with_mask / pixelwise_ssim_with_mask).
from diff_gaussian_rasterization import bilagrid_slice as _BILAGRID_SLICE
from diff_gaussian_rasterization import capturing as _capturing
from diff_gaussian_rasterization import current_stream as _current_stream
from diff_gaussian_rasterization import fused_band_loss as _FUSED_LOSS
from diff_gaussian_rasterization import fused_band_loss_exposure as _FUSED_LOSS_EXPOSURE
from diff_gaussian_rasterization import fused_band_loss_masked as _FUSED_LOSS_MASKED
from diff_gaussian_rasterization import fused_l1_ssim_band as _FUSED


def _device():
    """the current HIP device.  Deliberately NOT a helper of `utils`: when these files are grafted over the
    reference's (INTEGRATION.md level B2) `utils` is the reference's own module, which has no such function."""
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def get_coverage_y_min(tile_row_l):
    return tile_row_l * utils.BLOCK_Y


def get_coverage_y_max(tile_row_r):
    return min(tile_row_r * utils.BLOCK_Y, utils.IMG_H)


def get_coverage_y_min_max(tile_row_l, tile_row_r):
    return get_coverage_y_min(tile_row_l), get_coverage_y_max(tile_row_r)


# ------------------------------------------------------------------------------- GT staging
def _band_of(camera, l, r, device):
    """uint8 rows [l * 16, min(r * 16, H)) of the camera's ground truth, dense, on `device`.  When the image already
    lives on the device (preload_dataset_to_gpu, scene/cameras.py:66-69) the dense band is a strided-slice copy kernel
    per iteration: the last few bands of a camera are kept (a converged partition asks for the same rows again)."""
    return _rows_of(camera, camera.original_image_backup, "_gsr_bands", l, r, device)


def _mask_band_of(camera, l, r, device):
    """the same rows of the camera's loss mask (alpha_mask_backup, uint8 [H, W] or [1, H, W]) as [1, rows, W], staged and
    cached exactly like the ground truth's band"""
    src = camera.alpha_mask_backup
    if src.dtype != torch.uint8 or src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[0] != 1):
        raise ValueError(f"alpha_mask_backup must be uint8 [H, W] or [1, H, W], got {src.dtype} {tuple(src.shape)}")
    return _rows_of(camera, src if src.dim() == 3 else src.unsqueeze(0), "_gsr_mask_bands", l, r, device)


def _rows_of(camera, src, cache_name, l, r, device):
    y0, y1 = get_coverage_y_min_max(l, r)
    if not src.is_cuda:
        return src[:, y0:y1, :].to(device, non_blocking=True).contiguous()
    cache = getattr(camera, cache_name, None)
    key = (y0, y1, src.data_ptr(), src._version)
    if cache is None or (cache and cache[0][0][2:] != key[2:]):  # entries are (key, band): another image / new contents
        cache = []
    for k_, band in cache:
        if k_ == key:
            return band
    band = src[:, y0:y1, :].to(device, non_blocking=True).contiguous()
    cache = [(key, band)] + cache[:3]
    try:
        setattr(camera, cache_name, cache)
    except AttributeError:
        pass
    return band


# ------------------------------------------------------------------------------- loss masks (opt-in)
_LOSS_MASKS = [os.environ.get("GSR_LOSS_MASKS", "0") == "1"]


def set_loss_masks(on):
    """Per-pixel loss masks (include/gsraster.h, N1m; GSR_LOSS_MASKS=1 sets the default), off unless asked for.  With the
    switch on, a camera that carries `alpha_mask_backup` (uint8 [H, W] or [1, H, W]: 255 = the pixel counts, 0 = ignore it,
    in between a weight) gets the rows of its band staged into camera.alpha_mask by load_camera_from_cpu_to_all_gpu --
    the same rows, cache and (under distributed_dataset_storage) one more send / receive per task as original_image --
    and batched_loss_computation takes the loss of m x against m gt inside the fused kernels (fused_band_loss_masked,
    with the camera's exposure when a model is set); n stays H*W*3.  A camera without a mask, or the switch off, takes
    the unmasked path call for call.  final_system_loss_computation and evaluation stay unmasked (as they stay
    uncompensated under an exposure model).  A graphed iteration refuses to capture while the switch is on and a camera
    of the batch carries a mask (graphed_step.py)."""
    _LOSS_MASKS[0] = bool(on)


def get_loss_masks():
    return _LOSS_MASKS[0]


def camera_carries_mask(camera):
    """whether the camera has a loss mask SOMEWHERE: alpha_mask_backup on the ranks that hold its pixels; on a rank that
    holds none (distributed_dataset_storage) the dataset sets camera.has_alpha_mask, which wins when present -- every
    rank has to give the same answer, the sends and receives are paired by it"""
    flag = getattr(camera, "has_alpha_mask", None)
    if flag is not None:
        return bool(flag)
    return getattr(camera, "alpha_mask_backup", None) is not None


def _set_mask(camera, band):
    try:
        camera.alpha_mask = band
    except AttributeError:
        if band is not None:
            raise


def load_camera_from_cpu_to_all_gpu(batched_cameras, batched_strategies, gpuid2tasks):
    """camera.original_image <- exactly the uint8 ground-truth rows [row_l*16, min(row_r*16, H)) this rank
    renders.  With `distributed_dataset_storage` only the first rank of a node holds the images and
    sends the other ranks their bands over xGMI (batched isend/irecv).  With set_loss_masks(True),
    camera.alpha_mask <- the same rows of alpha_mask_backup as [1, rows, W] (None for a camera without a mask)."""
    args = utils.get_args()
    dev = _device()
    me = utils.GLOBAL_RANK
    if not args.distributed_dataset_storage or args.local_sampling or utils.DEFAULT_GROUP.size() == 1:
        for (k, l, r) in gpuid2tasks[me]:
            batched_cameras[k].original_image = _band_of(batched_cameras[k], l, r, dev)
        if _LOSS_MASKS[0]:
            for (k, l, r) in gpuid2tasks[me]:
                cam = batched_cameras[k]
                _set_mask(cam, _mask_band_of(cam, l, r, dev) if camera_carries_mask(cam) else None)
        return

    root = utils.get_first_rank_on_cur_node()
    masks_on = _LOSS_MASKS[0]
    ops, bufs, mbufs = [], [], []
    if me == root:
        node = range(root, root + utils.IN_NODE_GROUP.size())
        for g in node:
            for (k, l, r) in gpuid2tasks[g]:
                band = _band_of(batched_cameras[k], l, r, dev)
                if g == me:
                    bufs.append((k, band))
                else:
                    ops.append(dist.P2POp(dist.isend, band, g))
                if masks_on and camera_carries_mask(batched_cameras[k]):  # right behind the task's image, on both sides
                    mband = _mask_band_of(batched_cameras[k], l, r, dev)
                    if g == me:
                        mbufs.append((k, mband))
                    else:
                        ops.append(dist.P2POp(dist.isend, mband, g))
    else:
        for (k, l, r) in gpuid2tasks[me]:
            y0, y1 = get_coverage_y_min_max(l, r)
            buf = torch.empty((3, y1 - y0, utils.IMG_W), dtype=torch.uint8, device=dev)
            bufs.append((k, buf))
            ops.append(dist.P2POp(dist.irecv, buf, root))
            if masks_on and camera_carries_mask(batched_cameras[k]):
                mbuf = torch.empty((1, y1 - y0, utils.IMG_W), dtype=torch.uint8, device=dev)
                mbufs.append((k, mbuf))
                ops.append(dist.P2POp(dist.irecv, mbuf, root))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    for k, band in bufs:
        batched_cameras[k].original_image = band
    if masks_on:
        for (k, l, r) in gpuid2tasks[me]:
            _set_mask(batched_cameras[k], None)
        for k, mband in mbufs:
            _set_mask(batched_cameras[k], mband)


def load_camera_from_cpu_to_all_gpu_for_eval(batched_cameras, batched_strategies, gpuid2tasks):
    """evaluation wants the FULL ground-truth image on every rank (PSNR after the image all-reduce)."""
    args = utils.get_args()
    dev = _device()
    if not args.distributed_dataset_storage or utils.DEFAULT_GROUP.size() == 1:
        for camera in batched_cameras:
            camera.original_image = camera.original_image_backup.to(dev)
        return
    if args.local_sampling:
        # every camera of the batch is held by the rank that sampled it: idx // (bsz / world) (loss_distribution.py:
        # 2339-2365 of the reference scatters from that rank; a broadcast moves the same bytes)
        per_gpu = max(args.bsz // utils.WORLD_SIZE, 1)
        for idx, camera in enumerate(batched_cameras):
            owner = idx // per_gpu
            if camera.original_image_backup is not None:
                camera.original_image = camera.original_image_backup.to(dev)
            else:
                camera.original_image = torch.empty((3, utils.IMG_H, utils.IMG_W), dtype=torch.uint8, device=dev)
            dist.broadcast(camera.original_image, src=owner, group=utils.IN_NODE_GROUP)
        return
    root = utils.get_first_rank_on_cur_node()
    for camera in batched_cameras:
        if utils.GLOBAL_RANK == root:
            camera.original_image = camera.original_image_backup.to(dev)
        else:
            camera.original_image = torch.empty((3, utils.IMG_H, utils.IMG_W), dtype=torch.uint8, device=dev)
        dist.broadcast(camera.original_image, src=root, group=utils.IN_NODE_GROUP)


# ------------------------------------------------------------------------------------- loss
_EXPOSURE_MODEL = [None]


def set_exposure_model(model):
    """model (exposure.ExposureModel) or None.  With a model, batched_loss_computation takes the loss of every camera on
    x' = A x + b with model.of(camera) (fused into the loss kernels: fused_band_loss_exposure) and the backward fills the
    model's gradient; with None (the default) the path is the plain one, call for call.  final_system_loss_computation
    and evaluation stay uncompensated.  A graphed iteration refuses to capture while a model is set (graphed_step.py)."""
    if model is not None and _BILATERAL_GRID[0] is not None:
        raise ValueError(_BOTH_COLOUR_MODELS)
    _EXPOSURE_MODEL[0] = model


def get_exposure_model():
    return _EXPOSURE_MODEL[0]


_BILATERAL_GRID = [None]
_BOTH_COLOUR_MODELS = ("an exposure model (loss_distribution.set_exposure_model) and a bilateral grid "
                       "(loss_distribution.set_bilateral_grid) cannot both be set: the grid contains the exposure's affine "
                       "transform; set one of them to None first")


def set_bilateral_grid(model):
    """model (bilagrid.BilateralGridModel) or None.  With a model, batched_loss_computation passes every camera's rendered
    band through diff_gaussian_rasterization.bilagrid_slice with model.of(camera) and the rank's rows, then calls the loss
    it would have called, plain or masked (a mask therefore applies to the corrected image), and the backward fills the
    model's gradient; with None (the default) the path is the plain one, call for call.  ValueError while an exposure
    model is set (and set_exposure_model refuses while a grid is set): the grid contains the affine transform.
    final_system_loss_computation and evaluation stay uncorrected.  A graphed iteration refuses to capture while a
    model is set (graphed_step.py)."""
    if model is not None and _EXPOSURE_MODEL[0] is not None:
        raise ValueError(_BOTH_COLOUR_MODELS)
    _BILATERAL_GRID[0] = model


def get_bilateral_grid():
    return _BILATERAL_GRID[0]


def _timings_wanted():
    """HIP events around the loss only when somebody reads the timing (workload_division.timings_have_consumer)"""
    from gaussian_renderer.workload_division import timings_have_consumer

    return timings_have_consumer()


def final_system_loss_computation(image, viewpoint_cam, compute_locally, strategy, statistic_collector):
    """-> (Ll1, ssim) partial sums of this rank's row band, each / (H * W * 3); fills
    statistic_collector["forward_loss_time"] (ms) for the load balancer.  Unmasked and uncompensated, whatever
    set_loss_masks / set_exposure_model say (those act on batched_loss_computation only)."""
    assert utils.GLOBAL_RANK in strategy.gpu_ids, "The current gpu must be used to render this camera."
    j = strategy.gpu_ids.index(utils.GLOBAL_RANK)
    y0, y1 = get_coverage_y_min_max(strategy.division_pos[j], strategy.division_pos[j + 1])
    n = utils.get_num_pixels() * 3
    if not image.is_cuda:
        raise RuntimeError("final_system_loss_computation: the rendered band must live on the gfx950 device "
                           "(there is no CPU path)")
    timed = _timings_wanted()
    if timed:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(_current_stream())
    # one HIP kernel each way (include/gsraster.h: gsr_l1_ssim_forward / _backward)
    l1_sum, ssim_sum = _FUSED(image, viewpoint_cam.original_image, y0, y1)
    Ll1, ssim = l1_sum / n, ssim_sum / n
    # no device sync here (the reference synchronises twice per camera, loss_distribution.py:2566,2578):
    # finish_strategy_final resolves the event pair when -- and only when -- the balancer needs it
    if timed:
        ev1.record(_current_stream())
        statistic_collector["_loss_events"] = (ev0, ev1)
    statistic_collector.setdefault("forward_loss_time", 0.0)
    return Ll1, ssim


def batched_loss_computation(batched_image, batched_cameras, batched_compute_locally, batched_strategies,
                             batched_statistic_collector):
    """loss = (1 - lambda) * L1 + lambda * (1 - ssim), summed over the cameras this rank renders
    (x lr_scale_loss); also returns the per-camera [Ll1, ssim] pairs for logging."""
    args = utils.get_args()
    timers = utils.get_timers()
    if timers is not None:
        timers.start("loss_computation")
    total = None
    parts = []
    for image, camera, mask, strategy, stats in zip(batched_image, batched_cameras, batched_compute_locally,
                                                    batched_strategies, batched_statistic_collector):
        if image is None:  # not rendered here
            parts.append([0.0, 0.0])
            continue
        if image.dim() == 0:  # scalar stand-in (< 10 Gaussians): keeps the graph, contributes nothing
            loss = image * 0
            parts.append([loss, 0.0])
        else:
            if not image.is_cuda:
                raise RuntimeError("batched_loss_computation: images must live on the gfx950 device (no CPU path)")
            # the whole band loss in one autograd node (map kernel + finalize); HIP events instead of the
            # reference's two device syncs per camera (loss_distribution.py:2566,2578)
            # (a band-agnostic hipGraph capture, graphed_step.py: the rows are device data and camera.original_image is
            # a capacity-sized buffer that carries the band in its first rows)
            band_rows = getattr(strategy, "_gsr_dyn_band", None)
            if band_rows is None:
                j = strategy.gpu_ids.index(utils.GLOBAL_RANK)
                y0, y1 = get_coverage_y_min_max(strategy.division_pos[j], strategy.division_pos[j + 1])
            else:
                y0 = y1 = 0
            timed = _timings_wanted()
            if timed:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(_current_stream())
            cap = _capturing()
            if cap is not None:  # (a hipGraph capture: device timestamps instead of events, graphed_step.py)
                cap.stamp("loss0", id(stats))
            if _BILATERAL_GRID[0] is not None:
                if band_rows is not None:
                    raise RuntimeError("batched_loss_computation: the bilateral grid takes its band from the host; a "
                                       "band that is device data (a graphed iteration) is not supported")
                image = _BILAGRID_SLICE(image, _BILATERAL_GRID[0].of(camera), y0, y1, image.shape[1])
            model = _EXPOSURE_MODEL[0]
            mask_band = getattr(camera, "alpha_mask", None) if _LOSS_MASKS[0] else None
            if mask_band is not None:
                loss, Ll1, ssim = _FUSED_LOSS_MASKED(image, camera.original_image, mask_band, y0, y1, args.lambda_dssim,
                                                     utils.get_num_pixels() * 3, band_rows,
                                                     None if model is None else model.of(camera))
            elif model is None:
                loss, Ll1, ssim = _FUSED_LOSS(image, camera.original_image, y0, y1, args.lambda_dssim,
                                              utils.get_num_pixels() * 3, band_rows)
            else:
                loss, Ll1, ssim = _FUSED_LOSS_EXPOSURE(image, model.of(camera), camera.original_image, y0, y1,
                                                       args.lambda_dssim, utils.get_num_pixels() * 3, band_rows)
            if cap is not None:
                cap.stamp("loss1", id(stats))
            if timed:
                ev1.record(_current_stream())
                stats["_loss_events"] = (ev0, ev1)
            stats.setdefault("forward_loss_time", 0.0)
            parts.append([Ll1, ssim])
        total = loss if total is None else total + loss
    assert torch.is_tensor(total) and total.dim() == 0, "The loss_sum must be a scalar tensor."
    if timers is not None:
        timers.stop("loss_computation")
    return (total if args.lr_scale_loss == 1.0 else total * args.lr_scale_loss), parts


# ------------------------------------------------------------------------------ depth supervision (opt-in)
def invdepth_l1(invdepth, target, mask=None, y0=0, y1=None):
    """mean(|invdepth - target| * mask) over the rows [y0, y1) of this rank's band -- the official 3DGS depth
    regulariser's L1 on the inverse-depth map render_final leaves in pkg["batched_invdepth"] (gaussian_renderer
    .set_invdepth); `target` the prior's inverse depth, `mask` its validity (None: everywhere), all [1,H,W] or [H,W].
    Four element-wise operations on one channel, in plain torch (extension of this build: the reference has no depth
    loss); the caller multiplies by invdepth_weight(iteration, ...)."""
    if not invdepth.is_cuda:
        raise RuntimeError("invdepth_l1: the map must live on the gfx950 device (there is no CPU path)")
    H = invdepth.shape[-2]
    y1 = H if y1 is None else min(int(y1), H)
    rows = slice(int(y0), y1)
    diff = (invdepth[..., rows, :] - target[..., rows, :].to(invdepth.dtype)).abs()
    if mask is not None:
        diff = diff * mask[..., rows, :].to(invdepth.dtype)
    return diff.mean()


def invdepth_weight(iteration, init=1.0, final=0.01, max_steps=30_000):
    """the official exponential schedule of the depth regulariser's weight (log-linear from `init` at iteration 0 to
    `final` at `max_steps`, constant afterwards; 0 when both ends are 0 or the iteration is negative)"""
    if iteration < 0 or (init == 0.0 and final == 0.0):
        return 0.0
    if init <= 0.0 or final <= 0.0:
        raise ValueError("invdepth_weight: `init` and `final` must both be positive (or both 0)")
    t = min(max(iteration / float(max_steps), 0.0), 1.0)
    return math.exp(math.log(init) * (1.0 - t) + math.log(final) * t)
