"""MI355X-native drop-in for the reference's `diff_gaussian_rasterization` operator module.

Host-side mirror (Python, because the reference's wrapper is Python) of the operator surface the
reference binds for its hot path -- same names, argument meaning and output order -- on top of the
C-ABI of include/gsraster.h (libgsraster.so, hand-written HIP for gfx950):

  GaussianRasterizationSettings        built at gaussian_renderer/__init__.py:930-943
  GaussianRasterizer.preprocess_gaussians   called at gaussian_renderer/__init__.py:949-956
  GaussianRasterizer.render_gaussians       called at gaussian_renderer/__init__.py:1271-1282
  _C.get_block_XY                      arguments/__init__.py:254-257
  _C.get_local2j_ids_bool              gaussian_renderer/workload_division.py:727-738
  load_image_tiles_by_pos / merge_image_tiles_by_pos / _C.get_touched_locally / ... : only dead
  callers in the reference (loss_distribution.py:136-213, workload_division.py:483) -> raise.

PyTorch is used for device memory, streams and autograd plumbing only; every kernel on the path is in
the HIP library and the module refuses to work without it (no CPU / eager fallback).
"""
import contextlib
import ctypes
import os
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.utils._pytree

from . import _lib
from ._lib import check, lib

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "_C", "load_image_tiles_by_pos",
           "merge_image_tiles_by_pos", "set_timing_mode", "fused_l1_ssim_band", "fused_band_loss", "fused_band_loss_exposure", "fused_activations", "pack_camera",
           "preprocess_gaussians_raw_batched", "knn_mean_dist2", "group_rows", "gather_rows", "densify_plan", "densify_move", "exchange_need",
           "exchange_count", "exchange_pack", "exchange_pack_slab", "exchange_unpack", "zeros_async", "scatter_add_rows", "absgrad_rows", "densify_stats",
           "set_tie_order", "scatter_rows", "local_pixels", "GraphCapture", "capturing", "image_metrics", "metrics_from_sums",
           "bilagrid_slice", "bilagrid_tv"]

BLOCK_X, BLOCK_Y, ONE_DIM_BLOCK_SIZE = 16, 16, 256

# how render_gaussians fills cuda_args["stats_collector"]["backward_render_time"]:
#   "sync"  : one HIP-event synchronisation at the end of the backward op -> exact per-call value
#   "stale" : no extra host sync; reports the most recent backward whose events have completed
#   "deferred": like "stale", and additionally leaves the HIP event pairs under the private keys
#             "_fwd_events" / "_bwd_events" so that a cooperating caller (this package's
#             gaussian_renderer.workload_division.finish_strategy_final) resolves exact values with the
#             one sync it performs anyway
#   "off"   : 0.0 (no events recorded)
_TIMING_MODE = "auto"
_last_backward_ms = 0.0


def set_timing_mode(mode):
    global _TIMING_MODE
    assert mode in ("auto", "sync", "stale", "deferred", "off")
    _TIMING_MODE = mode


def _timing_mode():
    if _TIMING_MODE != "auto":
        return _TIMING_MODE
    if torch.distributed.is_available() and torch.distributed.is_initialized() and \
            torch.distributed.get_world_size() > 1:
        return "sync"  # the load balancer consumes the value (workload_division.py:944-998)
    return "stale"


class _KernelTimer:
    """optional HIP-event brackets around each C-ABI call (bench.py's `roofline` leg): events are
    recorded on the stream the kernels are launched on and resolved by the caller after a sync.  Every record
    carries the launch's own sizes (N, P, D, Px, ...), so that bytes and time describe the SAME launches."""

    def __init__(self):
        self.enabled = False
        self.records = {}

    class _Range:
        def __init__(self, owner, name, meta):
            self.owner, self.name, self.meta = owner, name, meta

        def __enter__(self):
            if self.owner.enabled:
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.e1 = torch.cuda.Event(enable_timing=True)
                self.e0.record()
            return self

        def __exit__(self, *exc):
            if self.owner.enabled:
                self.e1.record()
                self.owner.records.setdefault(self.name, []).append((self.e0, self.e1, self.meta))

    def range(self, name, **meta):
        return _KernelTimer._Range(self, name, meta)

    def reset(self):
        self.records = {}

    def summary_ms(self):
        """name -> (launches, mean ms); call after torch.cuda.synchronize()"""
        return {k: (len(v), sum(r[0].elapsed_time(r[1]) for r in v) / len(v)) for k, v in self.records.items() if v}

    def launches(self):
        """name -> list of (ms, meta dict) per launch; call after torch.cuda.synchronize()"""
        return {k: [(r[0].elapsed_time(r[1]), r[2]) for r in v] for k, v in self.records.items() if v}


kernel_timer = _KernelTimer()



# ------------------------------------------------------------------ native GPU-timer logs (--zhx_time)
# The reference's rasterizer writes per-stage GPU times of the logged iterations to
# <log_folder>/gpu_time_ws=<W>_rk=<r>.log when cuda_args["zhx_time"] is "True" (gaussian_renderer/__init__.py:524-538);
# analyze_statistic.py:747-805 parses "it=<n>, ..." headers followed by "<stage name>: <ms> ms" lines and :1972-1991
# lists the stage names.  The same file is written here from HIP events around the C-ABI calls.  Stages this build has
# fused report 0: "24 ...updateTileTouched" = K3 + depth sort + offsets scan (the reference's 24 + 30), "50 SortPairs"
# = emission + tile sort + ranges (its 40 + 50 + 60).
_ZHX_STAGES = ["10 preprocess time", "24 updateDistributedStatLocally.updateTileTouched time", "30 InclusiveSum time",
               "40 duplicateWithKeys time", "50 SortPairs time", "60 identifyTileRanges time", "70 render time",
               "81 sum_n_render time", "82 sum_n_consider time", "83 sum_n_contrib time", "b10 render time",
               "b20 preprocess time"]
_NULL_RANGE = contextlib.nullcontext()


def _zhx_on(ca):
    if not isinstance(ca, dict) or str(ca.get("zhx_time")) != "True" or ca.get("mode") != "train":
        return False
    try:
        it, every = int(ca.get("iteration", -1)), max(int(ca.get("log_interval", 1)), 1)
    except (TypeError, ValueError):
        return False
    return bool(ca.get("log_folder")) and it >= 0 and (every == 1 or it % every == 1)


class _ZhxRange:
    def __init__(self, targets, label):
        self.targets, self.label = targets, label

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record()
        return self

    def __exit__(self, *exc):
        self.e1.record()
        for ca in self.targets:
            ca.setdefault("_zhx_events", []).append((self.label, self.e0, self.e1, 1.0 / len(self.targets)))
            if self.label == "b20 preprocess time":
                _zhx_flush(ca)


def zhx_range(cuda_args, label):
    """HIP-event bracket of one stage for every cuda_args dict (one, or a list for a camera batch) that asks for the
    native timer log on this iteration; a no-op context otherwise"""
    cas = cuda_args if isinstance(cuda_args, (list, tuple)) else (cuda_args,)
    targets = [ca for ca in cas if _zhx_on(ca)]
    return _ZhxRange(targets, label) if targets else _NULL_RANGE


def _zhx_flush(ca):
    events = ca.pop("_zhx_events", [])
    if not events:
        return
    events[-1][2].synchronize()
    ms = dict.fromkeys(_ZHX_STAGES, 0.0)
    for label, e0, e1, share in events:
        ms[label] = ms.get(label, 0.0) + e0.elapsed_time(e1) * share
    os.makedirs(ca["log_folder"], exist_ok=True)
    path = os.path.join(ca["log_folder"], f"gpu_time_ws={ca.get('world_size', '1')}_rk={ca.get('global_rank', '0')}.log")
    with open(path, "a") as f:
        f.write(f"it={ca.get('iteration')}, mode={ca.get('mode')}, mp_rank={ca.get('mp_rank', '0')}\n")
        for label in _ZHX_STAGES:
            f.write(f"{label}: {ms[label]:.6f} ms\n")


def composite_walked(reset=False):
    """-> (K8, K10) list entries walked since the last reset (include/gsraster.h: gsr_composite_walked); synchronous"""
    out = (ctypes.c_ulonglong * 2)()
    check(lib.gsr_composite_walked(out, 1 if reset else 0), "gsr_composite_walked")
    return int(out[0]), int(out[1])


def local_pixels(mask, W, H):
    """number of image pixels inside the tiles marked in `mask` (uint8/bool [TILE_Y*TILE_X]); host-syncing helper for
    bench bookkeeping, called after the timed region"""
    gx, gy = (W + BLOCK_X - 1) // BLOCK_X, (H + BLOCK_Y - 1) // BLOCK_Y
    m = mask.reshape(gy, gx).to(torch.int64).cpu()
    hh = torch.full((gy,), BLOCK_Y, dtype=torch.int64)
    hh[-1] = H - (gy - 1) * BLOCK_Y
    ww = torch.full((gx,), BLOCK_X, dtype=torch.int64)
    ww[-1] = W - (gx - 1) * BLOCK_X
    return int((m * hh[:, None] * ww[None, :]).sum())


def _on(dev):
    """`with torch.cuda.device(dev)` only when `dev` is not already the current device (the guard costs ~10 us per use
    -- hipGetDevice / hipSetDevice pairs -- and every C-ABI call sits in one; one process drives one GPU)"""
    idx = dev.index
    if idx is None or idx == torch._C._cuda_getDevice():
        return _NULL_RANGE
    return torch.cuda.device(dev)


def _ptr(t):
    # a plain int: the prototypes declare c_void_p, ctypes converts (building a c_void_p object per argument was
    # ~60 objects per iteration)
    return t.data_ptr() if t is not None else None


def _stream():
    # the raw handle of the current stream of the current device (torch.cuda.current_stream() builds a Stream object
    # through three Python layers: ~10 us per call, and every C-ABI call needs one)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


_STREAM_OBJECTS = {}
_NO_STREAM_CACHE = os.environ.get("GSR_STREAM_CACHE", "1") == "0"  # env: A/B measurements only


def current_stream(dev=None):
    """torch.cuda.current_stream(dev), without its three Python layers per call (~5-9 us; an eager iteration of one rank
    asks a dozen times -- stream hand-overs, event records): the Stream object of a raw handle is built once"""
    idx = dev.index if (dev is not None and dev.index is not None) else torch._C._cuda_getDevice()
    if _NO_STREAM_CACHE:
        return torch.cuda.current_stream(idx)
    key = (idx, torch._C._cuda_getCurrentRawStream(idx))
    s = _STREAM_OBJECTS.get(key)
    if s is None:
        s = _STREAM_OBJECTS[key] = torch.cuda.current_stream(idx)
    return s


def _f32c(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"diff_gaussian_rasterization: `{name}` must live on the gfx950 device "
                           "(there is no CPU fallback)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


# ------------------------------------------------------------------------------------ K1 / K11
def _grad_triple(g_means2D, g_rgb, g_conic_opacity, P, dev):
    """the three incoming gradients of a preprocess op as (means2D, rgb, conic_opacity, row stride in floats):
    when they are column views of row-major buffers with one common row stride (K10's [P,9] record) they are passed
    through untouched (stride > 0); otherwise dense copies / zeros (stride 0)."""
    gs = (g_means2D, g_rgb, g_conic_opacity)
    if all(g is not None and g.dtype == torch.float32 and g.dim() == 2 and g.shape[0] == P and
           (P <= 1 or (g.stride(1) == 1 and g.stride(0) == gs[0].stride(0))) for g in gs) and P > 1 and \
            gs[0].stride(0) > 4:
        return g_means2D, g_rgb, g_conic_opacity, int(gs[0].stride(0))

    def z(g, cols):
        return torch.zeros((P, cols), dtype=torch.float32, device=dev) if g is None else g.float().contiguous()

    return z(g_means2D, 2), z(g_rgb, 3), z(g_conic_opacity, 4), 0


# ---- anti-aliased splatting (include/gsraster.h: gsr_set_antialiasing) ------------------------------------------------
# The library's switch is process-wide and read per launch; a backward has to run under the mode of ITS forward, whatever
# the setting is by then.  So every forward notes the mode it ran under (ctx.aa, or the last entry of the batched path's
# `meta`), and every K1 / K11 launch of this module goes through _lib_antialiasing(mode) first, which calls into the
# library only when the mode differs from the last one it set.
_ANTIALIASING = [os.environ.get("GSR_ANTIALIASING", "0").strip().lower() not in ("", "0", "false", "off", "no")]
_ANTIALIASING_LIB = [0]  # what the library was last set to (its initial mode is 0)


def set_antialiasing(on):
    """opacity compensation for the 0.3 px^2 dilation of every splat (the 2D Mip filter; include/gsraster.h:
    gsr_set_antialiasing has the definition).  Off by default (the reference's behaviour); the initial value comes from
    GSR_ANTIALIASING.  Takes effect for the forwards that follow; a backward or a fused optimizer step runs under the
    mode of its own forward.  Camera-pose gradients are not implemented under it (NotImplementedError)."""
    _ANTIALIASING[0] = bool(on)


def get_antialiasing():
    """the mode that the next forward will run under"""
    return _ANTIALIASING[0]


def _lib_antialiasing(mode):
    mode = 1 if mode else 0
    if _ANTIALIASING_LIB[0] != mode:
        if lib.gsr_set_antialiasing(mode) < 0:
            raise RuntimeError("gsr_set_antialiasing failed")
        _ANTIALIASING_LIB[0] = mode


def _refuse_camera_grad_under_antialiasing(what):
    if _ANTIALIASING[0]:
        raise NotImplementedError(
            f"{what}: camera tensors (viewmatrix / projmatrix / campos / cams) that require grad together with "
            "set_antialiasing(True) -- the opacity's compensation factor depends on the pose as well, and its camera "
            "gradient is not implemented; detach the camera tensors or switch anti-aliasing off")


def _meta_aa(meta):
    """the anti-aliasing mode at the end of a batched forward's meta (a five-entry meta predates it: off)"""
    return bool(meta[5]) if len(meta) > 5 else False


class _PreprocessGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, shs, opacities, raster_settings, cuda_args):
        rs = raster_settings
        means3D, scales, rotations = _f32c(means3D, "means3D"), _f32c(scales, "scales"), _f32c(rotations, "rotations")
        shs, opacities = _f32c(shs, "shs"), _f32c(opacities, "opacities")
        P = means3D.shape[0]
        M = shs.shape[1] if shs.dim() == 3 else 0
        if shs.dim() != 3 or shs.shape[0] != P or shs.shape[2] != 3:
            raise ValueError(f"shs must be [P, K, 3], got {tuple(shs.shape)}")
        if scales.shape != (P, 3) or rotations.shape != (P, 4) or opacities.numel() != P:
            raise ValueError("scales [P,3], rotations [P,4], opacities [P,1] expected")
        dev = means3D.device
        view = _f32c(rs.viewmatrix, "viewmatrix")
        proj = _f32c(rs.projmatrix, "projmatrix")
        campos = _f32c(rs.campos, "campos")
        means2D = torch.empty((P, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((P,), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        cov3D = torch.empty((P, 6), dtype=torch.float32, device=dev)
        conic_opacity = torch.empty((P, 4), dtype=torch.float32, device=dev)
        rgb = torch.empty((P, 3), dtype=torch.float32, device=dev)
        clamped = torch.empty((P, 3), dtype=torch.uint8, device=dev)
        ctx.cuda_args = cuda_args
        ctx.aa = _ANTIALIASING[0]
        _lib_antialiasing(ctx.aa)
        with _on(dev), kernel_timer.range("preprocess_forward", N=P, B=1, M=M), \
                zhx_range(cuda_args, "10 preprocess time"):
            check(lib.gsr_preprocess_forward(
                P, int(rs.sh_degree), M, _ptr(means3D), _ptr(scales), float(rs.scale_modifier), _ptr(rotations),
                _ptr(shs), _ptr(opacities), _ptr(view), _ptr(proj), _ptr(campos), int(rs.image_width),
                int(rs.image_height), float(rs.tanfovx), float(rs.tanfovy), _ptr(means2D), _ptr(depths), _ptr(radii),
                _ptr(cov3D), _ptr(conic_opacity), _ptr(rgb), _ptr(clamped), _stream()), "gsr_preprocess_forward")
        ctx.raster_settings = rs
        ctx.M = M
        ctx.save_for_backward(means3D, scales, rotations, shs, view, proj, campos, radii, cov3D, clamped)
        ctx.opacities = opacities if ctx.aa else None  # (an input: only K11's anti-aliased form reads it again)
        ctx.mark_non_differentiable(radii, depths)
        return means2D, rgb, conic_opacity, radii, depths

    @staticmethod
    def backward(ctx, g_means2D, g_rgb, g_conic_opacity, g_radii, g_depths):
        rs = ctx.raster_settings
        means3D, scales, rotations, shs, view, proj, campos, radii, cov3D, clamped = ctx.saved_tensors
        P, M = means3D.shape[0], ctx.M
        dev = means3D.device

        g_means2D, g_rgb, g_conic_opacity, gstride = _grad_triple(g_means2D, g_rgb, g_conic_opacity, P, dev)
        d_means3D = torch.empty((P, 3), dtype=torch.float32, device=dev)
        d_scales = torch.empty((P, 3), dtype=torch.float32, device=dev)
        d_rot = torch.empty((P, 4), dtype=torch.float32, device=dev)
        d_shs = torch.empty((P, M, 3), dtype=torch.float32, device=dev)
        d_opac = torch.empty((P, 1), dtype=torch.float32, device=dev)
        _lib_antialiasing(ctx.aa)
        with _on(dev), kernel_timer.range("preprocess_backward", N=P, B=1, M=M), \
                zhx_range(ctx.cuda_args, "b20 preprocess time"):
            tail = (_ptr(view), _ptr(proj), _ptr(campos), int(rs.image_width), int(rs.image_height),
                    float(rs.tanfovx), float(rs.tanfovy), _ptr(radii), _ptr(cov3D), _ptr(clamped), _ptr(g_means2D),
                    _ptr(g_conic_opacity), _ptr(g_rgb), gstride, _ptr(d_means3D), _ptr(d_scales), _ptr(d_rot),
                    _ptr(d_shs), _ptr(d_opac), _stream())
            head = (P, int(rs.sh_degree), M, _ptr(means3D), _ptr(scales), float(rs.scale_modifier), _ptr(rotations),
                    _ptr(shs))
            if ctx.aa:
                check(lib.gsr_preprocess_backward_aa(*head, _ptr(ctx.opacities), *tail), "gsr_preprocess_backward_aa")
            else:
                check(lib.gsr_preprocess_backward(*head, *tail), "gsr_preprocess_backward")
        return d_means3D, d_scales, d_rot, d_shs, d_opac, None, None


class _PreprocessGaussiansRaw(torch.autograd.Function):
    """K1 / K11 taking GaussianModel's RAW parameters; the getters' activations run inside the kernels
    (include/gsraster.h: gsr_preprocess_forward_raw / _backward_raw)."""

    @staticmethod
    def forward(ctx, xyz, scaling, rotation, features_dc, features_rest, opacity, raster_settings, cuda_args):
        rs = raster_settings
        xyz, scaling, rotation = _f32c(xyz, "xyz"), _f32c(scaling, "scaling"), _f32c(rotation, "rotation")
        features_dc, features_rest = _f32c(features_dc, "features_dc"), _f32c(features_rest, "features_rest")
        opacity = _f32c(opacity, "opacity")
        P = xyz.shape[0]
        if features_dc.shape != (P, 1, 3) or features_rest.dim() != 3 or features_rest.shape[0] != P or \
                features_rest.shape[2] != 3 or features_rest.shape[1] < 1:
            raise ValueError("features_dc [P,1,3] and features_rest [P,K-1,3] expected")
        M = 1 + features_rest.shape[1]
        dev = xyz.device
        view, proj, campos = _f32c(rs.viewmatrix, "viewmatrix"), _f32c(rs.projmatrix, "projmatrix"), \
            _f32c(rs.campos, "campos")
        means2D = torch.empty((P, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((P,), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        cov3D = torch.empty((P, 6), dtype=torch.float32, device=dev)
        conic_opacity = torch.empty((P, 4), dtype=torch.float32, device=dev)
        rgb = torch.empty((P, 3), dtype=torch.float32, device=dev)
        clamped = torch.empty((P, 3), dtype=torch.uint8, device=dev)
        ctx.cuda_args = cuda_args
        ctx.aa = _ANTIALIASING[0]
        _lib_antialiasing(ctx.aa)
        with _on(dev), kernel_timer.range("preprocess_forward", N=P, B=1, M=M), \
                zhx_range(cuda_args, "10 preprocess time"):
            check(lib.gsr_preprocess_forward_raw(
                P, int(rs.sh_degree), M, _ptr(xyz), _ptr(scaling), float(rs.scale_modifier), _ptr(rotation),
                _ptr(features_dc), _ptr(features_rest), _ptr(opacity), _ptr(view), _ptr(proj), _ptr(campos),
                int(rs.image_width), int(rs.image_height), float(rs.tanfovx), float(rs.tanfovy), _ptr(means2D),
                _ptr(depths), _ptr(radii), _ptr(cov3D), _ptr(conic_opacity), _ptr(rgb), _ptr(clamped), _stream()),
                "gsr_preprocess_forward_raw")
        ctx.raster_settings, ctx.M = rs, M
        ctx.save_for_backward(xyz, scaling, rotation, features_dc, features_rest, opacity, view, proj, campos, radii,
                              cov3D, clamped)
        ctx.mark_non_differentiable(radii, depths)
        return means2D, rgb, conic_opacity, radii, depths

    @staticmethod
    def backward(ctx, g_means2D, g_rgb, g_conic_opacity, g_radii, g_depths):
        rs = ctx.raster_settings
        xyz, scaling, rotation, f_dc, f_rest, opacity, view, proj, campos, radii, cov3D, clamped = ctx.saved_tensors
        P, M = xyz.shape[0], ctx.M
        dev = xyz.device

        g_means2D, g_rgb, g_conic_opacity, gstride = _grad_triple(g_means2D, g_rgb, g_conic_opacity, P, dev)
        d_xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        d_scaling = torch.empty((P, 3), dtype=torch.float32, device=dev)
        d_rot = torch.empty((P, 4), dtype=torch.float32, device=dev)
        d_dc = torch.empty((P, 1, 3), dtype=torch.float32, device=dev)
        d_rest = torch.empty((P, M - 1, 3), dtype=torch.float32, device=dev)
        d_opac = torch.empty((P, 1), dtype=torch.float32, device=dev)
        _lib_antialiasing(ctx.aa)
        with _on(dev), kernel_timer.range("preprocess_backward", N=P, B=1, M=M), \
                zhx_range(ctx.cuda_args, "b20 preprocess time"):
            check(lib.gsr_preprocess_backward_raw(
                P, int(rs.sh_degree), M, _ptr(xyz), _ptr(scaling), float(rs.scale_modifier), _ptr(rotation),
                _ptr(f_dc), _ptr(f_rest), _ptr(opacity), _ptr(view), _ptr(proj), _ptr(campos), int(rs.image_width),
                int(rs.image_height), float(rs.tanfovx), float(rs.tanfovy), _ptr(radii), _ptr(cov3D), _ptr(clamped),
                _ptr(g_means2D), _ptr(g_conic_opacity), _ptr(g_rgb), gstride, _ptr(d_xyz), _ptr(d_scaling),
                _ptr(d_rot), _ptr(d_dc), _ptr(d_rest), _ptr(d_opac), _stream()), "gsr_preprocess_backward_raw")
        return d_xyz, d_scaling, d_rot, d_dc, d_rest, d_opac, None, None


def pack_camera(raster_settings):
    """[40] float tensor { viewmatrix, projmatrix, campos, tanfovx, tanfovy, 0, 0, 0 } of one camera (device).
    Only `cat` and `float`: differentiable, so the gradient of a record ([B,40], slot `cams` of
    preprocess_gaussians_raw_batched) flows back into viewmatrix / projmatrix / campos tensors that require grad."""
    rs = raster_settings
    dev = rs.viewmatrix.device
    tail = torch.tensor([float(rs.tanfovx), float(rs.tanfovy), 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    return torch.cat([rs.viewmatrix.reshape(16).float(), rs.projmatrix.reshape(16).float(),
                      rs.campos.reshape(3).float(), tail]).contiguous()


# ---- camera (pose) gradients: dL/d(viewmatrix, projmatrix, campos) --------------------------------------------------
def preprocess_backward_cameras(means3D, sh, cams, width, height, sh_degree, radii, cov3D, clamped, g_means2D,
                                g_conic_opacity, g_rgb, gstride=0, workspace=None):
    """-> dL_dcams [B,40] in the layout of `cams` (include/gsraster.h: gsr_preprocess_backward_cams; words 35..39 are
    zero: no tanfov gradients).  `sh`: the activated shs [P,M,3], or the raw pair (features_dc [P,1,3], features_rest
    [P,M-1,3]).  radii [B,P] / clamped [B,P,3] / cov3D [P,6] as saved by the forward; the incoming gradients are
    camera-major, dense (gstride 0) or column views of one [B*P,9] record (gstride 9).  Launched only when a camera
    tensor requires grad; `workspace`: optional uint8 / any tensor of gsr_preprocess_backward_cams_bytes(P, B) bytes."""
    P, B = means3D.shape[0], cams.shape[0]
    dev = means3D.device
    # the kernel addresses every argument by pointer + row stride: anything else would give wrong sums silently
    f32 = [("means3D", means3D, (P, 3)), ("cams", cams, (B, 40)), ("cov3D", cov3D, (P, 6))]
    f32 += [(f"sh[{k}]", t, None) for k, t in enumerate(sh)] if isinstance(sh, (tuple, list)) else [("sh", sh, None)]
    for name, t, shape in f32 + [("radii", radii, (B, P)), ("clamped", clamped, (B, P, 3))]:
        want = {"radii": torch.int32, "clamped": torch.uint8}.get(name, torch.float32)
        if t.dtype != want or not t.is_contiguous() or t.device != dev or (shape and tuple(t.shape) != shape):
            raise ValueError(f"preprocess_backward_cameras: {name} must be a contiguous {want} tensor"
                             f"{' of shape ' + str(shape) if shape else ''} on {dev}")
    for name, t, k in (("g_means2D", g_means2D, 2), ("g_conic_opacity", g_conic_opacity, 4), ("g_rgb", g_rgb, 3)):
        # (may be the first camera's [P,k] slice of one dense [B,P,k] block: the row layout is checked, not the extent)
        if gstride == 0:
            ok = t.is_contiguous()
        else:
            ok = t.dim() == 2 and t.shape[1] == k and (t.shape[0] <= 1 or t.stride() == (gstride, 1))
        if t.dtype != torch.float32 or t.device != dev or not ok:
            raise ValueError(f"preprocess_backward_cameras: {name} must be float32 on {dev}, dense (gstride 0) or "
                             f"[rows,{k}] column views with row stride gstride = {gstride}")
    if isinstance(sh, (tuple, list)):
        f_dc, f_rest = sh
        M = 1 + f_rest.shape[1]
        dc_ptr, dc_stride, rest_ptr, rest_stride = _ptr(f_dc), 3, (_ptr(f_rest) if M > 1 else None), 3 * (M - 1)
    else:
        M = sh.shape[1]
        dc_ptr, dc_stride = _ptr(sh), 3 * M
        rest_ptr, rest_stride = (ctypes.c_void_p(sh.data_ptr() + 12) if M > 1 else None), 3 * M
    nbytes = int(lib.gsr_preprocess_backward_cams_bytes(P, B))
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    d_cams = torch.empty((B, 40), dtype=torch.float32, device=dev)
    with _on(dev), kernel_timer.range("preprocess_backward_camera", N=P, B=B, M=M):
        check(lib.gsr_preprocess_backward_cams(
            P, B, int(sh_degree), M, _ptr(means3D), dc_ptr, dc_stride, rest_ptr, rest_stride, _ptr(cams), int(width),
            int(height), _ptr(radii), _ptr(cov3D), _ptr(clamped), _ptr(g_means2D), _ptr(g_conic_opacity), _ptr(g_rgb),
            int(gstride), _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(d_cams), _stream()),
            "gsr_preprocess_backward_cams")
    return d_cams


def _camera_requires_grad(rs):
    return any(torch.is_tensor(t) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos))


def _single_camera_grads(ctx, means3D, sh, view, proj, campos, radii, cov3D, clamped, g_means2D, g_conic_opacity,
                         g_rgb, gstride):
    """the three camera gradients of a one-camera preprocess node ([4,4], [4,4], [3]; None where not needed)"""
    rs = ctx.raster_settings
    need = ctx.needs_input_grad[ctx.cam_slot:ctx.cam_slot + 3]
    if not any(need):
        return None, None, None
    P = means3D.shape[0]
    cams = pack_camera(rs._replace(viewmatrix=view, projmatrix=proj, campos=campos)).view(1, 40)
    d = preprocess_backward_cameras(means3D, sh, cams, rs.image_width, rs.image_height, rs.sh_degree,
                                    radii.view(1, P), cov3D, clamped.view(1, P, 3), g_means2D, g_conic_opacity, g_rgb,
                                    gstride)[0]
    outs = (d[0:16].view(4, 4), d[16:32].view(4, 4), d[32:35])
    return tuple(o.to(dt).reshape(shape) if n else None for o, n, (dt, shape) in zip(outs, need, ctx.cam_like))


class _PreprocessGaussiansCam(torch.autograd.Function):
    """_PreprocessGaussians with viewmatrix / projmatrix / campos as differentiable tensor inputs (used only when one of
    them requires grad): the same two launches plus gsr_preprocess_backward_cams in the backward."""

    @staticmethod
    def forward(ctx, means3D, scales, rotations, shs, opacities, viewmatrix, projmatrix, campos, raster_settings,
                cuda_args):
        _refuse_camera_grad_under_antialiasing("preprocess_gaussians")
        ctx.cam_slot = 5
        ctx.cam_like = [(t.dtype, t.shape) for t in (viewmatrix, projmatrix, campos)]
        rs = raster_settings._replace(viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos)
        return _PreprocessGaussians.forward(ctx, means3D, scales, rotations, shs, opacities, rs, cuda_args)

    @staticmethod
    def backward(ctx, g_means2D, g_rgb, g_conic_opacity, g_radii, g_depths):
        means3D, scales, rotations, shs, view, proj, campos, radii, cov3D, clamped = ctx.saved_tensors
        g_means2D, g_rgb, g_conic_opacity, gstride = _grad_triple(g_means2D, g_rgb, g_conic_opacity,
                                                                  means3D.shape[0], means3D.device)
        d_cam = _single_camera_grads(ctx, means3D, shs, view, proj, campos, radii, cov3D, clamped, g_means2D,
                                     g_conic_opacity, g_rgb, gstride)
        return _PreprocessGaussians.backward(ctx, g_means2D, g_rgb, g_conic_opacity, g_radii, g_depths)[:5] + \
            d_cam + (None, None)


class _PreprocessGaussiansRawCam(torch.autograd.Function):
    """_PreprocessGaussiansRaw with differentiable camera tensors (see _PreprocessGaussiansCam)."""

    @staticmethod
    def forward(ctx, xyz, scaling, rotation, features_dc, features_rest, opacity, viewmatrix, projmatrix, campos,
                raster_settings, cuda_args):
        _refuse_camera_grad_under_antialiasing("preprocess_gaussians_raw")
        ctx.cam_slot = 6
        ctx.cam_like = [(t.dtype, t.shape) for t in (viewmatrix, projmatrix, campos)]
        rs = raster_settings._replace(viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos)
        return _PreprocessGaussiansRaw.forward(ctx, xyz, scaling, rotation, features_dc, features_rest, opacity, rs,
                                               cuda_args)

    @staticmethod
    def backward(ctx, g_means2D, g_rgb, g_conic_opacity, g_radii, g_depths):
        xyz, scaling, rotation, f_dc, f_rest, opacity, view, proj, campos, radii, cov3D, clamped = ctx.saved_tensors
        g_means2D, g_rgb, g_conic_opacity, gstride = _grad_triple(g_means2D, g_rgb, g_conic_opacity, xyz.shape[0],
                                                                  xyz.device)
        d_cam = _single_camera_grads(ctx, xyz, (f_dc, f_rest), view, proj, campos, radii, cov3D, clamped, g_means2D,
                                     g_conic_opacity, g_rgb, gstride)
        return _PreprocessGaussiansRaw.backward(ctx, g_means2D, g_rgb, g_conic_opacity, g_radii, g_depths)[:6] + \
            d_cam + (None, None)


def _batched_record(grads, B, P):
    """the [B*P, 9] fp32 record whose column blocks 0:2 / 2:5 / 5:9 of rows [kP, (k+1)P) ARE the gradients of camera
    k's means2D / rgb / conic_opacity, or None"""
    g0 = grads[0]
    if g0 is None or g0._base is None:
        return None
    base = g0._base
    if base.dtype != torch.float32 or not base.is_contiguous() or base.numel() != B * P * 9:
        return None
    p0 = base.data_ptr()
    for k in range(B):
        for col, (off, cols) in enumerate(((0, 2), (2, 3), (5, 4))):
            g = grads[5 * k + col]
            if g is None or g._base is not base or tuple(g.shape) != (P, cols) or g.stride() != (9, 1) or \
                    g.data_ptr() != p0 + 4 * (k * P * 9 + off):
                return None
    return base.view(B * P, 9)


# ---- deferred rounding: K10's fp64 sums and row flags handed to the fused K11 + Adam launch as they are ----------
# (include/gsraster.h: gsr_render_backward_sums, gsr_render_record_materialize, gsr_set_deferred_rounding)
# The render op's backward normally ends with a launch that rounds the rows K10 touched into the fp32 record, whose
# column views are the gradients of means2D / rgb / conic_opacity.  When the only reader of those gradients is the
# fused K11 + Adam launch of the same step, that launch reads the sums and flags itself and the rounding launch and
# most of the 67 bytes K11 loads per row and camera are work nobody needs.
#   armed    by the caller of the render op, per view: cuda_args["_gsr_defer_record"] (the gaussian_renderer mirror sets
#            it for a training view at world size 1 without pose gradients and without the inverse-depth map, in a
#            batch of at most DEFER_MAX_CAMERAS views: a larger one ends in the record path anyway), and only
#            when the switch is on, a FusedAdam(fuse_backward=True) that is not sparse is the sink, nothing is being
#            captured and the flags exist.  A hipGraph capture is never armed: the captured body keeps today's launches.
#   record   the views the backward returns are the same tensors as ever, but their memory holds the forward's zeros
#            until materialize() has run; the _DeferredRecord of the view travels in _DEFERRED under the address of the
#            render op's means2D input, where the projection op's backward -- the next node -- picks it up.
#   readers  K11's node checks that each gradient it received IS the record's view (address, shape, strides); then
#            the sums go to the fused launch.  Anything else first runs materialize(): a missing gradient, a pose
#            gradient (K11c reads the record), a sink that declines, the sparse update, a materialized pending
#            backward.  `.grad` of means2D as the mirror keeps it is a lazy_record_view: the first use materializes.
#            A gradient that is neither None nor the view means autograd has already ADDED something to unrounded
#            memory: that raises.
DEFER_MAX_CAMERAS = 8  # cameras one gsr_preprocess_backward_adam_raw_batched_sums launch takes (include/gsraster.h)
_DEFERRED = {}  # data_ptr of the render op's means2D input -> _DeferredRecord, until the projection backward pops it
# counts since import: render backwards that left the rounding out, records rounded afterwards after all, fused launches
# that read sums and flags (camera-launches: a batch of B counts B)
deferred_rounding_stats = {"deferred": 0, "materialized": 0, "fused_from_sums": 0}


def set_deferred_rounding(mode):
    """"env" (GSR_DEFER_ROUNDING, default on), True / "on", False / "off": whether an armed render backward leaves the
    rounding of K10's record to the fused K11 + Adam launch (include/gsraster.h: gsr_set_deferred_rounding)"""
    code = {"env": -1, True: 1, "on": 1, False: 0, "off": 0}.get(mode)
    if code is None:
        raise ValueError('set_deferred_rounding: mode must be "env", True / "on" or False / "off"')
    check(lib.gsr_set_deferred_rounding(code), "gsr_set_deferred_rounding")


def deferred_rounding():
    return bool(lib.gsr_deferred_rounding())


def _defer_armed(cuda_args, P, have_flags):
    """forward of the render op: may this view's backward leave the rounding out?"""
    if not (isinstance(cuda_args, dict) and cuda_args.get("_gsr_defer_record")) or not have_flags or P < 2:
        return False
    if _CAPTURE[0] is not None or not deferred_rounding():
        return False
    sink = deferred_backward_sink()
    return sink is not None and bool(getattr(sink, "fuse_backward", False)) and not getattr(sink, "sparse", False)


class _DeferredRecord:
    """one view's record whose rounding has been left out: (record, fp64 sums, row flags) and the stream K10 ran on"""

    def __init__(self, record, acc64, touched, stream):
        self.record, self.acc64, self.touched, self.stream = record, acc64, touched, stream
        self.materialized = False
        deferred_rounding_stats["deferred"] += 1

    def is_view(self, g, off, cols):
        """g IS columns off : off + cols of the record (same memory, shape and strides)"""
        r = self.record
        return g is not None and g.dtype == torch.float32 and tuple(g.shape) == (r.shape[0], cols) and \
            g.stride() == (9, 1) and g.data_ptr() == r.data_ptr() + 4 * off

    def materialize(self):
        """run the rounding that was left out, once, on the current stream behind K10's"""
        if self.materialized:
            return
        self.materialized = True
        deferred_rounding_stats["materialized"] += 1
        r = self.record
        with _on(r.device):
            if self.stream is not None:
                cur = current_stream(r.device)
                if cur != self.stream:
                    cur.wait_stream(self.stream)
            check(lib.gsr_render_record_materialize(r.shape[0], _ptr(self.acc64), _ptr(self.touched), _ptr(r), 1,
                                                    _stream()), "gsr_render_record_materialize")


_DEFERRED_MAX = 16  # pending records the table holds: twice the cameras one sums launch takes


def _register_deferred(key, entry):
    """file a record for the projection backward.  The table is bounded; the record that has to leave it (a view whose
    projection backward never ran, or a batch of more views than the table holds) is rounded on its way out, so a
    record nobody can find any more is a complete one"""
    while len(_DEFERRED) >= _DEFERRED_MAX:
        _DEFERRED.pop(next(iter(_DEFERRED))).materialize()
    _DEFERRED[key] = entry


def _deferred_of(g):
    """the pending _DeferredRecord whose record tensor g is a column view of, or None"""
    if g is None or not _DEFERRED:
        return None
    p = g.data_ptr()
    for e in _DEFERRED.values():
        lo = e.record.data_ptr()
        if lo <= p < lo + 36 * e.record.shape[0] and not e.materialized:
            return e
    return None


def _take_deferred(key, g):
    """the projection backward's lookup: the record filed under the address of its means2D output, else the one whose
    memory the gradient it received lies in; the entry leaves _DEFERRED"""
    e = _DEFERRED.pop(key, None)
    if e is None:
        e = _deferred_of(g)
        if e is not None:
            for k in [k for k, v in _DEFERRED.items() if v is e]:
                del _DEFERRED[k]
    return e


class _LazyRecordView(torch.Tensor):
    """a view of a record whose rounding is deferred: whatever is done with it first materializes the record"""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        for t in torch.utils._pytree.tree_leaves((args, kwargs)):  # positional, keyword (`other=`, `out=`), nested
            e = getattr(t, "_gsr_deferred", None) if isinstance(t, _LazyRecordView) else None
            if e is not None:
                e.materialize()
        with torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **(kwargs or {}))
        return out.as_subclass(torch.Tensor) if isinstance(out, _LazyRecordView) else out


def lazy_record_view(g):
    """g itself, or -- when g is a view of a record whose rounding is deferred -- the same view as a tensor that
    materializes the record on first use.  For whoever keeps such a gradient to read it later (`means2D.grad`)."""
    e = _deferred_of(g)
    return g if e is None else _lazy_view(g, e)


def _lazy_view(g, entry):
    v = torch.Tensor._make_subclass(_LazyRecordView, g)
    v._gsr_deferred = entry
    return v


# ---- deferred K11: the projection backward handed to an optimizer that fuses it with its step -------------------
# A sink (fused_optim.FusedAdam(fuse_backward=True)) registers itself here.  When the six raw parameters of a
# _PreprocessGaussiansRawBatched node are exactly the tensors the sink optimizes, the node's backward does not launch
# K11: it returns no gradients (`.grad` stays None) and hands the sink everything K11 needs; the sink's step() then
# runs K11 and Adam as ONE kernel (gsr_preprocess_backward_adam_raw_batched) -- or, whenever that is not possible,
# materializes the gradients with the plain K11 and steps as usual.  Opt-in: nothing is deferred without a sink.
_DEFERRED_SINK = [None]  # a weak reference: an optimizer that is dropped stops being the sink


def set_deferred_backward_sink(sink):
    """sink: object with accepts(params) -> bool and offer(PendingProjectionBackward), or None to switch deferral off.
    Held weakly -- a superseded optimizer that nobody references any more cannot swallow a backward."""
    import weakref

    _DEFERRED_SINK[0] = weakref.ref(sink) if sink is not None else None


def deferred_backward_sink():
    ref = _DEFERRED_SINK[0]
    return ref() if ref is not None else None


class PendingProjectionBackward:
    """K11's inputs of one backward pass, alive until the optimizer's step"""

    def __init__(self, params, cams, radii, cov3D, clamped, g_means2D, g_conic_opacity, g_rgb, gstride, meta, tanfov0,
                 deferred=None):
        # deferred: the cameras' _DeferredRecord when the three gradients ARE views of records whose rounding was left
        # out (B == 1: the views themselves; B > 1: g_* are None until materialize() has assembled them)
        self.deferred = deferred
        self.params = params  # xyz, scaling, rotation, features_dc, features_rest, opacity (the saved inputs)
        self.versions = tuple(t._version for t in params)
        self.cams, self.radii, self.cov3D, self.clamped = cams, radii, cov3D, clamped
        self.g_means2D, self.g_conic_opacity, self.g_rgb, self.gstride = g_means2D, g_conic_opacity, g_rgb, gstride
        self.meta, self.tanfov0 = meta, tanfov0
        self.stream = current_stream(params[0].device) if params[0].is_cuda else None

    def join_stream(self):
        """make the current stream wait for the stream the backward ran on (no-op when they are the same)"""
        if self.stream is not None:
            cur = current_stream(self.params[0].device)
            if cur != self.stream:
                cur.wait_stream(self.stream)

    def round_records(self):
        """the gradients as fp32 tensors: runs the rounding that was left out (deferred) and, for a batch, gathers the
        cameras' records into the dense [B,P,.] blocks the kernels read"""
        entries, self.deferred = self.deferred, None
        if entries is None:
            return
        self.join_stream()
        for e in entries:
            e.materialize()
        if len(entries) > 1:
            recs = [e.record for e in entries]
            self.g_means2D = torch.stack([r[:, 0:2] for r in recs])
            self.g_rgb = torch.stack([r[:, 2:5] for r in recs])
            self.g_conic_opacity = torch.stack([r[:, 5:9] for r in recs])
            self.gstride = 0

    def materialize(self):
        """-> the six gradients, computed by the plain K11 (what the node's backward would have returned)"""
        self.join_stream()
        self.round_records()
        return _launch_k11(self.params, self.cams, self.radii, self.cov3D, self.clamped, self.g_means2D,
                           self.g_conic_opacity, self.g_rgb, self.gstride, self.meta, self.tanfov0, None)

    def fused_step(self, exp_avgs, exp_avg_sqs, lrs, beta1s, beta2s, epss, steps, grad_scale, cache=None,
                   sparse=False):
        """K11 + Adam of the six tensors in one launch; arguments in the order of self.params.  `cache`: a dict the
        caller keeps between steps -- the ctypes tables of the moments' addresses and of the betas / eps only change
        when the model is rebuilt, and this call sits on the host's critical path in front of the launch.
        `sparse`: the lazy update over the rows that received a gradient (include/gsraster.h:
        gsr_preprocess_backward_adam_raw_batched_sparse) instead of the dense one; its workspace and the device word
        that receives the number of active rows live in `cache` ("sparse_ws", "num_active"), grow-only and re-made when
        P changes, so a captured iteration allocates nothing new on replay."""
        self.join_stream()
        if self.deferred is not None and (sparse or not deferred_rounding()):
            self.round_records()  # (the sparse launch classifies the rows from the record; the switch went off)
        sums = self.deferred
        xyz, scaling, rotation, f_dc, f_rest, opacity = self.params
        deg, smod, W, H, M = self.meta[:5]
        P, B = xyz.shape[0], self.cams.shape[0]
        VP, D, I64 = ctypes.c_void_p * 6, ctypes.c_double * 6, ctypes.c_int64 * 6
        key = (tuple(t.data_ptr() for t in exp_avgs), tuple(t.data_ptr() for t in exp_avg_sqs), tuple(beta1s),
               tuple(beta2s), tuple(epss))
        tabs = cache.get("tabs") if cache is not None else None
        if tabs is None or tabs[0] != key:
            tabs = (key, VP(*key[0]), VP(*key[1]), D(*beta1s), D(*beta2s), D(*epss))
            if cache is not None:
                cache["tabs"] = tabs
        tf = (ctypes.c_float * 2)(float(self.tanfov0[0]), float(self.tanfov0[1])) \
            if (B == 1 and self.tanfov0 is not None) else None
        cap_ctx = _CAPTURE[0]
        # captured launch: lr / bias corrections come from the capture's device block at execution time, and the launch
        # is a no-op when a capacity check of the same replay has raised the flag word
        dyn, flag = (_ptr(cap_ctx.dyn), _ptr(cap_ctx.flag)) if cap_ctx is not None else (None, None)
        if sums is not None:  # K10's sums and flags of each camera in place of the record's columns
            PB = ctypes.c_void_p * B
            grad_args = [PB(*[e.acc64.data_ptr() for e in sums]), PB(*[e.touched.data_ptr() for e in sums])]
        else:
            grad_args = [_ptr(self.g_means2D), _ptr(self.g_conic_opacity), _ptr(self.g_rgb), self.gstride]
        args = [P, B, deg, M, _ptr(xyz), _ptr(scaling), smod, _ptr(rotation), _ptr(f_dc), _ptr(f_rest), _ptr(opacity),
                _ptr(self.cams), W, H, _ptr(self.radii), _ptr(self.cov3D), _ptr(self.clamped)] + grad_args + \
               [tabs[1], tabs[2], None if cap_ctx is not None else D(*lrs), tabs[3], tabs[4], tabs[5],
                None if cap_ctx is not None else I64(*steps), float(grad_scale)]
        if sums is not None:
            name, timed = "gsr_preprocess_backward_adam_raw_batched_sums", "preprocess_backward_adam"
            args += [tf, dyn, flag]
            deferred_rounding_stats["fused_from_sums"] += B
        elif sparse:
            if cache is None:
                cache = {}
            need = int(lib.gsr_sparse_step_workspace_bytes(P))
            ws = cache.get("sparse_ws")
            if ws is None or ws[0] != P or ws[1].device != xyz.device or ws[1].numel() * 8 < need:
                ws = (P, torch.empty((need + 7) // 8, dtype=torch.int64, device=xyz.device),
                      torch.zeros(1, dtype=torch.int32, device=xyz.device))
                cache["sparse_ws"] = ws
                cache["num_active"] = ws[2]
            name, timed = "gsr_preprocess_backward_adam_raw_batched_sparse", "preprocess_backward_adam_sparse"
            args += [dyn, flag, _ptr(ws[1]), ws[1].numel() * 8, None, _ptr(ws[2])]
        elif cap_ctx is not None:
            name, timed = "gsr_preprocess_backward_adam_raw_batched_dyn", None  # (never timed: captured)
            args += [tf, dyn, flag]
        else:
            name, timed = "gsr_preprocess_backward_adam_raw_batched", "preprocess_backward_adam"
            args += [tf]
        _lib_antialiasing(_meta_aa(self.meta))  # the forward's mode, whatever the setting is by now
        with _on(xyz.device), (kernel_timer.range(timed, N=P, B=B, M=M) if cap_ctx is None else _NULL_RANGE):
            check(getattr(lib, name)(*args, _stream()), name)


def _launch_k11(params, cams, radii, cov3D, clamped, g_means2D, g_conic_opacity, g_rgb, gstride, meta, tanfov0,
                cuda_args_list):
    xyz, scaling, rotation, f_dc, f_rest, opacity = params
    deg, smod, W, H, M = meta[:5]
    _lib_antialiasing(_meta_aa(meta))  # the forward's mode, whatever the setting is by now
    P, B = xyz.shape[0], cams.shape[0]
    dev = xyz.device
    d_xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
    d_scaling = torch.empty((P, 3), dtype=torch.float32, device=dev)
    d_rot = torch.empty((P, 4), dtype=torch.float32, device=dev)
    d_dc = torch.empty((P, 1, 3), dtype=torch.float32, device=dev)
    d_rest = torch.empty((P, M - 1, 3), dtype=torch.float32, device=dev)
    d_opac = torch.empty((P, 1), dtype=torch.float32, device=dev)
    with _on(dev), kernel_timer.range("preprocess_backward", N=P, B=B, M=M), \
            zhx_range(cuda_args_list, "b20 preprocess time"):
        if B == 1 and tanfov0 is not None:
            # single camera: the leaner one-camera kernel (no accumulators); camera fields are slices of `cams`
            base = cams.data_ptr()
            check(lib.gsr_preprocess_backward_raw(
                P, deg, M, _ptr(xyz), _ptr(scaling), smod, _ptr(rotation), _ptr(f_dc), _ptr(f_rest),
                _ptr(opacity), ctypes.c_void_p(base), ctypes.c_void_p(base + 64), ctypes.c_void_p(base + 128), W,
                H, float(tanfov0[0]), float(tanfov0[1]), _ptr(radii), _ptr(cov3D), _ptr(clamped),
                _ptr(g_means2D), _ptr(g_conic_opacity), _ptr(g_rgb), gstride, _ptr(d_xyz), _ptr(d_scaling),
                _ptr(d_rot), _ptr(d_dc), _ptr(d_rest), _ptr(d_opac), _stream()), "gsr_preprocess_backward_raw")
        else:
            check(lib.gsr_preprocess_backward_raw_batched(
                P, B, deg, M, _ptr(xyz), _ptr(scaling), smod, _ptr(rotation), _ptr(f_dc), _ptr(f_rest),
                _ptr(opacity), _ptr(cams), W, H, _ptr(radii), _ptr(cov3D), _ptr(clamped), _ptr(g_means2D),
                _ptr(g_conic_opacity), _ptr(g_rgb), gstride, _ptr(d_xyz), _ptr(d_scaling), _ptr(d_rot),
                _ptr(d_dc), _ptr(d_rest), _ptr(d_opac), _stream()), "gsr_preprocess_backward_raw_batched")
    return d_xyz, d_scaling, d_rot, d_dc, d_rest, d_opac


class _PreprocessGaussiansRawBatched(torch.autograd.Function):
    """K1 / K11 for a batch of B cameras in one launch each way (gsr_preprocess_*_raw_batched)."""

    @staticmethod
    def forward(ctx, xyz, scaling, rotation, features_dc, features_rest, opacity, cams, sh_degree, scale_modifier,
                width, height, tanfov0, cuda_args_list=None):
        xyz, scaling, rotation = _f32c(xyz, "xyz"), _f32c(scaling, "scaling"), _f32c(rotation, "rotation")
        features_dc, features_rest = _f32c(features_dc, "features_dc"), _f32c(features_rest, "features_rest")
        opacity, cams = _f32c(opacity, "opacity"), _f32c(cams, "cams")
        ctx.tanfov0 = tanfov0
        ctx.cuda_args_list = cuda_args_list
        ctx.set_materialize_grads(False)  # unused outputs arrive as None, not as zero-filled tensors
        P, B = xyz.shape[0], cams.shape[0]
        if cams.dim() != 2 or cams.shape[1] != 40:
            raise ValueError("cams must be [B, 40]")
        M = 1 + features_rest.shape[1]
        dev = xyz.device
        aa = _ANTIALIASING[0]
        if aa and ctx.needs_input_grad[6]:
            _refuse_camera_grad_under_antialiasing("preprocess_gaussians_raw_batched")
        _lib_antialiasing(aa)
        means2D = torch.empty((B, P, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((B, P), dtype=torch.float32, device=dev)
        radii = torch.empty((B, P), dtype=torch.int32, device=dev)
        cov3D = torch.empty((P, 6), dtype=torch.float32, device=dev)
        conic_opacity = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
        rgb = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
        clamped = torch.empty((B, P, 3), dtype=torch.uint8, device=dev)
        with _on(dev), kernel_timer.range("preprocess_forward", N=P, B=B, M=M), \
                zhx_range(cuda_args_list, "10 preprocess time"):
            check(lib.gsr_preprocess_forward_raw_batched(
                P, B, int(sh_degree), M, _ptr(xyz), _ptr(scaling), float(scale_modifier), _ptr(rotation),
                _ptr(features_dc), _ptr(features_rest), _ptr(opacity), _ptr(cams), int(width), int(height),
                _ptr(means2D), _ptr(depths), _ptr(radii), _ptr(cov3D), _ptr(conic_opacity), _ptr(rgb), _ptr(clamped),
                _stream()), "gsr_preprocess_forward_raw_batched")
        ctx.meta = (int(sh_degree), float(scale_modifier), int(width), int(height), M, aa)
        ctx.m2_ptr = means2D.data_ptr()  # (deferred rounding: the key a render op's backward files its record under)
        ctx.save_for_backward(xyz, scaling, rotation, features_dc, features_rest, opacity, cams, radii, cov3D, clamped)
        # per-camera outputs are separate autograd outputs (dense views of the camera-major buffers): a caller
        # that uses camera k alone gets its gradient straight back, without the zeros + copy of a select-backward
        outs = []
        for k in range(B):
            outs += [means2D[k], rgb[k], conic_opacity[k], radii[k], depths[k]]
        ctx.mark_non_differentiable(*[o for i, o in enumerate(outs) if i % 5 >= 3])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        xyz, scaling, rotation, f_dc, f_rest, opacity, cams, radii, cov3D, clamped = ctx.saved_tensors
        deg, smod, W, H, M = ctx.meta[:5]
        P, B = xyz.shape[0], cams.shape[0]
        dev = xyz.device

        def assemble(col, cols):
            """[B,P,cols] gradient buffer of output `col` (0 means2D, 1 rgb, 2 conic_opacity) without copies when
            there is one camera or the per-camera gradients already are the slices of one dense buffer"""
            gs = [grads[5 * k + col] for k in range(B)]
            if B == 1:
                return torch.zeros((1, P, cols), dtype=torch.float32, device=dev) if gs[0] is None \
                    else gs[0].float().contiguous()
            if all(g is not None and g.dtype == torch.float32 and g.is_contiguous() for g in gs):
                base, step = gs[0]._base, P * cols * 4
                if base is not None and all(g._base is base and g.data_ptr() == gs[0].data_ptr() + k * step
                                            for k, g in enumerate(gs)):
                    return gs[0]  # slices of one dense [B,P,cols] block (e.g. an unbound stack gradient)
            out = torch.zeros((B, P, cols), dtype=torch.float32, device=dev)
            for k, g in enumerate(gs):
                if g is not None:
                    out[k].copy_(g)
            return out

        params = (xyz, scaling, rotation, f_dc, f_rest, opacity)
        # records whose rounding the render ops' backward left out (deferred rounding, above): the sums go to the fused
        # launch when every gradient IS its record's view and the sink takes the backward; else they are rounded now
        entries = [_take_deferred(ctx.m2_ptr + 8 * k * P, grads[5 * k]) if _DEFERRED else None for k in range(B)]
        deferred = None
        if any(e is not None for e in entries):
            for k, e in enumerate(entries):
                for col, (off, cols) in enumerate(((0, 2), (2, 3), (5, 4))):
                    g = grads[5 * k + col]
                    if e is not None and g is not None and not e.is_view(g, off, cols):
                        raise RuntimeError(
                            "diff_gaussian_rasterization: the rounding of a view's gradient record was deferred, but "
                            "another gradient reached means2D / rgb / conic_opacity of that view and autograd has added "
                            "it to the unrounded record; call set_deferred_rounding(False) for such a graph")
            whole = all(e is not None and all(grads[5 * k + c] is not None for c in range(3))
                        for k, e in enumerate(entries))
            sink = deferred_backward_sink()
            if whole and not ctx.needs_input_grad[6] and B <= DEFER_MAX_CAMERAS and M == 16 and sink is not None and \
                    not getattr(sink, "sparse", False) and deferred_rounding() and sink.accepts(params):
                deferred = entries
            else:
                for e in entries:
                    if e is not None:
                        e.materialize()
        if deferred is not None and B > 1:
            g_means2D = g_rgb = g_conic_opacity = None  # (PendingProjectionBackward.round_records assembles them)
            gstride = 0
        elif B == 1:  # K10's [P,9] record (or any common-stride column views) goes straight into the kernel
            g_means2D, g_rgb, g_conic_opacity, gstride = _grad_triple(grads[0], grads[1], grads[2], P, dev)
            if deferred is not None:  # (whoever takes these views instead of the sums has the record rounded first)
                g_means2D, g_rgb, g_conic_opacity = (_lazy_view(g, deferred[0])
                                                     for g in (g_means2D, g_rgb, g_conic_opacity))
        else:
            rec = _batched_record(grads, B, P)
            if rec is not None:  # column views of ONE [B,P,9] record (the exchange's backward): read through the stride
                g_means2D, g_rgb, g_conic_opacity, gstride = rec[:, 0:2], rec[:, 2:5], rec[:, 5:9], 9
            else:
                g_means2D, g_rgb, g_conic_opacity, gstride = assemble(0, 2), assemble(1, 3), assemble(2, 4), 0
        d_cams = None
        if ctx.needs_input_grad[6]:  # pose refinement: dL/dcams [B,40], before K11 is launched or handed on
            d_cams = preprocess_backward_cameras(xyz, (f_dc, f_rest), cams, W, H, deg, radii, cov3D, clamped,
                                                 g_means2D, g_conic_opacity, g_rgb, gstride)
        sink = deferred_backward_sink()
        if deferred is not None or (sink is not None and M == 16 and sink.accepts(params)):
            # K11 runs inside the optimizer's step (fused with Adam); `.grad` of the six parameters stays None
            sink.offer(PendingProjectionBackward(params, cams, radii, cov3D, clamped, g_means2D, g_conic_opacity,
                                                 g_rgb, gstride, ctx.meta, ctx.tanfov0, deferred))
            return (None,) * 6 + (d_cams,) + (None,) * 6
        return _launch_k11(params, cams, radii, cov3D, clamped, g_means2D, g_conic_opacity, g_rgb, gstride, ctx.meta,
                           ctx.tanfov0, ctx.cuda_args_list) + (d_cams,) + (None,) * 6


def preprocess_gaussians_raw_batched(xyz, scaling, rotation, features_dc, features_rest, opacity, cams, sh_degree,
                                     scale_modifier, width, height, tanfov0=None, cuda_args_list=None):
    """-> per-camera lists (means2D [P,2], rgb [P,3], conic_opacity [P,4], radii int32 [P], depths [P]) x B for the B
    cameras packed in `cams` [B,40] (pack_camera); entry k of each list is a dense view of a camera-major [B,P,.]
    buffer.  Extension of this build used by the gaussian_renderer mirror."""
    flat = _PreprocessGaussiansRawBatched.apply(xyz, scaling, rotation, features_dc, features_rest, opacity, cams,
                                                sh_degree, scale_modifier, width, height, tanfov0, cuda_args_list)
    return tuple([flat[5 * k + c] for k in range(cams.shape[0])] for c in range(5))


# ------------------------------------------------------------------------------- K3..K8 / K10
def _bucket(nbytes):
    """Round a D-dependent buffer size up to 1/8 of its leading power of two.  The pair count differs from view to
    view, and every new size is a miss of torch's caching allocator -- a hipMalloc (tens of ms for the multi-GB
    buffers of a 4K / 40 M-Gaussian view) inside the iteration; with <= 12.5 % of slack a handful of buckets
    serves every view."""
    if nbytes < (1 << 20):
        return nbytes
    step = 1 << (int(nbytes).bit_length() - 4)
    return (nbytes + step - 1) // step * step


_SORT_SCRATCH = {}  # (device index, stream) -> grow-only uint8 buffer
_MAX_PAIRS = {}     # (device index, stream) -> largest pair count sorted there


def _sort_scratch(nbytes, dev):
    """The sort's ping-pong buffers are dead when gsr_bin_sort's kernels have run, so consecutive calls on one stream
    can share ONE grow-only buffer (stream order makes the reuse safe; another stream gets its own).  Measured on the
    40 M-Gaussian / 4K shape: 260 -> ~30 ms of 'binning' per view were allocator misses on the 22 GB scratch."""
    idx = dev.index if dev.index is not None else torch._C._cuda_getDevice()
    key = (idx, int(torch._C._cuda_getCurrentRawStream(idx)))
    buf = _SORT_SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        _SORT_SCRATCH.pop(key, None)
        buf = None  # drop the old block before asking for the larger one
        buf = torch.empty((_bucket(nbytes),), dtype=torch.uint8, device=dev)
        _SORT_SCRATCH[key] = buf
    return buf


def release_workspaces():
    """drop the cached sort scratch (e.g. before switching to a much smaller scene)"""
    _SORT_SCRATCH.clear()
    _MAX_PAIRS.clear()


_SPECULATIVE_SORT = [os.environ.get("GSR_SPECULATIVE_SORT", "1") != "0"]  # env: A/B measurements only
_SEGMENTS = [{"0": False, "always": "always"}.get(os.environ.get("GSR_SEGMENTS", "1"), True)]  # env: A/B only
_BAND_GRID = [os.environ.get("GSR_BAND_GRID", "1") != "0"]  # env: A/B measurements only
_ZERO_IN_FORWARD = [os.environ.get("GSR_ZERO_IN_FORWARD", "1") != "0"]  # env: A/B measurements only
_KEEP_BACKWARD_BUFFERS = [None]  # tests: a list here receives every composite backward's (record, fp64 sums, row flags)
_TOUCHED_ROWS = [os.environ.get("GSR_TOUCHED_ROWS", "1") != "0"]  # env: A/B measurements only (0: the full rounding pass)


def set_list_segments(on):
    """True (default): on THIN bands (<= 2048 tiles, named by the caller through cuda_args["_gsr_band"]) the composite
    forward leaves checkpoints every 256 walked list entries and the backward runs the segments in parallel workgroups
    (seg_ws of gsr_render_forward / gsr_render_backward); "always": on every launch; False: one workgroup walks a tile's
    whole list"""
    _SEGMENTS[0] = "always" if on == "always" else bool(on)


def set_speculative_sort(on):
    """True (default): launch the tile sort for the scratch's capacity before the pair count has reached the host
    (gsr_bin_sort_bounded); False: the reference's order -- read num_rendered, size the buffers, sort."""
    _SPECULATIVE_SORT[0] = bool(on)


GSR_ERETRY = -3


_PERSIST_USER = [None]  # the mode a caller chose explicitly (None: the environment's)
_LAST_SEGMENTS = [0]    # row segments of the last view binned while kernel_timer was enabled


def set_bin_persistent(mode, _internal=False):
    """K3-K7 as two persistent launches with grid-wide barriers (default) or as the nine launches of the look-back
    pipeline: "env" (GSR_BIN_PERSIST, default on), False / "off", "prepare", "sort", True / "both"
    (include/gsraster.h: gsr_set_bin_persistent).  Lists are bit-identical either way.  A choice made through this
    function is the caller's: the package's own temporary switches (gaussian_renderer: look-back pipeline while an
    exchange overlaps on the side stream) never override it."""
    code = {"env": -1, False: 0, "off": 0, "prepare": 1, "sort": 2, True: 3, "both": 3}[mode]
    if not _internal:
        _PERSIST_USER[0] = None if mode == "env" else mode
    check(lib.gsr_set_bin_persistent(code), "gsr_set_bin_persistent")


def bin_persistent_user_choice():
    """the mode set_bin_persistent was last given by a caller, or None (the environment decides)"""
    return _PERSIST_USER[0]


def set_bin_rowmajor(mode):
    """K5-K7 with one pass over the pairs (csrc/binning_rows.h; include/gsraster.h: gsr_set_bin_rowmajor): "env"
    (GSR_BIN_ROWS, default on), True / "on", False / "off" (the two-pass split-key pipelines).  Same lists either way."""
    code = {"env": -1, False: 0, "off": 0, True: 1, "on": 1}[mode]
    check(lib.gsr_set_bin_rowmajor(code), "gsr_set_bin_rowmajor")


def bin_persist_status():
    """-> dict(done, fault_code, faults, solo_recoveries) of the persistent binning launches on the current device
    (include/gsraster.h: gsr_bin_persist_status).  `solo_recoveries` counts the views whose tile sort was finished by one
    workgroup because the grid did not become resident within the time-out (a shared device); `faults` the barrier
    time-outs that the next binning call reports as an exception (GSR_EFAULT)."""
    w = (ctypes.c_uint32 * 4)()
    check(lib.gsr_bin_persist_status(w), "gsr_bin_persist_status")
    return dict(done=int(w[0]), fault_code=int(w[1]), faults=int(w[2]), solo_recoveries=int(w[3]))


def set_tile_cull(mode):
    """exact tile culling in K3 (include/gsraster.h: gsr_set_tile_cull): "env" (GSR_TILE_CULL, default off), False / "off",
    True / "on", "auto" (on for frames of more than 16384 tiles, i.e. above ~2048 x 2048).  Lists stay order-preserving
    subsequences of the uncut ones; image and gradients unchanged up to the blend's summation order."""
    code = {"env": -1, False: 0, "off": 0, True: 1, "on": 1, "auto": 2}[mode]
    check(lib.gsr_set_tile_cull(code), "gsr_set_tile_cull")


def set_tie_order(order):
    """order of Gaussians with EXACTLY equal depth inside a tile list: "arrival" (default; the reference: index in the
    arrays the op is given, i.e. (source rank, index on the source) at world size > 1) or "position" (means2D.x, .y,
    then index): the image and the gradients then do not depend on the number of ranks or on the order of the
    Gaussians (include/gsraster.h: gsr_set_depth_tie_order)."""
    if order not in ("arrival", "position"):
        raise ValueError('tie order must be "arrival" or "position"')
    check(lib.gsr_set_depth_tie_order(1 if order == "position" else 0), "gsr_set_depth_tie_order")


# ---- an iteration captured in a hipGraph (graphed_step.GraphedIteration) --------------------------------------------
# Inside a capture nothing may reach the host: the pair count is not polled, buffers are sized from the counts of earlier
# (eager) iterations, and the kernels whose capacity may not hold raise bits of the capture's device flag word
# (include/gsraster.h: gsr_flag_if_greater), which turns the optimizer launch of the same replay into a no-op.
FLAG_PAIRS, FLAG_SLAB, FLAG_FEW = 1, 2, 4
_CAPTURE = [None]


class GraphCapture:
    """what the ops need to know while an iteration is being captured (set by graphed_step.GraphedIteration)"""

    def __init__(self, flag, dyn, pair_slack=1.25):
        self.flag, self.dyn, self.pair_slack = flag, dyn, pair_slack  # device uint32 [1], device float32 [12]
        self.pairs = []     # per render op of the iteration: (pinned int32 [1] that receives D, capacity)
        self.counts = None  # (pinned int32 [W*W*B] that receives the exchange's all-gathered counts, caps numpy, shape)
        self.slab_caps_dev = None  # device int32 [W*W*B]: the exchange planner's capacities, uploaded before the capture
        # pinned memory is allocated BEFORE the capture starts (hipHostMalloc is not a capturable call)
        self._words, self._next = torch.zeros((8192,), dtype=torch.int32).pin_memory(), 0
        # device timestamps for the load balancer (include/gsraster.h: gsr_stamp): (pinned int64 ring, slots, words per
        # slot), set by GraphedIteration(timings=True); `stamps` lists what was taken, in launch order, as (kind, tag)
        self.stamp_ring = None
        self.stamps = []

    def stamp(self, kind, tag):
        """a device timestamp at this point of the captured stream (kind: "fwd0" / "fwd1" around K3-K8, "loss0" /
        "loss1" around the loss forward, "bwd0" / "bwd1" around K10; tag: the camera's stats_collector)"""
        if self.stamp_ring is None:
            return
        ring, slots, per = self.stamp_ring
        idx = len(self.stamps)
        if idx >= per:
            raise RuntimeError("graph capture: out of timestamp words")
        check(lib.gsr_stamp(self.dyn.data_ptr() + 48, ring.data_ptr(), slots, per, idx, _stream()), "gsr_stamp")
        self.stamps.append((kind, tag))

    def take_pinned(self, n):
        """-> a pinned int32 view of n words (from the block allocated before the capture)"""
        if self._next + n > self._words.numel():
            raise RuntimeError("graph capture: out of pinned result words")
        v = self._words[self._next:self._next + n]
        self._next += n
        return v

    def pair_capacity(self, dev):
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        seen = max([v for (d, _s), v in _MAX_PAIRS.items() if d == idx], default=0)
        if seen <= 0:
            raise RuntimeError("graph capture: no eager iteration has sorted a view on this device yet")
        return _bucket(4 * int(seen * self.pair_slack + 4096)) // 4


def capturing():
    return _CAPTURE[0]


_DEBUG_RANGES = []  # (GSR_GRAPH_DEBUG=1) buffers of captured iterations: eager allocations must never overlap them


def _debug_overlap(name, t):
    a0, a1 = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
    for n, p, sz in _DEBUG_RANGES:
        if a0 < p + sz and p < a1:
            print(f"[graphed] OVERLAP: eager {name} [{a0:#x}, {a1:#x}) with captured {n} [{p:#x}, {p + sz:#x})",
                  file=__import__("sys").stderr, flush=True)


def _bin_workspaces(means2D, depths, radii, conic_opacity, compute_locally, width, height):
    """what every K3-K7 call starts with -> (P, dev, ranges, prep, args): the range table, the prepare workspace and the
    ten leading arguments of gsr_bin_prepare_async / gsr_bin_speculative_async"""
    P = means2D.shape[0]
    dev = means2D.device
    tiles = ((width + BLOCK_X - 1) // BLOCK_X) * ((height + BLOCK_Y - 1) // BLOCK_Y)
    # tiles + 1 rows: the last one receives the row hull of the mask (the band), which K8 / K10 read through the same
    # pointer; callers see the per-tile rows
    ranges = torch.empty((tiles + 1, 2), dtype=torch.int32, device=dev)[:tiles]
    prep_bytes = lib.gsr_bin_prepare_bytes(P, width, height)
    prep = torch.empty((max(prep_bytes, 4),), dtype=torch.uint8, device=dev)
    args = (P, width, height, _ptr(means2D), _ptr(depths), _ptr(radii), _ptr(conic_opacity), _ptr(compute_locally),
            _ptr(prep), prep_bytes)
    return P, dev, ranges, prep, args


def _bin_gaussians_captured(cap_ctx, means2D, depths, radii, conic_opacity, compute_locally, width, height):
    """K3-K7 inside a hipGraph capture: the tile sort is launched for a CAPACITY taken from earlier iterations, the pair
    count stays on the device (copied to a pinned word the host reads after the replay) and a count above the capacity
    raises FLAG_PAIRS instead of a re-sort.  Returns the capacity as D."""
    P, dev, ranges, prep, args = _bin_workspaces(means2D, depths, radii, conic_opacity, compute_locally, width, height)
    stream = _stream()
    ticket = ctypes.c_uint32(0)
    check(lib.gsr_bin_prepare_async(*args, ctypes.byref(ticket), stream), "gsr_bin_prepare_async")
    cap = cap_ctx.pair_capacity(dev)
    if int(lib.gsr_bin_sort_capacity(P, lib.gsr_bin_sort_bytes(P, cap, width, height), width, height)) < cap:
        raise RuntimeError("graph capture: frames above 256 x 256 tiles have no bounded tile sort")
    sort_bytes = lib.gsr_bin_sort_bytes(P, cap, width, height)
    scratch = torch.empty((max(sort_bytes, 4),), dtype=torch.uint8, device=dev)
    point_list = torch.empty((cap,), dtype=torch.int32, device=dev)
    check(lib.gsr_bin_sort_bounded(P, width, height, _ptr(compute_locally), _ptr(prep), cap, _ptr(scratch), sort_bytes,
                                   _ptr(point_list), _ptr(ranges), stream), "gsr_bin_sort_bounded")
    off = int(lib.gsr_bin_total_offset(P, width, height))
    host = cap_ctx.take_pinned(1)  # the kernel leaves the pair count there (pinned, device-accessible)
    check(lib.gsr_flag_if_greater(prep.data_ptr() + off, cap, _ptr(cap_ctx.flag), FLAG_PAIRS, host.data_ptr(), stream),
          "gsr_flag_if_greater")
    cap_ctx.pairs.append((host, cap))
    if os.environ.get("GSR_GRAPH_DEBUG") == "1":
        _DEBUG_RANGES.extend([("prep", prep.data_ptr(), prep.numel()), ("scratch", scratch.data_ptr(), scratch.numel()),
                              ("point_list", point_list.data_ptr(), 4 * point_list.numel())])
    return point_list, ranges, cap


class PendingPairs:
    """The pair count of a view whose K3-K7 (and, by the time finish() is called, K8) are already in flight (round 6).
    The kernels that consume the lists read the range table, never the count, so the host need not stand between the
    tile sort and the composite kernel: it launches both against the CAPACITY of the kept scratch and looks at the
    count afterwards.  finish() -> (D, new_point_list or None): None when the count fitted the capacity (the lists in
    flight are complete); otherwise the bounded sort wrote nothing and left every range empty (the composite kernel drew
    the background), the tile sort has been repeated HERE with exact sizes into a new point_list, and the caller
    launches its consumer again (same outputs, same stream: stream order makes the repeat invisible to later work)."""

    def __init__(self, ticket, sorted_, cap, P, width, height, mask, prep, ranges, dev, stream, key, cuda_args):
        self.ticket, self.sorted, self.cap = ticket, sorted_, cap
        self.P, self.width, self.height = P, width, height
        self.mask, self.prep, self.ranges = mask, prep, ranges  # (keeps the prepare workspace alive for a repeat)
        self.dev, self.stream, self.key, self.cuda_args = dev, stream, key, cuda_args
        self.D = None

    def finish(self):
        # (the stream guard only when the caller settles from another stream: entering / leaving it is ~15 us of Python)
        same = (not _NO_STREAM_CACHE) and self.stream is current_stream(self.dev)
        with _on(self.dev), (_NULL_RANGE if same else torch.cuda.stream(self.stream)):
            stream = _stream()
            D = ctypes.c_int64(0)
            rc = lib.gsr_bin_count_wait(self.ticket, ctypes.byref(D), stream)
            if rc != GSR_ERETRY:
                check(rc, "gsr_bin_count_wait")
            self.D = D = int(D.value)
            if D > _MAX_PAIRS.get(self.key, 0):
                _MAX_PAIRS[self.key] = D
            if rc == 0 and self.sorted and D <= self.cap:
                self.prep = None
                return D, None
            sort_bytes = lib.gsr_bin_sort_bytes(self.P, D, self.width, self.height)
            scratch = _sort_scratch(max(sort_bytes, 4), self.dev)
            point_list = torch.empty((_bucket(max(D, 1) * 4) // 4,), dtype=torch.int32, device=self.dev)[:max(D, 1)]
            with zhx_range(self.cuda_args, "50 SortPairs time"):
                check(lib.gsr_bin_sort(self.P, self.width, self.height, _ptr(self.mask), _ptr(self.prep), D,
                                       _ptr(scratch), sort_bytes, _ptr(point_list), _ptr(self.ranges), stream),
                      "gsr_bin_sort")
            self.prep = None
            return D, point_list


def bin_gaussians(means2D, depths, radii, conic_opacity, compute_locally, width, height, cuda_args=None, defer=False):
    """K3-K7: returns (point_list uint32-as-int32 [D], ranges int32 [tiles,2], D).  One host read-back (the pair count
    D, like the reference's own num_rendered) -- but the GPU does not wait for it: once a view of this size has been
    sorted, the next sort is launched for the CAPACITY of the scratch kept from then, the kernels take D from device
    memory, and the host reads D while they run (it only re-sorts if D outgrew the capacity).
    `defer` (round 6): do not even read D here -- returns (point_list [capacity], ranges, PendingPairs) and the caller
    calls .finish() after it has launched the consumer of the lists.
    Per tile the list is the reference's (depth, then index) order restricted to the Gaussians that
    can reach alpha >= 1/255 somewhere in the tile's neighbourhood (see include/gsraster.h)."""
    if _CAPTURE[0] is not None:
        return _bin_gaussians_captured(_CAPTURE[0], means2D, depths, radii, conic_opacity, compute_locally, width, height)
    P, dev, ranges, prep, args = _bin_workspaces(means2D, depths, radii, conic_opacity, compute_locally, width, height)
    if _DEBUG_RANGES:
        _debug_overlap("prep", prep)
        _debug_overlap("means2D", means2D)
    stream = _stream()
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(stream.value or 0))
    cap, point_list = 0, None
    kept = _SORT_SCRATCH.get(key)
    if _SPECULATIVE_SORT[0] and kept is not None:
        # pairs the kept scratch can sort, but no more than the largest count seen here plus some slack (point_list
        # is allocated at the capacity)
        cap = min(int(lib.gsr_bin_sort_capacity(P, kept.numel(), width, height)), _bucket(4 * _MAX_PAIRS.get(key, 0)) // 4)
        if cap > 0:
            point_list = torch.empty((cap,), dtype=torch.int32, device=dev)
    ticket, sorted_ = ctypes.c_uint32(0), ctypes.c_int(0)
    if _zhx_on(cuda_args):
        # the native timer log wants the reference's two stages apart (analyze_statistic.py:1972-1991): two host calls
        with zhx_range(cuda_args, "24 updateDistributedStatLocally.updateTileTouched time"):
            check(lib.gsr_bin_prepare_async(*args, ctypes.byref(ticket), stream), "gsr_bin_prepare_async")
        if cap > 0 and ticket.value != 0:
            with zhx_range(cuda_args, "50 SortPairs time"):
                check(lib.gsr_bin_sort_bounded(P, width, height, _ptr(compute_locally), _ptr(prep), cap, _ptr(kept),
                                               kept.numel(), _ptr(point_list), _ptr(ranges), stream),
                      "gsr_bin_sort_bounded")
            sorted_.value = 1
    else:
        # ONE host-side call: K3-K4 and the tile sort at the scratch's capacity (include/gsraster.h)
        check(lib.gsr_bin_speculative_async(*args, cap if cap > 0 else 0, _ptr(kept) if cap > 0 else None,
                                            kept.numel() if cap > 0 else 0, _ptr(point_list) if cap > 0 else None,
                                            _ptr(ranges), ctypes.byref(ticket), ctypes.byref(sorted_), stream),
              "gsr_bin_speculative_async")
    pend = PendingPairs(ticket.value, bool(sorted_.value), cap, P, width, height, compute_locally, prep, ranges, dev,
                        current_stream(dev), key, cuda_args)
    if kernel_timer.enabled and ticket.value:
        # bench.py's instrumented replay only (a device read-back): the row segments R of this view, for the bytes of the
        # row-major pipeline (include/gsraster.h: gsr_bin_segments_offset)
        off = int(lib.gsr_bin_segments_offset(P, width, height))
        _LAST_SEGMENTS[0] = int(prep[off:off + 4].view(torch.int32).item())
    if defer and sorted_.value:
        return point_list, ranges, pend
    D, again = pend.finish()
    if again is not None:
        return again, ranges, D
    return point_list[:max(D, 1)], ranges, D


class _RenderGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2D, conic_opacity, rgb, depths, radii, compute_locally, raster_settings, cuda_args,
                token=None):
        # `token`: an optional 1-element tensor that only ties this node into the caller's autograd graph (the mirror
        # chains its per-camera exchanges through it so that every rank runs their backward collectives in one order)
        ctx.set_materialize_grads(False)
        rs = raster_settings
        means2D, conic_opacity, rgb = _f32c(means2D, "means2D"), _f32c(conic_opacity, "conic_opacity"), _f32c(rgb, "rgb")
        depths = _f32c(depths, "depths")
        if not radii.is_cuda:
            raise RuntimeError("diff_gaussian_rasterization: `radii` must live on the gfx950 device")
        radii = radii.to(torch.int32).contiguous()
        H, W = int(rs.image_height), int(rs.image_width)
        gx, gy = (W + BLOCK_X - 1) // BLOCK_X, (H + BLOCK_Y - 1) // BLOCK_Y
        P = means2D.shape[0]
        dev = means2D.device
        if compute_locally is None:
            mask = torch.ones((gy * gx,), dtype=torch.uint8, device=dev)
        else:
            if compute_locally.numel() != gx * gy:
                raise ValueError(f"compute_locally must have TILE_Y*TILE_X = {gy}x{gx} entries")
            mask = compute_locally.to(device=dev).contiguous().view(-1)
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
        bg = _f32c(rs.bg, "bg")
        # per call (the mirror asks through cuda_args, so a module-wide mode a user chose is never overridden), else
        # the module-wide mode
        timing = (cuda_args.get("_gsr_timing") if isinstance(cuda_args, dict) else None) or _timing_mode()
        if _CAPTURE[0] is not None:
            timing = "off"  # events recorded inside a capture cannot be read
        stats = cuda_args.get("stats_collector") if isinstance(cuda_args, dict) else None
        # opt-in: a ContributionStats the view's per-Gaussian statistics are accumulated into, by a kernel of its own
        # behind K8 (contribution_stats).  The pair count is then NOT deferred: the lists K8 drew from are final before
        # the statistics walk them, and K8 is never redrawn underneath them
        contrib = cuda_args.get("contributions") if isinstance(cuda_args, dict) else None
        if contrib is not None:
            if _CAPTURE[0] is not None:
                raise RuntimeError("diff_gaussian_rasterization: cuda_args['contributions'] is not available under graph "
                                   "capture (the statistics need the view's final lists)")
            if not isinstance(contrib, ContributionStats) or contrib.P != P or \
                    contrib.hits.get_device() != means2D.get_device():
                raise ValueError(f"cuda_args['contributions'] must be a ContributionStats of {P} rows on {dev}")
        # opt-in: the view's lists, mask, band, final_T and n_contrib are left in cuda_args for render_invdepth (the
        # inverse-depth map, a kernel of its own behind K8).  The pair count is then NOT deferred either
        invd = bool(cuda_args.get("invdepth")) if isinstance(cuda_args, dict) else False
        if invd and _CAPTURE[0] is not None:
            raise RuntimeError("diff_gaussian_rasterization: cuda_args['invdepth'] is not available under graph capture "
                               "(the map needs the view's final lists)")
        # opt-in: the same view tuple under a sibling key for render_features (an N-channel feature map, kernels of their
        # own behind K8).  The pair count is then NOT deferred either
        feat = bool(cuda_args.get("features")) if isinstance(cuda_args, dict) else False
        if feat and _CAPTURE[0] is not None:
            raise RuntimeError("diff_gaussian_rasterization: cuda_args['features'] is not available under graph capture "
                               "(the map needs the view's final lists)")
        # opt-in: the backward launches the absolute-gradient kernel behind K10 (gsr_render_absgrad) and leaves its
        # [P,2] result in cuda_args.  The pair count stays deferred: the backward runs on final lists
        ctx.absgrad = bool(cuda_args.get("absgrad")) if isinstance(cuda_args, dict) else False
        if ctx.absgrad and _CAPTURE[0] is not None:
            raise RuntimeError("diff_gaussian_rasterization: cuda_args['absgrad'] is not available under graph capture "
                               "(its result is handed over through cuda_args, outside the captured buffers)")
        with _on(dev):
            if timing != "off":
                ev0 = torch.cuda.Event(enable_timing=True)
                ev1 = torch.cuda.Event(enable_timing=True)
                ev0.record(current_stream(dev))
            if _CAPTURE[0] is not None:
                _CAPTURE[0].stamp("fwd0", id(stats))
            with kernel_timer.range("binning", P=P, tiles=gx * gy) as kt:
                # (round 6) the pair count is looked at AFTER K8 has been launched -- by the caller, after ALL its cameras
                # have been launched, when it hands a list through cuda_args["_gsr_pending"] (gaussian_renderer.render_final)
                point_list, ranges, D = bin_gaussians(means2D, depths, radii, conic_opacity, mask, W, H, cuda_args,
                                                      defer=contrib is None and not invd and not feat)
            pend = D if isinstance(D, PendingPairs) else None
            kt.meta["D"] = D = (0 if pend is not None else D)
            if kernel_timer.enabled:
                kt.meta["R"] = _LAST_SEGMENTS[0]
            out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
            final_T = torch.empty((H, W), dtype=torch.float32, device=dev)
            n_contrib = torch.empty((H, W), dtype=torch.int32, device=dev)
            # bench bookkeeping: the launch's local pixel count is derived from the mask AFTER the run (no sync here)
            ctx.px_meta = dict(mask=mask, W=W, H=H) if kernel_timer.enabled else {}
            ctx.cuda_args = cuda_args
            # the tile rows of the caller's band, when it names them (the mirror does: cuda_args["_gsr_band"]; the
            # mask must be false outside): the launches then cover the band's tiles only
            band = cuda_args.get("_gsr_band") if (isinstance(cuda_args, dict) and _BAND_GRID[0]) else None
            row_lo, row_hi = (int(band[0]), int(band[1])) if band else (0, 0)
            # (-1, capacity): the band is device data -- the mask's row hull, left behind the range table by the tile
            # sort -- and the launches are sized for `capacity` tile rows (include/gsraster.h; graphed_step.py)
            band_rows = row_hi if row_lo == -1 else row_hi - row_lo
            thin = 0 < band_rows * gx <= 2048  # at most two rounds of resident workgroups
            # list segments for the backward (include/gsraster.h: seg_ws of gsr_render_forward) when a backward can follow
            # and
            # the band is THIN: measured (profiles/r04_ab_segments.txt) -9 us net on a 1/8 band, nothing on a whole image
            # (its lists finish in staggered rounds anyway) where the checkpoints only cost the forward 4-9 us
            seg_ws, seg_bytes = None, 0
            if any(ctx.needs_input_grad[:3]) and (_SEGMENTS[0] == "always" or (_SEGMENTS[0] and thin)):
                seg_bytes = int(lib.gsr_render_seg_bytes(W, H))
                seg_ws = torch.empty((seg_bytes,), dtype=torch.uint8, device=dev)
            lists = [point_list]  # (a list: a late pair count may replace the point_list, see settle below)
            # K10's [P,9] gradient record (means2D 0:2, rgb 2:5, conic_opacity 5:9) and the [P,9] fp64 sums it is rounded
            # from are allocated HERE when a backward can follow; the sums are cleared by K8's own workgroups
            # (include/gsraster.h: zero_ptr of gsr_render_forward) instead of by a 72 MB fill launch at the head of the
            # backward.  With them, in the same buffer, go the record's own rows and one byte per row that K10 sets
            # where it adds into the row (gsr_render_backward's `touched`): [72 P | 36 P | P, padded to 16] bytes, all
            # cleared
            # here, so that the backward rounds only the rows K10 touched and every other row of the record is the 0.0f
            # the forward left
            record = acc64 = touched = None
            zero_buf, zero_bytes = None, 0
            # deferred rounding (see _DEFERRED): the backward files sums and flags for the fused K11 + Adam launch.  The
            # buffers are the same, record included: leaving its 36 P bytes out of K8's clear measured nothing
            # (profiles/k10_k11_handoff_ab.txt), and a record nobody rounded reads as zeros, not as garbage
            ctx.defer = all(ctx.needs_input_grad[:3]) and _ZERO_IN_FORWARD[0] and \
                _defer_armed(cuda_args, P, _TOUCHED_ROWS[0])
            if any(ctx.needs_input_grad[:3]) and P > 0 and _ZERO_IN_FORWARD[0]:
                if _TOUCHED_ROWS[0]:
                    zero_bytes = 108 * P + ((P + 15) & ~15)
                    zero_buf = torch.empty((zero_bytes,), dtype=torch.uint8, device=dev)
                    acc64 = zero_buf[:72 * P].view(torch.float64).view(P, 9)
                    record = zero_buf[72 * P:108 * P].view(torch.float32).view(P, 9)
                    touched = zero_buf[108 * P:109 * P]
                else:
                    record = torch.empty((P, 9), dtype=torch.float32, device=dev)
                    zero_buf = acc64 = torch.empty((P, 9), dtype=torch.float64, device=dev)
                    zero_bytes = 72 * P
            ctx.record = (record, acc64, touched) if record is not None else None

            def launch_k8(meta_D):
                with kernel_timer.range("composite_forward", P=P, D=meta_D, **ctx.px_meta) as k8t, \
                        zhx_range(cuda_args, "70 render time"):
                    check(lib.gsr_render_forward(P, W, H, _ptr(ranges), _ptr(lists[0]), _ptr(means2D),
                                                 _ptr(conic_opacity), _ptr(rgb), _ptr(mask), _ptr(bg), _ptr(out),
                                                 _ptr(final_T), _ptr(n_contrib), _ptr(seg_ws), seg_bytes, row_lo,
                                                 row_hi, _ptr(zero_buf), zero_bytes, _stream()), "gsr_render_forward")
                return k8t

            k8t = launch_k8(D)
            if contrib is not None:  # the same lists, mask and band, behind K8 on the same stream
                contribution_stats(ranges, lists[0], means2D, conic_opacity, n_contrib, mask, W, H, contrib,
                                   band=(row_lo, row_hi))
            if invd:
                cuda_args[_INVDEPTH_KEY] = (ranges, lists[0], mask, (row_lo, row_hi), final_T, n_contrib, W, H)
            if feat:
                cuda_args[_FEATURES_KEY] = (ranges, lists[0], mask, (row_lo, row_hi), final_T, n_contrib, W, H)
            if _CAPTURE[0] is not None:
                _CAPTURE[0].stamp("fwd1", id(stats))
            ctx.seg = (seg_ws, seg_bytes, row_lo, row_hi)
            ctx.lists = lists
            ctx.num_rendered = D
            _RenderGaussians.last_num_rendered = D
            if pend is not None:
                def settle(ctx=ctx, pend=pend, kt=kt, k8t=k8t, lists=lists):
                    D, again = pend.finish()
                    kt.meta["D"] = k8t.meta["D"] = D
                    ctx.num_rendered = D
                    _RenderGaussians.last_num_rendered = D
                    if again is not None:  # the capacity did not hold: K8 drew the background; draw the view now
                        lists[0] = again
                        with _on(pend.dev), torch.cuda.stream(pend.stream):
                            launch_k8(D)
                    return D

                collector = cuda_args.get("_gsr_pending") if isinstance(cuda_args, dict) else None
                if isinstance(collector, list):  # (the caller settles after its last camera's launches)
                    collector.append(settle)
                else:
                    settle()
            if timing != "off":
                ev1.record(current_stream(dev))
                ctx.fwd_events = (ev0, ev1)
        if stats is not None:
            # placeholders are real floats so that a forward-only caller can read them; the backward
            # replaces them with measured values (workload_division.py:953-957 reads them afterwards)
            stats.setdefault("forward_render_time", 0.0)
            stats.setdefault("backward_render_time", 0.0)
        ctx.raster_settings = rs
        ctx.cuda_args = cuda_args
        ctx.timing = timing
        # the image itself is an input of the segmented backward (the colour behind a boundary is reconstructed from it):
        # saved through autograd, so that an in-place edit of the output raises instead of corrupting gradients, and
        # no ctx -> output -> grad_fn cycle keeps the buffers alive until the cyclic collector runs
        ctx.save_for_backward(means2D, conic_opacity, rgb, mask, bg, ranges, final_T, n_contrib,
                              out if seg_ws is not None else None)
        ctx.mark_non_differentiable(n_contrib)
        return out, n_contrib

    @staticmethod
    def backward(ctx, g_out, _g_ncontrib):
        global _last_backward_ms
        rs = ctx.raster_settings
        means2D, conic_opacity, rgb, mask, bg, ranges, final_T, n_contrib, out_img = ctx.saved_tensors
        point_list = ctx.lists[0]  # (not a saved tensor: a late pair count may have replaced it, see forward)
        H, W = int(rs.image_height), int(rs.image_width)
        P = means2D.shape[0]
        dev = means2D.device
        if g_out is None:
            return None, None, None, None, None, None, None, None, None
        g_out = g_out.float().contiguous()
        # ONE [P,9] record (means2D 0:2, rgb 2:5, conic_opacity 5:9): K10 flushes a (tile, Gaussian) pair's nine sums
        # from nine adjacent lanes into one row; K11 and the exchange read the record through its row stride
        # K10 adds the tiles' contributions into [P,9] fp64 sums (cleared by the forward's composite kernel when they
        # were allocated there; a second backward over the same forward -- retain_graph, gradcheck -- takes fresh ones
        # and the fill) and rounds each sum once into the record: on one GPU the record, hence the training step, is
        # reproducible from run to run in practice (fp32 atomic adds made it depend on the order the tiles finished)
        pair, ctx.record = ctx.record, None
        record_is_zero = pair is not None
        if pair is None:  # (no flags: every row is rounded)
            pair = (torch.empty((P, 9), dtype=torch.float32, device=dev),
                    torch.empty((P, 9), dtype=torch.float64, device=dev), None)
        record, acc64, touched = pair
        if _KEEP_BACKWARD_BUFFERS[0] is not None:
            _KEEP_BACKWARD_BUFFERS[0].append(pair)
        d_means2D, d_rgb, d_conic_opacity = record[:, 0:2], record[:, 2:5], record[:, 5:9]
        timing = ctx.timing
        with _on(dev):
            if timing != "off":
                ev0 = torch.cuda.Event(enable_timing=True)
                ev1 = torch.cuda.Event(enable_timing=True)
                ev0.record(current_stream(dev))
            cap_stats = ctx.cuda_args.get("stats_collector") if isinstance(ctx.cuda_args, dict) else None
            if _CAPTURE[0] is not None:
                _CAPTURE[0].stamp("bwd0", id(cap_stats))
            defer = record_is_zero and getattr(ctx, "defer", False)
            with kernel_timer.range("composite_backward", P=P, D=ctx.num_rendered, **ctx.px_meta), \
                    zhx_range(ctx.cuda_args, "b10 render time"):
                seg_ws, seg_bytes, row_lo, row_hi = ctx.seg
                if defer:  # K10 alone: the sums and flags are the result
                    check(lib.gsr_render_backward_sums(P, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D),
                                                       _ptr(conic_opacity), _ptr(rgb), _ptr(mask), _ptr(bg),
                                                       _ptr(final_T), _ptr(n_contrib), _ptr(g_out), _ptr(out_img),
                                                       _ptr(seg_ws), seg_bytes, row_lo, row_hi, _ptr(acc64),
                                                       _ptr(touched), _stream()), "gsr_render_backward_sums")
                    entry = _DeferredRecord(record, acc64, touched, current_stream(dev))
                    if _defer_armed(ctx.cuda_args, P, True):
                        _register_deferred(means2D.data_ptr(), entry)
                    else:  # (the switch or the sink changed since the forward)
                        entry.materialize()
                else:
                    check(lib.gsr_render_backward(P, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D),
                                                  _ptr(conic_opacity), _ptr(rgb), _ptr(mask), _ptr(bg), _ptr(final_T),
                                                  _ptr(n_contrib), _ptr(g_out), _ptr(record), _ptr(out_img),
                                                  _ptr(seg_ws), seg_bytes, row_lo, row_hi,
                                                  1 if record_is_zero else 0, _ptr(acc64), _ptr(touched), _stream()),
                          "gsr_render_backward")
            if getattr(ctx, "absgrad", False):
                # the same lists, mask, band, final_T, n_contrib and dL/dpixels, behind K10 on the same stream; the
                # record (rounded or not) is not read
                absg = torch.empty((P, 2), dtype=torch.float32, device=dev)
                abs64 = torch.empty((P, 2), dtype=torch.float64, device=dev)
                with kernel_timer.range("composite_absgrad", P=P):
                    check(lib.gsr_render_absgrad(P, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D),
                                                 _ptr(conic_opacity), _ptr(rgb), _ptr(mask), _ptr(bg), _ptr(final_T),
                                                 _ptr(n_contrib), _ptr(g_out), row_lo, row_hi, _ptr(absg), _ptr(abs64),
                                                 _stream()), "gsr_render_absgrad")
                ctx.cuda_args[_ABSGRAD_KEY] = absg
            if _CAPTURE[0] is not None:
                _CAPTURE[0].stamp("bwd1", id(cap_stats))
            if timing != "off":
                ev1.record(current_stream(dev))
        stats = ctx.cuda_args.get("stats_collector") if isinstance(ctx.cuda_args, dict) else None
        if stats is not None and timing != "off":
            f0, f1 = ctx.fwd_events
            if timing == "sync":
                ev1.synchronize()
                _last_backward_ms = float(ev0.elapsed_time(ev1))
                stats["forward_render_time"] = float(f0.elapsed_time(f1))
                stats["backward_render_time"] = _last_backward_ms
            else:  # "stale" / "deferred": never wait for the device here
                if timing == "deferred":
                    stats["_fwd_events"] = (f0, f1)
                    stats["_bwd_events"] = (ev0, ev1)
                if f1.query():
                    stats["forward_render_time"] = float(f0.elapsed_time(f1))
                pend = getattr(_RenderGaussians, "_pending", None)
                if pend is not None and pend[1].query():
                    _last_backward_ms = float(pend[0].elapsed_time(pend[1]))
                _RenderGaussians._pending = (ev0, ev1)
                stats["backward_render_time"] = float(_last_backward_ms)
        return d_means2D, d_conic_opacity, d_rgb, None, None, None, None, None, None


_ABSGRAD_KEY = "_gsr_absgrad"  # where _RenderGaussians.backward leaves the [P,2] tensor when cuda_args["absgrad"] is set
_INVDEPTH_KEY = "_gsr_invdepth"  # what _RenderGaussians leaves in cuda_args when cuda_args["invdepth"] is set
_FEATURES_KEY = "_gsr_features"  # the same view tuple, left when cuda_args["features"] is set
FEATURES_MAX = 256  # GSR_FEATURES_MAX of include/gsraster.h


class _RenderInvDepth(torch.autograd.Function):
    """the inverse-depth map of a view K8 has drawn (include/gsraster.h: gsr_render_invdepth), from the colour render's
    own lists, mask, band, final_T and n_contrib; backward: the three column groups of the [P,7] record"""

    @staticmethod
    def forward(ctx, means2D, conic_opacity, depths, view):
        if _CAPTURE[0] is not None:
            raise RuntimeError("diff_gaussian_rasterization: the inverse-depth map is not available under graph capture "
                               "(it needs the view's final lists)")
        ranges, point_list, mask, band, final_T, n_contrib, W, H = view
        means2D, conic_opacity = _f32c(means2D, "means2D"), _f32c(conic_opacity, "conic_opacity")
        depths = _f32c(depths, "depths")
        P = means2D.shape[0]
        if conic_opacity.shape[0] != P or depths.numel() != P:
            raise ValueError(f"render_invdepth: means2D, conic_opacity and depths must have the {P} rows of the view")
        dev = means2D.device
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
        with _on(dev), kernel_timer.range("composite_invdepth", P=P):
            check(lib.gsr_render_invdepth(P, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D), _ptr(conic_opacity),
                                          _ptr(depths), _ptr(mask), _ptr(n_contrib), band[0], band[1], _ptr(out),
                                          _stream()), "gsr_render_invdepth")
        ctx.view = view
        ctx.save_for_backward(means2D, conic_opacity, depths, out)
        return out

    @staticmethod
    def backward(ctx, g):
        means2D, conic_opacity, depths, out = ctx.saved_tensors
        ranges, point_list, mask, band, final_T, n_contrib, W, H = ctx.view
        P = means2D.shape[0]
        dev = means2D.device
        g = g.float().contiguous()
        record = torch.empty((P, 7), dtype=torch.float32, device=dev)
        acc64 = torch.empty((P, 7), dtype=torch.float64, device=dev)
        with _on(dev), kernel_timer.range("composite_invdepth_backward", P=P):
            check(lib.gsr_render_invdepth_backward(P, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D),
                                                   _ptr(conic_opacity), _ptr(depths), _ptr(mask), _ptr(n_contrib),
                                                   _ptr(final_T), _ptr(out), _ptr(g), band[0], band[1], _ptr(record),
                                                   _ptr(acc64), _stream()), "gsr_render_invdepth_backward")
        return record[:, 0:2], record[:, 2:6], record[:, 6], None


class _RenderFeatures(torch.autograd.Function):
    """an N-channel feature map of a view K8 has drawn (include/gsraster.h: gsr_render_features), from the colour render's
    own lists, mask, band, final_T and n_contrib; backward: the two column groups of the [P,6] record and, when the
    features require grad, dL/dfeatures [P,C] (otherwise the kernel does not form it)"""

    @staticmethod
    def forward(ctx, means2D, conic_opacity, features, view):
        if _CAPTURE[0] is not None:
            raise RuntimeError("diff_gaussian_rasterization: the feature map is not available under graph capture "
                               "(it needs the view's final lists)")
        ranges, point_list, mask, band, final_T, n_contrib, W, H = view
        means2D, conic_opacity = _f32c(means2D, "means2D"), _f32c(conic_opacity, "conic_opacity")
        features = _f32c(features, "features")
        P = means2D.shape[0]
        if conic_opacity.shape[0] != P or features.dim() != 2 or features.shape[0] != P:
            raise ValueError(f"render_features: means2D, conic_opacity and features [P,C] must have the {P} rows of the "
                             f"view")
        C = int(features.shape[1])
        if not 1 <= C <= FEATURES_MAX:
            raise ValueError(f"render_features: C = {C} channels, the kernels take 1 .. {FEATURES_MAX}")
        dev = means2D.device
        out = torch.empty((C, H, W), dtype=torch.float32, device=dev)
        with _on(dev), kernel_timer.range("composite_features", P=P, C=C):
            check(lib.gsr_render_features(P, C, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D), _ptr(conic_opacity),
                                          _ptr(features), _ptr(mask), _ptr(n_contrib), band[0], band[1], _ptr(out),
                                          _stream()), "gsr_render_features")
        ctx.view = view
        ctx.feature_grad = bool(ctx.needs_input_grad[2])
        ctx.save_for_backward(means2D, conic_opacity, features)
        return out

    @staticmethod
    def backward(ctx, g):
        means2D, conic_opacity, features = ctx.saved_tensors
        ranges, point_list, mask, band, final_T, n_contrib, W, H = ctx.view
        P, C = features.shape
        dev = means2D.device
        g = g.float().contiguous()
        record = torch.empty((P, 6), dtype=torch.float32, device=dev)
        d_feat = torch.empty((P, C), dtype=torch.float32, device=dev) if ctx.feature_grad else None
        acc64 = torch.empty((P, 6 + C if ctx.feature_grad else 6), dtype=torch.float64, device=dev)
        with _on(dev), kernel_timer.range("composite_features_backward", P=P, C=C):
            check(lib.gsr_render_features_backward(P, C, W, H, _ptr(ranges), _ptr(point_list), _ptr(means2D),
                                                   _ptr(conic_opacity), _ptr(features), _ptr(mask), _ptr(n_contrib),
                                                   _ptr(final_T), _ptr(g), band[0], band[1], _ptr(record),
                                                   _ptr(d_feat) if d_feat is not None else None, _ptr(acc64), _stream()),
                  "gsr_render_features_backward")
        return record[:, 0:2], record[:, 2:6], d_feat, None


class _ViewDepths(torch.autograd.Function):
    """K1's `depths` (the same values) with a grad_fn: depth = ([p,1] viewmatrix)[2], so dL/dmeans3D = dL/ddepth times
    the third column of the view matrix (gsr_depth_backward_means3d).  The projection ops themselves keep `depths`
    non-differentiable; this node is only built by a caller that supervises depth."""

    @staticmethod
    def forward(ctx, means3D, viewmatrix, depths, radii):
        if ctx.needs_input_grad[0]:
            sink = deferred_backward_sink()
            if sink is not None and getattr(sink, "fuse_backward", False):
                raise ValueError("the inverse-depth map's gradient needs an optimizer with fuse_backward=False: the "
                                 "fused K11 + Adam step never writes the xyz gradient the depth path is added to")
        if not (means3D.is_cuda and depths.is_cuda and radii.is_cuda):
            raise RuntimeError("diff_gaussian_rasterization: tensors must live on the gfx950 device (no CPU fallback)")
        ctx.save_for_backward(viewmatrix, radii)
        ctx.P = means3D.shape[0]
        return depths.view_as(depths)

    @staticmethod
    def backward(ctx, g):
        viewmatrix, radii = ctx.saved_tensors
        P = ctx.P
        dev = g.device
        if g.dtype != torch.float32 or g.dim() != 1 or (P > 1 and g.stride(0) < 1):
            g = g.float().contiguous().view(-1)
        stride = int(g.stride(0)) if P > 1 else 1
        view = viewmatrix.detach().to(device=dev, dtype=torch.float32).contiguous()
        radii = radii.to(torch.int32).contiguous()
        out = torch.empty((P, 3), dtype=torch.float32, device=dev)
        with _on(dev):
            check(lib.gsr_depth_backward_means3d(P, _ptr(radii), _ptr(view), _ptr(g), stride, _ptr(out), 1, _stream()),
                  "gsr_depth_backward_means3d")
        return out, None, None, None


class GaussianRasterizer(nn.Module):
    """one instance per camera per iteration (gaussian_renderer/__init__.py:945)."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def preprocess_gaussians(self, means3D, scales, rotations, shs, opacities, cuda_args=None):
        """-> (means2D [N,2], rgb [N,3], conic_opacity [N,4], radii int32 [N], depths [N]);
        radii == 0 <=> culled.  means2D supports .retain_grad(); its gradient is in NDC-scaled units
        (pixel gradient x (W/2, H/2)), the convention densification thresholds against
        (scene/gaussian_model.py:1046-1064).  When raster_settings.viewmatrix / projmatrix / campos require grad
        they receive their gradients too (pose refinement; one more launch in the backward, only then)."""
        rs = self.raster_settings
        if _camera_requires_grad(rs):
            return _PreprocessGaussiansCam.apply(means3D, scales, rotations, shs, opacities, rs.viewmatrix,
                                                 rs.projmatrix, rs.campos, rs, cuda_args)
        return _PreprocessGaussians.apply(means3D, scales, rotations, shs, opacities, self.raster_settings, cuda_args)

    def preprocess_gaussians_raw(self, xyz, scaling, rotation, features_dc, features_rest, opacity, cuda_args=None):
        """same outputs as preprocess_gaussians, from GaussianModel's RAW parameters (_xyz, _scaling, _rotation,
        _features_dc, _features_rest, _opacity): the getters' exp / normalize / sigmoid / cat are fused into the
        kernels.  Extension of this build (the reference's op takes activated tensors).  Camera tensors that require
        grad receive their gradients as in preprocess_gaussians."""
        rs = self.raster_settings
        if _camera_requires_grad(rs):
            return _PreprocessGaussiansRawCam.apply(xyz, scaling, rotation, features_dc, features_rest, opacity,
                                                    rs.viewmatrix, rs.projmatrix, rs.campos, rs, cuda_args)
        return _PreprocessGaussiansRaw.apply(xyz, scaling, rotation, features_dc, features_rest, opacity,
                                             self.raster_settings, cuda_args)

    def render_gaussians(self, means2D, conic_opacity, rgb, depths, radii, compute_locally,
                         extended_compute_locally=None, cuda_args=None):
        """-> (image [3,H,W], n_render, n_consider, n_contrib).  Pixels of tiles with
        compute_locally == False are exactly 0.  The last three values are debug statistics the
        reference's callers discard (gaussian_renderer/__init__.py:1271): n_render = number of
        (tile, Gaussian) pairs as a Python int (0 when the caller collects the late pair counts itself through
        cuda_args["_gsr_pending"]: the count is then known when it settles them), n_consider = None, n_contrib =
        per-pixel int32 map."""
        if cuda_args is None:
            cuda_args = {}
        fn = _RenderGaussians
        token = cuda_args.get("_exchange_token") if isinstance(cuda_args, dict) else None
        image, n_contrib = fn.apply(means2D, conic_opacity, rgb, depths, radii, compute_locally,
                                    self.raster_settings, cuda_args, token)
        return image, getattr(fn, "last_num_rendered", None), None, n_contrib

    def render_invdepth(self, means2D, conic_opacity, depths, cuda_args, means3D=None, radii=None):
        """-> the view's inverse-depth map [H,W] (extension of this build; include/gsraster.h: gsr_render_invdepth): per
        pixel the sum of alpha T / depth over what render_gaussians blended, no background term, exactly 0 outside the
        locally computed tiles.  Call it after render_gaussians of the SAME view and rows with cuda_args["invdepth"]
        set: the colour render leaves its lists, mask, band, final_T and n_contrib in `cuda_args`.  Differentiable in
        means2D and conic_opacity (added to K10's gradients by autograd) and, when `means3D` and `radii` (the rows K1
        projected, the same P) are given, in means3D through the depth (depths = ([p,1] viewmatrix)[2])."""
        view = cuda_args.get(_INVDEPTH_KEY) if isinstance(cuda_args, dict) else None
        if view is None:
            raise RuntimeError("render_invdepth: call render_gaussians of the same view with cuda_args['invdepth'] set "
                               "first (it leaves the view's lists and n_contrib in cuda_args)")
        if means3D is not None:
            if radii is None:
                raise ValueError("render_invdepth: `means3D` needs the `radii` of the same rows")
            depths = _ViewDepths.apply(means3D, self.raster_settings.viewmatrix, depths, radii)
        return _RenderInvDepth.apply(means2D, conic_opacity, depths, view)

    def render_features(self, means2D, conic_opacity, features, cuda_args):
        """-> an N-channel feature map [C,H,W] of the view (extension of this build; include/gsraster.h:
        gsr_render_features): per pixel and channel the sum of alpha T f[c] over what render_gaussians blended, no
        background term, exactly 0 outside the locally computed tiles.  `features`: fp32 [P,C], 1 <= C <= FEATURES_MAX.
        Call it after render_gaussians of the SAME view and rows with cuda_args["features"] set: the colour render leaves
        its lists, mask, band, final_T and n_contrib in `cuda_args`.  Differentiable in means2D and conic_opacity (added
        to K10's gradients by autograd) and in `features` when they require grad."""
        view = cuda_args.get(_FEATURES_KEY) if isinstance(cuda_args, dict) else None
        if view is None:
            raise RuntimeError("render_features: call render_gaussians of the same view with cuda_args['features'] set "
                               "first (it leaves the view's lists and n_contrib in cuda_args)")
        return _RenderFeatures.apply(means2D, conic_opacity, features, view)


# ------------------------------------------------------------------------------- N1: fused loss
class _FusedL1SSIMBand(torch.autograd.Function):
    """(sum |band - gt|, sum ssim_map(band, gt)) of rows [y0, y1) of `image` [C,H,W] against the uint8
    ground-truth band [C, y1-y0, W]; the two sums are what final_system_loss_computation divides by
    H*W*3 (gaussian_renderer/loss_distribution.py:2567-2576)."""

    @staticmethod
    def forward(ctx, image, gt_u8, y0, y1):
        if not image.is_cuda:
            raise RuntimeError("fused_l1_ssim_band: device tensors required (no CPU fallback)")
        image = image.float().contiguous()
        C, H, W = image.shape
        rows = y1 - y0
        gt_u8 = gt_u8.contiguous()
        if gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (C, rows, W):
            raise ValueError(f"gt band must be uint8 [{C},{rows},{W}], got {gt_u8.dtype} {tuple(gt_u8.shape)}")
        dev = image.device
        need_grad = ctx.needs_input_grad[0]
        nb = lib.gsr_l1_ssim_num_partials(C, rows, W)
        partials = torch.empty((max(nb, 1), 2), dtype=torch.float32, device=dev)
        maps = torch.empty((3, C, rows, W), dtype=torch.float32, device=dev) if need_grad else None
        band_ptr = ctypes.c_void_p(image.data_ptr() + 4 * y0 * W)
        with _on(dev), kernel_timer.range("l1_ssim_forward", Px=rows * W):
            check(lib.gsr_l1_ssim_forward(C, rows, W, band_ptr, H * W, _ptr(gt_u8), _ptr(partials),
                                          _ptr(maps[0]) if need_grad else None, _ptr(maps[1]) if need_grad else None,
                                          _ptr(maps[2]) if need_grad else None, _stream()), "gsr_l1_ssim_forward")
        sums = partials[:nb].sum(dim=0)
        ctx.y0, ctx.y1 = y0, y1
        if need_grad:
            ctx.save_for_backward(image, gt_u8, maps)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        image, gt_u8, maps = ctx.saved_tensors
        C, H, W = image.shape
        y0, y1 = ctx.y0, ctx.y1
        rows = y1 - y0
        dev = image.device
        g_l1 = (torch.zeros((), device=dev) if g_l1 is None else g_l1).float().contiguous()
        g_ssim = (torch.zeros((), device=dev) if g_ssim is None else g_ssim).float().contiguous()
        grad = torch.empty_like(image) if rows == H else torch.zeros_like(image)
        band_ptr = ctypes.c_void_p(image.data_ptr() + 4 * y0 * W)
        gband_ptr = ctypes.c_void_p(grad.data_ptr() + 4 * y0 * W)
        with _on(dev), kernel_timer.range("l1_ssim_backward", Px=rows * W):
            check(lib.gsr_l1_ssim_backward(C, rows, W, band_ptr, H * W, _ptr(gt_u8), _ptr(maps[0]), _ptr(maps[1]),
                                           _ptr(maps[2]), _ptr(g_l1), _ptr(g_ssim), 1.0, 1.0, gband_ptr, H * W,
                                           _stream()),
                  "gsr_l1_ssim_backward")
        return grad, None, None, None


def fused_l1_ssim_band(image, gt_u8, y0, y1):
    """-> (sum of |x - gt/255| , sum of the SSIM map) over rows [y0, y1) of image [C,H,W]"""
    return _FusedL1SSIMBand.apply(image, gt_u8, int(y0), int(y1))


class _FusedBandLoss(torch.autograd.Function):
    """loss = (1 - lambda) * Ll1 + lambda * (1 - ssim) of one rendered row band, Ll1 = sum|x - gt| / n and
    ssim = sum(ssim_map) / n with n = H*W*3 of the FULL image (gaussian_renderer/loss_distribution.py:2567-2576,
    2627-2629), as two launches forward (map kernel + finalize) and two backward (scalar scale + map kernel) --
    the reference's ~30 elementwise launches around its conv2d-based maps are gone.  Returns
    (loss, Ll1, ssim); the last two are detached (logging only)."""

    _coef_cache = {}

    @staticmethod
    def forward(ctx, image, gt_u8, y0, y1, lambda_dssim, n, band_rows=None):
        if not image.is_cuda:
            raise RuntimeError("fused_band_loss: device tensors required (no CPU fallback)")
        ctx.set_materialize_grads(False)
        image = image.float().contiguous()
        C, H, W = image.shape
        gt_u8 = gt_u8.contiguous()
        # band_rows (int32 [2] on the device: { y0, y1 }): the band is DEVICE data, `gt_u8` [C, capacity, W] carries it in
        # the first y1 - y0 rows of every channel and y0 / y1 are not looked at (graphed_step.py: one captured launch for
        # every band; include/gsraster.h: gsr_l1_ssim_forward_band)
        dyn = band_rows is not None
        if dyn and (band_rows.dtype != torch.int32 or not band_rows.is_cuda or band_rows.numel() < 2):
            raise ValueError("band_rows must be an int32 device tensor { y0, y1 }")
        rows = int(gt_u8.shape[1]) if dyn else y1 - y0
        if gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (C, rows, W):
            raise ValueError(f"gt band must be uint8 [{C},{rows},{W}], got {gt_u8.dtype} {tuple(gt_u8.shape)}")
        dev = image.device
        need_grad = ctx.needs_input_grad[0]
        nb = lib.gsr_l1_ssim_num_partials(C, rows, W)
        partials = torch.empty((max(nb, 1), 2), dtype=torch.float32, device=dev)
        maps = torch.empty((3, C, rows, W), dtype=torch.float32, device=dev) if need_grad else None
        out3 = torch.empty((3,), dtype=torch.float32, device=dev)
        c_l1, c_ssim = (1.0 - lambda_dssim) / n, -lambda_dssim / n
        m = [_ptr(maps[i]) if need_grad else None for i in range(3)]
        with _on(dev):
            with kernel_timer.range("l1_ssim_forward", Px=rows * W):
                if dyn:
                    check(lib.gsr_l1_ssim_forward_band(C, rows, W, _ptr(image), H * W, _ptr(gt_u8), _ptr(partials), m[0],
                                                       m[1], m[2], _ptr(band_rows), _stream()),
                          "gsr_l1_ssim_forward_band")
                else:
                    band_ptr = ctypes.c_void_p(image.data_ptr() + 4 * y0 * W)
                    check(lib.gsr_l1_ssim_forward(C, rows, W, band_ptr, H * W, _ptr(gt_u8), _ptr(partials), m[0], m[1],
                                                  m[2], _stream()), "gsr_l1_ssim_forward")
            check(lib.gsr_l1_ssim_finalize(nb, _ptr(partials), c_l1, c_ssim, lambda_dssim, 1.0 / n, _ptr(out3),
                                           _stream()), "gsr_l1_ssim_finalize")
        ctx.y0, ctx.y1, ctx.coef, ctx.band_rows = y0, y1, (c_l1, c_ssim), band_rows
        if need_grad:
            ctx.save_for_backward(image, gt_u8, maps)
        loss, Ll1, ssim = out3[0], out3[1], out3[2]
        ctx.mark_non_differentiable(Ll1, ssim)
        return loss, Ll1, ssim

    @staticmethod
    def backward(ctx, g_loss, _g1, _g2):
        if g_loss is None:
            return None, None, None, None, None, None, None
        image, gt_u8, maps = ctx.saved_tensors
        C, H, W = image.shape
        y0, y1 = ctx.y0, ctx.y1
        dyn = ctx.band_rows is not None
        rows = int(gt_u8.shape[1]) if dyn else y1 - y0
        dev = image.device
        g_loss = g_loss if (g_loss.dtype == torch.float32 and g_loss.is_contiguous()) else g_loss.float().contiguous()
        # (dL/dS_l1, dL/dS_ssim) = dL/dloss * (c_l1, c_ssim): the product is formed inside the kernel
        grad = torch.empty_like(image) if (rows == H and not dyn) else torch.zeros_like(image)
        with _on(dev), kernel_timer.range("l1_ssim_backward", Px=rows * W):
            if dyn:
                check(lib.gsr_l1_ssim_backward_band(C, rows, W, _ptr(image), H * W, _ptr(gt_u8), _ptr(maps[0]),
                                                    _ptr(maps[1]), _ptr(maps[2]), _ptr(g_loss), _ptr(g_loss),
                                                    float(ctx.coef[0]), float(ctx.coef[1]), _ptr(grad), H * W,
                                                    _ptr(ctx.band_rows), _stream()), "gsr_l1_ssim_backward_band")
            else:
                band_ptr = ctypes.c_void_p(image.data_ptr() + 4 * y0 * W)
                gband_ptr = ctypes.c_void_p(grad.data_ptr() + 4 * y0 * W)
                check(lib.gsr_l1_ssim_backward(C, rows, W, band_ptr, H * W, _ptr(gt_u8), _ptr(maps[0]), _ptr(maps[1]),
                                               _ptr(maps[2]), _ptr(g_loss), _ptr(g_loss), float(ctx.coef[0]),
                                               float(ctx.coef[1]), gband_ptr, H * W, _stream()),
                      "gsr_l1_ssim_backward")
        return grad, None, None, None, None, None, None


def fused_band_loss(image, gt_u8, y0, y1, lambda_dssim, n, band_rows=None):
    """-> (loss, Ll1, ssim) of rows [y0, y1) of image [C,H,W]; n = H*W*3 of the full image.  band_rows (int32 [2] on
    the device): the rows are device data and gt_u8 is a [C, capacity, W] buffer (see _FusedBandLoss.forward)"""
    return _FusedBandLoss.apply(image, gt_u8, int(y0), int(y1), float(lambda_dssim), float(n), band_rows)


class _FusedBandLossExposure(torch.autograd.Function):
    """_FusedBandLoss of x' = A x + b, E = [A | b] the [3,4] exposure of the camera (include/gsraster.h, N1x): x' is
    formed inside the forward's staging and recomputed by the backward, which writes dL/dimage = A^T g' and reduces the 12
    sums of dL/dE (per-tile rows + a fixed-order fp64 finalize).  Same launch count as _FusedBandLoss plus that
    finalize; `exposure` is read on the device.  Returns (loss, Ll1, ssim); the last two are detached."""

    @staticmethod
    def forward(ctx, image, exposure, gt_u8, y0, y1, lambda_dssim, n, band_rows=None):
        if not image.is_cuda or not exposure.is_cuda:
            raise RuntimeError("fused_band_loss_exposure: device tensors required (no CPU fallback)")
        ctx.set_materialize_grads(False)
        image = image.float().contiguous()
        C, H, W = image.shape
        if C != 3 or tuple(exposure.shape) != (3, 4):
            raise ValueError(f"exposure compensation needs a [3,H,W] image and a [3,4] exposure, got "
                             f"{tuple(image.shape)} and {tuple(exposure.shape)}")
        exposure = exposure.float().contiguous()
        gt_u8 = gt_u8.contiguous()
        dyn = band_rows is not None
        if dyn and (band_rows.dtype != torch.int32 or not band_rows.is_cuda or band_rows.numel() < 2):
            raise ValueError("band_rows must be an int32 device tensor { y0, y1 }")
        rows = int(gt_u8.shape[1]) if dyn else y1 - y0
        if gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (C, rows, W):
            raise ValueError(f"gt band must be uint8 [{C},{rows},{W}], got {gt_u8.dtype} {tuple(gt_u8.shape)}")
        dev = image.device
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        nb = lib.gsr_l1_ssim_num_partials(C, rows, W)
        partials = torch.empty((max(nb, 1), 2), dtype=torch.float32, device=dev)
        maps = torch.empty((3, C, rows, W), dtype=torch.float32, device=dev) if need_grad else None
        out3 = torch.empty((3,), dtype=torch.float32, device=dev)
        c_l1, c_ssim = (1.0 - lambda_dssim) / n, -lambda_dssim / n
        m = [_ptr(maps[i]) if need_grad else None for i in range(3)]
        with _on(dev):
            with kernel_timer.range("l1_ssim_forward", Px=rows * W):
                img_ptr = _ptr(image) if dyn else ctypes.c_void_p(image.data_ptr() + 4 * y0 * W)
                check(lib.gsr_l1_ssim_forward_exposure(C, rows, W, img_ptr, H * W, _ptr(gt_u8), _ptr(partials), m[0],
                                                       m[1], m[2], _ptr(band_rows), _ptr(exposure), _stream()),
                      "gsr_l1_ssim_forward_exposure")
            check(lib.gsr_l1_ssim_finalize(nb, _ptr(partials), c_l1, c_ssim, lambda_dssim, 1.0 / n, _ptr(out3),
                                           _stream()), "gsr_l1_ssim_finalize")
        ctx.y0, ctx.y1, ctx.coef, ctx.band_rows = y0, y1, (c_l1, c_ssim), band_rows
        if need_grad:
            ctx.save_for_backward(image, exposure, gt_u8, maps)
        loss, Ll1, ssim = out3[0], out3[1], out3[2]
        ctx.mark_non_differentiable(Ll1, ssim)
        return loss, Ll1, ssim

    @staticmethod
    def backward(ctx, g_loss, _g1, _g2):
        if g_loss is None:
            return None, None, None, None, None, None, None, None
        image, exposure, gt_u8, maps = ctx.saved_tensors
        C, H, W = image.shape
        y0, y1 = ctx.y0, ctx.y1
        dyn = ctx.band_rows is not None
        rows = int(gt_u8.shape[1]) if dyn else y1 - y0
        dev = image.device
        g_loss = g_loss if (g_loss.dtype == torch.float32 and g_loss.is_contiguous()) else g_loss.float().contiguous()
        grad = torch.empty_like(image) if (rows == H and not dyn) else torch.zeros_like(image)
        grad_e = torch.empty((3, 4), dtype=torch.float32, device=dev)
        ne = lib.gsr_l1_ssim_exposure_num_partials(rows, W)
        e_partials = torch.empty((max(ne, 1), 12), dtype=torch.float32, device=dev)
        off = 0 if dyn else 4 * y0 * W
        with _on(dev), kernel_timer.range("l1_ssim_backward", Px=rows * W):
            check(lib.gsr_l1_ssim_backward_exposure(C, rows, W, ctypes.c_void_p(image.data_ptr() + off), H * W,
                                                    _ptr(gt_u8), _ptr(maps[0]), _ptr(maps[1]), _ptr(maps[2]),
                                                    _ptr(g_loss), _ptr(g_loss), float(ctx.coef[0]), float(ctx.coef[1]),
                                                    ctypes.c_void_p(grad.data_ptr() + off), H * W, _ptr(ctx.band_rows),
                                                    _ptr(exposure), _ptr(e_partials), _ptr(grad_e), _stream()),
                  "gsr_l1_ssim_backward_exposure")
        return grad, grad_e, None, None, None, None, None, None


def fused_band_loss_exposure(image, exposure, gt_u8, y0, y1, lambda_dssim, n, band_rows=None):
    """fused_band_loss of the exposure-compensated band x' = A x + b (exposure = [A | b], float32 [3,4] on the device;
    include/gsraster.h, N1x) -> (loss, Ll1, ssim), with gradients for `image` and `exposure`"""
    return _FusedBandLossExposure.apply(image, exposure, gt_u8, int(y0), int(y1), float(lambda_dssim), float(n),
                                        band_rows)


class _FusedBandLossMasked(torch.autograd.Function):
    """_FusedBandLoss (exposure None) or _FusedBandLossExposure of the masked band x' = m x, y' = m y, m = mask / 255 per
    pixel (include/gsraster.h, N1m): the mask is applied inside the forward's staging and the backward's recomputation --
    no masked copy of the image, no extra launch.  n stays H*W*3 of the full image.  Returns (loss, Ll1, ssim); the last
    two are detached."""

    @staticmethod
    def forward(ctx, image, gt_u8, mask_u8, y0, y1, lambda_dssim, n, band_rows, exposure):
        expo = exposure is not None
        if not image.is_cuda or not mask_u8.is_cuda or (expo and not exposure.is_cuda):
            raise RuntimeError("fused_band_loss_masked: device tensors required (no CPU fallback)")
        ctx.set_materialize_grads(False)
        image = image.float().contiguous()
        C, H, W = image.shape
        if expo:
            if C != 3 or tuple(exposure.shape) != (3, 4):
                raise ValueError(f"exposure compensation needs a [3,H,W] image and a [3,4] exposure, got "
                                 f"{tuple(image.shape)} and {tuple(exposure.shape)}")
            exposure = exposure.float().contiguous()
        gt_u8 = gt_u8.contiguous()
        dyn = band_rows is not None
        if dyn and (band_rows.dtype != torch.int32 or not band_rows.is_cuda or band_rows.numel() < 2):
            raise ValueError("band_rows must be an int32 device tensor { y0, y1 }")
        rows = int(gt_u8.shape[1]) if dyn else y1 - y0
        if gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (C, rows, W):
            raise ValueError(f"gt band must be uint8 [{C},{rows},{W}], got {gt_u8.dtype} {tuple(gt_u8.shape)}")
        if mask_u8.dtype != torch.uint8 or tuple(mask_u8.shape) not in ((rows, W), (1, rows, W)):
            raise ValueError(f"mask band must be uint8 [{rows},{W}] or [1,{rows},{W}], got {mask_u8.dtype} "
                             f"{tuple(mask_u8.shape)}")
        mask_u8 = mask_u8.contiguous()
        dev = image.device
        need_grad = ctx.needs_input_grad[0] or (expo and ctx.needs_input_grad[8])
        nb = lib.gsr_l1_ssim_num_partials(C, rows, W)
        partials = torch.empty((max(nb, 1), 2), dtype=torch.float32, device=dev)
        maps = torch.empty((3, C, rows, W), dtype=torch.float32, device=dev) if need_grad else None
        out3 = torch.empty((3,), dtype=torch.float32, device=dev)
        c_l1, c_ssim = (1.0 - lambda_dssim) / n, -lambda_dssim / n
        m = [_ptr(maps[i]) if need_grad else None for i in range(3)]
        with _on(dev):
            if rows > 0:
                with kernel_timer.range("l1_ssim_forward", Px=rows * W):
                    img_ptr = _ptr(image) if dyn else ctypes.c_void_p(image.data_ptr() + 4 * y0 * W)
                    check(lib.gsr_l1_ssim_forward_masked(C, rows, W, img_ptr, H * W, _ptr(gt_u8), _ptr(mask_u8),
                                                         _ptr(partials), m[0], m[1], m[2], _ptr(band_rows),
                                                         _ptr(exposure) if expo else None, _stream()),
                          "gsr_l1_ssim_forward_masked")
            check(lib.gsr_l1_ssim_finalize(nb, _ptr(partials), c_l1, c_ssim, lambda_dssim, 1.0 / n, _ptr(out3),
                                           _stream()), "gsr_l1_ssim_finalize")
        ctx.y0, ctx.y1, ctx.coef, ctx.band_rows, ctx.expo = y0, y1, (c_l1, c_ssim), band_rows, expo
        if need_grad:
            ctx.save_for_backward(image, gt_u8, mask_u8, maps, *([exposure] if expo else []))
        loss, Ll1, ssim = out3[0], out3[1], out3[2]
        ctx.mark_non_differentiable(Ll1, ssim)
        return loss, Ll1, ssim

    @staticmethod
    def backward(ctx, g_loss, _g1, _g2):
        if g_loss is None:
            return (None,) * 9
        image, gt_u8, mask_u8, maps = ctx.saved_tensors[:4]
        exposure = ctx.saved_tensors[4] if ctx.expo else None
        C, H, W = image.shape
        y0, y1 = ctx.y0, ctx.y1
        dyn = ctx.band_rows is not None
        rows = int(gt_u8.shape[1]) if dyn else y1 - y0
        dev = image.device
        g_loss = g_loss if (g_loss.dtype == torch.float32 and g_loss.is_contiguous()) else g_loss.float().contiguous()
        grad = torch.empty_like(image) if (rows == H and not dyn) else torch.zeros_like(image)
        grad_e = e_partials = None
        if ctx.expo:
            grad_e = (torch.empty if rows > 0 else torch.zeros)((3, 4), dtype=torch.float32, device=dev)
            ne = lib.gsr_l1_ssim_exposure_num_partials(rows, W)
            e_partials = torch.empty((max(ne, 1), 12), dtype=torch.float32, device=dev)
        off = 0 if dyn else 4 * y0 * W
        if rows > 0:
            with _on(dev), kernel_timer.range("l1_ssim_backward", Px=rows * W):
                check(lib.gsr_l1_ssim_backward_masked(C, rows, W, ctypes.c_void_p(image.data_ptr() + off), H * W,
                                                      _ptr(gt_u8), _ptr(mask_u8), _ptr(maps[0]), _ptr(maps[1]),
                                                      _ptr(maps[2]), _ptr(g_loss), _ptr(g_loss), float(ctx.coef[0]),
                                                      float(ctx.coef[1]), ctypes.c_void_p(grad.data_ptr() + off), H * W,
                                                      _ptr(ctx.band_rows), _ptr(exposure) if ctx.expo else None,
                                                      _ptr(e_partials) if ctx.expo else None,
                                                      _ptr(grad_e) if ctx.expo else None, _stream()),
                      "gsr_l1_ssim_backward_masked")
        return grad, None, None, None, None, None, None, None, grad_e


def fused_band_loss_masked(image, gt_u8, mask_u8, y0, y1, lambda_dssim, n, band_rows=None, exposure=None):
    """fused_band_loss of the masked band: x' = m x (with `exposure` = [A | b], float32 [3,4] on the device:
    x' = m (A x + b)), y' = m gt / 255, m = mask_u8 / 255 -- uint8 [rows, W] or [1, rows, W], one byte per pixel shared by
    the channels, laid out like one channel of gt_u8 (include/gsraster.h, N1m) -> (loss, Ll1, ssim), with gradients for
    `image` and, when given, `exposure`.  n = H*W*3 of the full image, masked or not."""
    return _FusedBandLossMasked.apply(image, gt_u8, mask_u8, int(y0), int(y1), float(lambda_dssim), float(n), band_rows,
                                      exposure)


# ------------------------------------------------------------------------------- N1g: bilateral-grid colour correction
def _bilagrid_sizes(grid, what):
    if grid.dim() != 4 or grid.shape[0] != 12:
        raise ValueError(f"{what}: a grid is [12, L, GH, GW], got {tuple(grid.shape)}")
    gl, gh, gw = (int(s) for s in grid.shape[1:])
    if not (2 <= gl <= 16 and 2 <= gh <= 64 and 2 <= gw <= 64):
        raise ValueError(f"{what}: grid sizes (GW, GH, L) = ({gw}, {gh}, {gl}) outside 2..64, 2..64, 2..16")
    return gw, gh, gl


class _BilagridSlice(torch.autograd.Function):
    """x' = A_M c + b_M of the rows [y0, y1) of a rendered image, M the trilinear sample of one camera's bilateral grid at
    (pixel position, luminance of c) -- include/gsraster.h, N1g: one launch forward, two backward (pieces of xy-cells +
    the fixed-order fp64 finalize of the lattice gradient)."""

    @staticmethod
    def forward(ctx, image, grid, y0, y1, height):
        if not image.is_cuda or not grid.is_cuda:
            raise RuntimeError("bilagrid_slice: device tensors required (no CPU fallback)")
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"bilagrid_slice: the image must be [3, H, W], got {tuple(image.shape)}")
        gw, gh, gl = _bilagrid_sizes(grid, "bilagrid_slice")
        image, grid = image.float().contiguous(), grid.float().contiguous()
        _, H, W = image.shape
        if H != height:
            raise ValueError(f"bilagrid_slice: the image has {H} rows, `height` says {height}")
        if not 0 <= y0 <= y1 <= H:
            raise ValueError(f"bilagrid_slice: rows [{y0}, {y1}) outside an image of {H} rows")
        dev = image.device
        # the rows outside the band are cleared, not left undefined: the loss kernels never read them (their zero
        # padding at a band's edge is a padding), but the tensor is handed to the caller
        out = torch.empty_like(image) if (y0 == 0 and y1 == H) else zeros_async(image.shape, torch.float32, dev)
        with _on(dev), kernel_timer.range("bilagrid_forward", Px=(y1 - y0) * W):
            check(lib.gsr_bilagrid_slice_forward(W, H, y0, y1, _ptr(image), H * W, _ptr(grid), gw, gh, gl, _ptr(out),
                                                 H * W, _stream()), "gsr_bilagrid_slice_forward")
        ctx.band = (y0, y1)
        ctx.save_for_backward(image, grid)
        return out

    @staticmethod
    def backward(ctx, g_out):
        image, grid = ctx.saved_tensors
        gw, gh, gl = (int(s) for s in reversed(grid.shape[1:]))
        _, H, W = image.shape
        y0, y1 = ctx.band
        dev = image.device
        g_out = g_out if (g_out.dtype == torch.float32 and g_out.is_contiguous()) else g_out.float().contiguous()
        grad = torch.empty_like(image) if (y0 == 0 and y1 == H) else zeros_async(image.shape, torch.float32, dev)
        grad_grid = torch.empty_like(grid)
        partials = torch.empty((max(int(lib.gsr_bilagrid_num_partials(W, H, gw, gh, gl)), 1),), dtype=torch.float32,
                               device=dev)
        with _on(dev), kernel_timer.range("bilagrid_backward", Px=(y1 - y0) * W):
            check(lib.gsr_bilagrid_slice_backward(W, H, y0, y1, _ptr(image), H * W, _ptr(grid), gw, gh, gl, _ptr(g_out),
                                                  H * W, _ptr(grad), H * W, _ptr(partials), _ptr(grad_grid), _stream()),
                  "gsr_bilagrid_slice_backward")
        return grad, grad_grid, None, None, None


def bilagrid_slice(image, grid, y0, y1, height):
    """-> the colour-corrected image [3, H, W]: rows [y0, y1) hold x' = A_M c + b_M with M sampled from `grid`
    ([12, L, GH, GW] float32 on the device, one camera's) at the pixel's position in the FULL image of `height` rows and
    at the luminance of its colour; the other rows are zero.  Gradients for `image` and `grid`."""
    return _BilagridSlice.apply(image, grid, int(y0), int(y1), int(height))


def bilagrid_tv(grids, weight, grad=None, value=False):
    """adds weight * dT/dG to `grad` (default: a fresh zero tensor), T the total variation of `grids` [N, 12, L, GH, GW]
    (include/gsraster.h, N1g), in one launch -> grad, or (grad, T) with value=True (T a float32 device scalar, reduced in
    fp64 in a fixed order by one more launch)"""
    if not grids.is_cuda:
        raise RuntimeError("bilagrid_tv: device tensors required (no CPU fallback)")
    if grids.dim() != 5:
        raise ValueError(f"bilagrid_tv: grids are [N, 12, L, GH, GW], got {tuple(grids.shape)}")
    gw, gh, gl = _bilagrid_sizes(grids[0], "bilagrid_tv")
    g = grids.detach()
    g = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
    dev, N = g.device, int(g.shape[0])
    if grad is None:
        grad = zeros_async(g.shape, torch.float32, dev)
    elif grad.dtype != torch.float32 or not grad.is_contiguous() or grad.shape != g.shape or grad.device != dev:
        raise ValueError("bilagrid_tv: `grad` must be a contiguous float32 device tensor of the grids' shape")
    T = partials = None
    if value:
        T = torch.empty((), dtype=torch.float32, device=dev)
        partials = torch.empty((max(lib.gsr_bilagrid_tv_num_partials(N, gw, gh, gl), 1),), dtype=torch.float64, device=dev)
    with _on(dev), kernel_timer.range("bilagrid_tv"):
        check(lib.gsr_bilagrid_tv(N, gw, gh, gl, _ptr(g), float(weight), _ptr(grad), _ptr(partials), _ptr(T), _stream()),
              "gsr_bilagrid_tv")
    return (grad, T) if value else grad


# ------------------------------------------------------------------------- a19: fused activations
# ------------------------------------------------------------------------------- N1e: evaluation metrics
METRICS_QUANTIZE, METRICS_NO_SSIM = 1, 2  # include/gsraster.h: GSR_METRICS_*


def image_metrics(image, gt_u8, y0=0, y1=None, *, ssim=True, quantize=False, out_u8=None):
    """-> float64 [C,3] on the device: per channel (sum |x - y|, sum (x - y)^2, sum ssim_map(x, y)) over rows [y0, y1) of
    the full image [C,H,W] against the full uint8 ground truth [C,H,W]; x = clamp(image, 0, 1) (quantize: the byte a saved
    PNG holds, / 255), y = gt / 255 (train_internal.py:471-478, utils/image_utils.py:19-21, metrics.py:78-79).  The SSIM
    window reads up to five rows above and below the band from the same two buffers, so the sums of the bands of a
    partition add up to the full image's.  ssim=False: the third column is 0 and nothing outside the band is read.
    out_u8 (uint8 [C, y1-y0, W], optional) receives the quantised band.  Forward only; no host sync."""
    if not (image.is_cuda and gt_u8.is_cuda and (out_u8 is None or out_u8.is_cuda)):
        raise RuntimeError("image_metrics: device tensors required (no CPU fallback)")
    if image.dim() != 3:
        raise ValueError(f"image must be [C,H,W], got {tuple(image.shape)}")
    image = image.detach()
    if image.dtype != torch.float32 or not image.is_contiguous():
        image = image.float().contiguous()
    C, H, W = image.shape
    y1 = H if y1 is None else int(y1)
    y0 = int(y0)
    if not 0 <= y0 < y1 <= H:
        raise ValueError(f"band [{y0}, {y1}) is not inside the {H} rows of the image")
    if gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (C, H, W):
        raise ValueError(f"ground truth must be uint8 [{C},{H},{W}], got {gt_u8.dtype} {tuple(gt_u8.shape)}")
    gt_u8 = gt_u8.contiguous()
    if out_u8 is not None and (out_u8.dtype != torch.uint8 or tuple(out_u8.shape) != (C, y1 - y0, W)
                               or not out_u8.is_contiguous()):
        raise ValueError(f"out_u8 must be a dense uint8 [{C},{y1 - y0},{W}]")
    dev = image.device
    flags = (METRICS_QUANTIZE if quantize else 0) | (0 if ssim else METRICS_NO_SSIM)
    nb = lib.gsr_image_metrics_num_partials(C, y1 - y0, W)
    partials = torch.empty((nb, 3), dtype=torch.float32, device=dev)
    sums = torch.empty((C, 3), dtype=torch.float64, device=dev)
    with _on(dev), kernel_timer.range("image_metrics", Px=(y1 - y0) * W, C=C, ssim=bool(ssim)):
        s = _stream()
        check(lib.gsr_image_metrics(C, H, W, _ptr(image), H * W, _ptr(gt_u8), H * W, y0, y1, flags, _ptr(partials),
                                    _ptr(out_u8), s), "gsr_image_metrics")
        check(lib.gsr_image_metrics_finalize(C, nb, _ptr(partials), _ptr(sums), s), "gsr_image_metrics_finalize")
    return sums


def metrics_from_sums(sums, H, W):
    """image_metrics' sums of a WHOLE image (all bands added) [..., C, 3] -> fp64 device scalars (l1, psnr, ssim) [...]:
    l1 = mean |x - y|, psnr = the mean of the per-channel 20 log10(1 / sqrt(mse_c)) exactly as psnr(image, gt).mean() forms
    it (utils/image_utils.py:19-21; an exact match gives inf there and here), ssim = the mean of the SSIM map."""
    sums = sums.double()
    C = sums.shape[-2]
    n = float(H) * float(W)
    l1 = sums[..., 0].sum(-1) / (C * n)
    psnr = (20.0 * torch.log10(1.0 / torch.sqrt(sums[..., 1] / n))).mean(-1)
    ssim = sums[..., 2].sum(-1) / (C * n)
    return l1, psnr, ssim


class _FusedActivations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, rotation, opacity, features_dc, features_rest):
        ts = [scaling, rotation, opacity, features_dc, features_rest]
        if not all(t.is_cuda for t in ts):
            raise RuntimeError("fused_activations: device tensors required (no CPU fallback)")
        scaling, rotation, opacity, features_dc, features_rest = [t.float().contiguous() for t in ts]
        N, rest = scaling.shape[0], features_rest.shape[1]
        dev = scaling.device
        scales = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rotations = torch.empty((N, 4), dtype=torch.float32, device=dev)
        opacities = torch.empty((N, 1), dtype=torch.float32, device=dev)
        shs = torch.empty((N, 1 + rest, 3), dtype=torch.float32, device=dev)
        with _on(dev), kernel_timer.range("activate_forward"):
            check(lib.gsr_activate_forward(N, rest, _ptr(scaling), _ptr(rotation), _ptr(opacity), _ptr(features_dc),
                                           _ptr(features_rest), _ptr(scales), _ptr(rotations), _ptr(opacities),
                                           _ptr(shs), _stream()), "gsr_activate_forward")
        ctx.save_for_backward(rotation, scales, opacities)
        ctx.rest = rest
        return scales, rotations, opacities, shs

    @staticmethod
    def backward(ctx, g_scales, g_rotations, g_opacities, g_shs):
        rotation, scales, opacities = ctx.saved_tensors
        N, rest = scales.shape[0], ctx.rest
        dev = scales.device

        def z(g, shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else g.float().contiguous()

        g_scales, g_rotations = z(g_scales, (N, 3)), z(g_rotations, (N, 4))
        g_opacities, g_shs = z(g_opacities, (N, 1)), z(g_shs, (N, 1 + rest, 3))
        d_scaling = torch.empty((N, 3), dtype=torch.float32, device=dev)
        d_rotation = torch.empty((N, 4), dtype=torch.float32, device=dev)
        d_opacity = torch.empty((N, 1), dtype=torch.float32, device=dev)
        d_dc = torch.empty((N, 1, 3), dtype=torch.float32, device=dev)
        d_rest = torch.empty((N, rest, 3), dtype=torch.float32, device=dev)
        with _on(dev), kernel_timer.range("activate_backward"):
            check(lib.gsr_activate_backward(N, rest, _ptr(rotation), _ptr(scales), _ptr(opacities), _ptr(g_scales),
                                            _ptr(g_rotations), _ptr(g_opacities), _ptr(g_shs), _ptr(d_scaling),
                                            _ptr(d_rotation), _ptr(d_opacity), _ptr(d_dc), _ptr(d_rest), _stream()),
                  "gsr_activate_backward")
        return d_scaling, d_rotation, d_opacity, d_dc, d_rest


def fused_activations(scaling, rotation, opacity, features_dc, features_rest):
    """(scales, rotations, opacities, shs) = (exp, normalize, sigmoid, cat) of the raw parameters in one
    kernel each way -- GaussianModel.get_scaling/get_rotation/get_opacity/get_features"""
    return _FusedActivations.apply(scaling, rotation, opacity, features_dc, features_rest)


# ---- the 3D smoothing filter of Mip-Splatting (include/gsraster.h: gsr_filter3d_*) -----------------------------------
def filter3d_focal_max(tanfovx, width):
    """the largest fx = width / (2 tanfovx) over the cameras, with K1's float32 roundings, on the host"""
    import numpy as np

    t = np.atleast_1d(np.asarray(tanfovx, dtype=np.float32))
    return float((np.float32(int(width)) / (np.float32(2.0) * t)).max())


def compute_filter3d(xyz, cams_block, width, height, all_reduce_max=None, focal_max=None, return_parts=False):
    """-> filter_3D [N,1] float32 (Mip-Splatting's shape): sqrt(0.2) x (depth in the nearest camera of `cams_block`
    [C,40] (pack_camera records) that sees the row) / focal_max; rows that no camera sees take the largest such depth,
    and zeros when nothing is seen at all.  include/gsraster.h (gsr_filter3d_distance) has the definition.
    `all_reduce_max`: at world size > 1, a callable that MAX-all-reduces a one-element device tensor in place; it runs
    between the two launches, on every rank (also one with no rows), and nothing is read back to the host.
    `focal_max`: the largest fx over ALL training cameras (filter3d_focal_max); when None it is formed from
    cams_block's tanfovx column, which is one small device-to-host copy.
    `return_parts`: also (dist [N], seen uint8 [N])."""
    if not (xyz.is_cuda and cams_block.is_cuda):
        raise RuntimeError("compute_filter3d: device tensors required (no CPU fallback)")
    xyz, cams = _f32c(xyz.detach(), "xyz"), _f32c(cams_block.detach(), "cams_block")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [N, 3]")
    if cams.dim() != 2 or cams.shape[1] != 40:
        raise ValueError("cams_block must be [C, 40]")
    N, C = xyz.shape[0], cams.shape[0]
    dev = xyz.device
    if focal_max is None:
        if C == 0:
            raise ValueError("compute_filter3d: no cameras and no focal_max")
        focal_max = filter3d_focal_max(cams[:, 35].cpu().numpy(), width)
    n_part = lib.gsr_filter3d_num_partials(N)
    dist = torch.empty((N,), dtype=torch.float32, device=dev)
    seen = torch.empty((N,), dtype=torch.uint8, device=dev)
    partials = torch.empty((max(n_part, 1),), dtype=torch.float32, device=dev)
    out = torch.empty((N, 1), dtype=torch.float32, device=dev)
    with _on(dev), kernel_timer.range("filter3d_distance"):
        check(lib.gsr_filter3d_distance(N, C, _ptr(xyz), _ptr(cams), int(width), int(height), _ptr(dist), _ptr(seen),
                                        _ptr(partials), _stream()), "gsr_filter3d_distance")
        gmax = None
        if all_reduce_max is not None:
            # (the one float the ranks exchange: a max over a few thousand partials, once per hundred iterations)
            gmax = partials[:n_part].amax().reshape(1) if n_part else torch.zeros(1, dtype=torch.float32, device=dev)
            all_reduce_max(gmax)
        check(lib.gsr_filter3d_finalize(N, _ptr(dist), _ptr(seen), _ptr(partials), n_part, _ptr(gmax),
                                        float(focal_max), _ptr(out), _stream()), "gsr_filter3d_finalize")
    return (out, dist, seen) if return_parts else out


class _Filter3DApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, opacity, filter_3D):
        if not (scaling.is_cuda and opacity.is_cuda and filter_3D.is_cuda):
            raise RuntimeError("filter3d_apply: device tensors required (no CPU fallback)")
        scaling, opacity = _f32c(scaling, "scaling"), _f32c(opacity, "opacity")
        f = _f32c(filter_3D.detach(), "filter_3D")
        N = scaling.shape[0]
        if scaling.dim() != 2 or scaling.shape[1] != 3 or opacity.numel() != N or f.numel() != N:
            raise ValueError(f"filter3d_apply: scaling [N,3], opacity [N,1] and filter_3D [N,1] expected, got "
                             f"{tuple(scaling.shape)}, {tuple(opacity.shape)}, {tuple(f.shape)}")
        dev = scaling.device
        scaling_eff, opacity_eff = torch.empty_like(scaling), torch.empty_like(opacity)
        with _on(dev), kernel_timer.range("filter3d_apply_forward"):
            check(lib.gsr_filter3d_apply_forward(N, _ptr(scaling), _ptr(opacity), _ptr(f), _ptr(scaling_eff),
                                                 _ptr(opacity_eff), _stream()), "gsr_filter3d_apply_forward")
        ctx.save_for_backward(scaling, opacity, f)
        ctx.set_materialize_grads(False)
        return scaling_eff, opacity_eff

    @staticmethod
    def backward(ctx, g_scaling, g_opacity):
        scaling, opacity, f = ctx.saved_tensors
        N, dev = scaling.shape[0], scaling.device
        if g_scaling is None and g_opacity is None:
            return None, None, None
        g_scaling = torch.zeros_like(scaling) if g_scaling is None else g_scaling.float().contiguous()
        g_opacity = torch.zeros_like(opacity) if g_opacity is None else g_opacity.float().contiguous()
        d_scaling, d_opacity = torch.empty_like(scaling), torch.empty_like(opacity)
        with _on(dev), kernel_timer.range("filter3d_apply_backward"):
            check(lib.gsr_filter3d_apply_backward(N, _ptr(scaling), _ptr(opacity), _ptr(f), _ptr(g_scaling),
                                                  _ptr(g_opacity), _ptr(d_scaling), _ptr(d_opacity), _stream()),
                  "gsr_filter3d_apply_backward")
        return d_scaling, d_opacity, None


def filter3d_apply(scaling, opacity, filter_3D):
    """(_scaling [N,3], _opacity [N,1], filter_3D [N,1]) -> (scaling_eff, opacity_eff): the raw parameters of the
    Gaussians with the 3D filter folded in -- exp(scaling_eff) = sqrt(exp(_scaling)^2 + f^2), sigmoid(opacity_eff) =
    sigmoid(_opacity) prod_k s_k / s'_k -- for the raw K1 / K11 in place of the parameters.  One kernel each way;
    filter_3D gets no gradient; a row with f == 0 keeps its bits, both ways."""
    return _Filter3DApply.apply(scaling, opacity, filter_3D)


def exchange_need(means2D_all, radii_all, bands, width, height):
    """K2 for the whole camera batch in the exchange's layout: means2D_all [B,P,2], radii_all int32 [B,P],
    bands int32 [B,W,2] (tile rows [lo,hi) of camera k rendered by global rank g) ->
    (need bool [W,B,P], counts int32 [W,B])."""
    m2 = _f32c(means2D_all.detach(), "means2D_all")
    if radii_all.dtype != torch.int32 or not radii_all.is_contiguous() or bands.dtype != torch.int32:
        raise ValueError("radii_all / bands must be contiguous int32")
    B, P = radii_all.shape
    W = bands.shape[1]
    bands = bands.to(m2.device).contiguous()
    need = torch.empty((W, B, P), dtype=torch.bool, device=m2.device)
    counts = torch.empty((W, B), dtype=torch.int32, device=m2.device)
    check(lib.gsr_exchange_need(P, B, W, width, height, _ptr(m2), _ptr(radii_all), _ptr(bands), _ptr(need),
                                _ptr(counts), _stream()), "gsr_exchange_need")
    return need, counts


def exchange_count(means2D_all, radii_all, bands, k0, nb, width, height):
    """K2 counted, not materialised: for the cameras [k0, k0 + nb) of the camera-major state (means2D_all fp32 [B,P,2],
    radii_all int32 [B,P]; bands int32 [B,W,2] on the device) -> (chunkcnt int32 [W * nb, chunks], counts int32 [W, nb])"""
    m2 = _f32c(means2D_all.detach(), "means2D_all")
    if radii_all.dtype != torch.int32 or not radii_all.is_contiguous() or bands.dtype != torch.int32 or \
            not bands.is_cuda or not bands.is_contiguous():
        raise ValueError("radii_all / bands must be contiguous int32 device tensors")
    B, P = radii_all.shape
    W = bands.shape[1]
    nchunk = lib.gsr_exchange_chunks(P)
    chunkcnt = torch.empty((W * nb, max(nchunk, 1)), dtype=torch.int32, device=m2.device)
    counts = torch.empty((W, nb), dtype=torch.int32, device=m2.device)
    with _on(m2.device):
        check(lib.gsr_exchange_count(P, B, k0, nb, W, width, height, _ptr(m2), _ptr(radii_all), _ptr(bands),
                                     _ptr(chunkcnt), _ptr(counts), _stream()), "gsr_exchange_count")
    return chunkcnt, counts


def exchange_pack(means2D_all, rgb_all, co_all, radii_all, depths_all, bands, chunkcnt, segment_offsets, n_send, k0, nb,
                  width, height, count_cameras=None, count_first=None):
    """-> (msg fp32 [n_send, 11], send_idx int32 [n_send]): the records of the cameras [k0, k0 + nb) in
    (destination, camera, local index) order; segment_offsets: python ints [W * nb] (first row of each segment);
    chunkcnt: what exchange_count returned for the camera range [count_first, count_first + count_cameras) (default:
    the same range)"""
    B, P = radii_all.shape
    W = bands.shape[1]
    dev = radii_all.device
    msg = torch.empty((n_send, 11), dtype=torch.float32, device=dev)
    send_idx = torch.empty((n_send,), dtype=torch.int32, device=dev)
    if len(segment_offsets) != W * nb:
        raise ValueError("segment_offsets must have W * nb entries")
    seg = (ctypes.c_int32 * (W * nb))(*segment_offsets)
    with _on(dev):
        check(lib.gsr_exchange_pack(P, B, k0, nb, W, width, height, nb if count_cameras is None else count_cameras,
                                    k0 if count_first is None else count_first, _ptr(means2D_all), _ptr(rgb_all), _ptr(co_all),
                                    _ptr(radii_all), _ptr(depths_all), _ptr(bands), _ptr(chunkcnt), seg, n_send,
                                    _ptr(msg), _ptr(send_idx), _stream()), "gsr_exchange_pack")
    return msg, send_idx


def exchange_pack_slab(means2D_all, rgb_all, co_all, radii_all, depths_all, bands, chunkcnt, counts, capacities, k0, nb,
                       width, height, count_cameras=None, count_first=None):
    """the exchange's pack WITHOUT this step's counts on the host (include/gsraster.h: gsr_exchange_pack_slab):
    capacities = python ints [W * nb], rows reserved per (destination, camera of [k0, k0 + nb)); `counts` = the DEVICE
    tensor exchange_count returned with `chunkcnt`.  -> (msg fp32 [sum(capacities), 11], send_idx int32
    [sum(capacities)]): every slab holds its records at the front (reference order), then all-zero padding rows
    (radius 0) whose send_idx is -1; records that do not fit are dropped (the caller detects that from the counts)."""
    B, P = radii_all.shape
    W = bands.shape[1]
    dev = radii_all.device
    if len(capacities) != W * nb:
        raise ValueError("capacities must have W * nb entries")
    n_rows = int(sum(capacities))
    msg = torch.empty((n_rows, 11), dtype=torch.float32, device=dev)
    send_idx = torch.empty((n_rows,), dtype=torch.int32, device=dev)
    caps = (ctypes.c_int32 * (W * nb))(*[int(c) for c in capacities])
    with _on(dev):
        check(lib.gsr_exchange_pack_slab(P, B, k0, nb, W, width, height, nb if count_cameras is None else count_cameras,
                                         k0 if count_first is None else count_first, _ptr(means2D_all), _ptr(rgb_all),
                                         _ptr(co_all), _ptr(radii_all), _ptr(depths_all), _ptr(bands), _ptr(chunkcnt),
                                         _ptr(counts), caps, n_rows, _ptr(msg), _ptr(send_idx), _stream()),
              "gsr_exchange_pack_slab")
    return msg, send_idx


def exchange_unpack(recv):
    """received message fp32 [n, 11] -> (means2D [n,2], rgb [n,3], conic_opacity [n,4], radii int32 [n], depths [n]) in
    one launch (include/gsraster.h: gsr_exchange_unpack)"""
    if not recv.is_cuda or recv.dtype != torch.float32 or recv.dim() != 2 or recv.shape[1] != 11 or \
            not recv.is_contiguous():
        raise ValueError("recv must be a contiguous fp32 [n, 11] device tensor")
    n, dev = recv.shape[0], recv.device
    outs = [torch.empty((n, w), dtype=torch.float32, device=dev) for w in (2, 3, 4)]
    radii = torch.empty((n,), dtype=torch.int32, device=dev)
    depths = torch.empty((n,), dtype=torch.float32, device=dev)
    with _on(dev):
        check(lib.gsr_exchange_unpack(n, _ptr(recv), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(radii),
                                      _ptr(depths), _stream()), "gsr_exchange_unpack")
    return outs[0], outs[1], outs[2], radii, depths


def exchange_check(all_counts, caps_dev, W, B, me, rendered_mask, few, flag, host_copy=None):
    """capacity check of a captured exchange (include/gsraster.h: gsr_exchange_check): raises FLAG_SLAB / FLAG_FEW in
    the device word `flag`"""
    if all_counts.dtype != torch.int32 or caps_dev.dtype != torch.int32 or all_counts.numel() != W * W * B or \
            caps_dev.numel() != W * W * B or not all_counts.is_contiguous() or not caps_dev.is_contiguous():
        raise ValueError("all_counts / caps_dev must be contiguous int32 [W*W*B]")
    with _on(all_counts.device):
        check(lib.gsr_exchange_check(_ptr(all_counts), _ptr(caps_dev), W, B, me, int(rendered_mask), int(few),
                                     _ptr(flag), FLAG_SLAB, FLAG_FEW,
                                     host_copy.data_ptr() if host_copy is not None else None, _stream()),
              "gsr_exchange_check")


def zeros_async(shape, dtype, device):
    """torch.zeros through hipMemsetAsync on the current stream (the fill kernel torch launches runs at ~1 TB/s)"""
    t = torch.empty(shape, dtype=dtype, device=device)
    with _on(device):
        check(lib.gsr_zero_async(_ptr(t), t.numel() * t.element_size(), _stream()), "gsr_zero_async")
    return t


def scatter_add_rows(idx, src, n_rows, dst=None):
    """-> dst fp32 [n_rows, 9] with dst[idx[r]] += src[r] (rows of 9 floats; duplicates in idx accumulate; rows with
    idx[r] < 0 are skipped); `dst`: an existing contiguous [n_rows, 9] view to add into (default: a fresh zero tensor)"""
    src = _f32c(src, "src")
    if src.dim() != 2 or src.shape[1] != 9 or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError("src must be [n, 9] fp32 and idx contiguous int32")
    if dst is None:
        dst = torch.zeros((n_rows, 9), dtype=torch.float32, device=src.device)
    elif tuple(dst.shape) != (n_rows, 9) or dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError("dst must be a contiguous fp32 [n_rows, 9] tensor")
    with _on(src.device):
        check(lib.gsr_scatter_add_rows(src.shape[0], _ptr(idx), _ptr(src), _ptr(dst), _stream()), "gsr_scatter_add_rows")
    return dst


def absgrad_rows(idx, src, n_rows, dst=None):
    """-> dst fp32 [n_rows, 2] with dst[idx[r]] += src[r] (gsr_absgrad_merge_rows: the absolute-gradient rows that came
    back from another rank; duplicates in idx accumulate, rows with idx[r] < 0 are skipped); `dst`: an existing
    contiguous [n_rows, 2] tensor to add into (default: a fresh zero tensor)"""
    src = _f32c(src, "src")
    if not idx.is_cuda:
        raise RuntimeError("diff_gaussian_rasterization: `idx` must live on the gfx950 device (no CPU fallback)")
    if src.dim() != 2 or src.shape[1] != 2 or idx.dtype != torch.int32 or not idx.is_contiguous() or \
            idx.numel() != src.shape[0]:
        raise ValueError("src must be [n, 2] fp32 and idx contiguous int32 [n]")
    if dst is None:
        dst = torch.zeros((n_rows, 2), dtype=torch.float32, device=src.device)
    elif tuple(dst.shape) != (n_rows, 2) or dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError("dst must be a contiguous fp32 [n_rows, 2] tensor")
    with _on(src.device):
        check(lib.gsr_absgrad_merge_rows(src.shape[0], _ptr(idx), _ptr(src), _ptr(dst), _stream()),
              "gsr_absgrad_merge_rows")
    return dst


class ContributionStats:
    """Per-Gaussian contribution statistics of rendered views (include/gsraster.h: gsr_render_contrib), accumulated over
    every view that is rendered into them: hits int64 [P] (pixels that blended the row), wmax fp32 [P] (the largest blend
    weight alpha T on any pixel), wsum fp64 [P] (the sum of the weights).  A row nobody blended stays all zero."""

    def __init__(self, P, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("diff_gaussian_rasterization: ContributionStats must live on the gfx950 device "
                               "(no CPU fallback)")
        self.P = int(P)
        self.hits = torch.zeros((self.P,), dtype=torch.int64, device=device)
        self.wmax = torch.zeros((self.P,), dtype=torch.float32, device=device)
        self.wsum = torch.zeros((self.P,), dtype=torch.float64, device=device)

    @classmethod
    def of(cls, hits, wmax, wsum):
        """a record around existing dense device tensors (int64 / float32 / float64, one length), e.g. rows that came
        back from another rank"""
        if not (hits.is_cuda and wmax.is_cuda and wsum.is_cuda):
            raise RuntimeError("diff_gaussian_rasterization: ContributionStats must live on the gfx950 device "
                               "(no CPU fallback)")
        if (hits.dtype, wmax.dtype, wsum.dtype) != (torch.int64, torch.float32, torch.float64) or \
                not (hits.shape == wmax.shape == wsum.shape and hits.dim() == 1) or \
                not (hits.is_contiguous() and wmax.is_contiguous() and wsum.is_contiguous()):
            raise ValueError("ContributionStats.of: dense int64 hits, float32 wmax and float64 wsum of one length expected")
        self = cls.__new__(cls)
        self.P, self.hits, self.wmax, self.wsum = hits.shape[0], hits, wmax, wsum
        return self

    def zero_(self):
        self.hits.zero_()
        self.wmax.zero_()
        self.wsum.zero_()
        return self

    def merge_rows(self, idx, other):
        """self[idx[r]]: hits += other.hits[r], wmax = max(., other.wmax[r]), wsum += other.wsum[r]; rows with
        idx[r] < 0 are skipped, duplicate indices accumulate (gsr_contrib_merge_rows).  idx: int32 [other.P]"""
        if not isinstance(other, ContributionStats):
            raise TypeError("merge_rows: a ContributionStats expected")
        if not idx.is_cuda:
            raise RuntimeError("diff_gaussian_rasterization: `idx` must live on the gfx950 device (no CPU fallback)")
        if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() != other.P:
            raise ValueError("merge_rows: idx must be contiguous int32 with one entry per row of `other`")
        with _on(self.hits.device):
            check(lib.gsr_contrib_merge_rows(other.P, _ptr(idx), _ptr(other.hits), _ptr(other.wmax), _ptr(other.wsum),
                                             _ptr(self.hits), _ptr(self.wmax), _ptr(self.wsum), _stream()),
                  "gsr_contrib_merge_rows")
        return self

    def importance(self, kind="max"):
        """the per-row score a pruning rule thresholds: "max" (RadSplat), "sum" (LightGaussian), "hits" -> float32 [P]"""
        if kind == "max":
            return self.wmax
        if kind == "sum":
            return self.wsum.to(torch.float32)
        if kind == "hits":
            return self.hits.to(torch.float32)
        raise ValueError(f"importance: kind must be 'max', 'sum' or 'hits', not {kind!r}")


def contribution_stats(ranges, point_list, means2D, conic_opacity, n_contrib, compute_locally, width, height, out,
                       band=None):
    """accumulate one rendered view's statistics into `out` (a ContributionStats of means2D.shape[0] rows): a forward-only
    walk over the lists K8 drew from, with K8's n_contrib -- blended pairs are exactly those of the image.  ranges int32
    [tiles, 2] (the mask's row hull in the row behind it) and point_list as bin_gaussians returns them, compute_locally
    uint8 / bool [tiles],
    band = (row_lo, row_hi) as gsr_render_forward takes it (None: the whole grid)"""
    means2D, conic_opacity = _f32c(means2D, "means2D"), _f32c(conic_opacity, "conic_opacity")
    P = means2D.shape[0]
    if not isinstance(out, ContributionStats) or out.P != P:
        raise ValueError(f"contribution_stats: `out` must be a ContributionStats of {P} rows")
    for t, n in ((ranges, "ranges"), (point_list, "point_list"), (n_contrib, "n_contrib"),
                 (compute_locally, "compute_locally")):
        if not t.is_cuda:
            raise RuntimeError(f"diff_gaussian_rasterization: `{n}` must live on the gfx950 device (no CPU fallback)")
    gx, gy = (int(width) + BLOCK_X - 1) // BLOCK_X, (int(height) + BLOCK_Y - 1) // BLOCK_Y
    mask = compute_locally.contiguous().view(-1)
    mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
    if ranges.dtype != torch.int32 or not ranges.is_contiguous() or ranges.numel() < 2 * gx * gy or \
            point_list.dtype != torch.int32 or not point_list.is_contiguous() or mask.numel() != gx * gy or \
            n_contrib.dtype != torch.int32 or not n_contrib.is_contiguous() or n_contrib.numel() != width * height:
        raise ValueError("contribution_stats: int32 ranges [tiles, 2], point_list and n_contrib [H, W], and a mask of "
                         "one entry per tile expected")
    row_lo, row_hi = (int(band[0]), int(band[1])) if band else (0, 0)
    with _on(means2D.device):
        check(lib.gsr_render_contrib(P, int(width), int(height), _ptr(ranges), _ptr(point_list), _ptr(means2D),
                                     _ptr(conic_opacity), _ptr(mask), _ptr(n_contrib), row_lo, row_hi, _ptr(out.hits),
                                     _ptr(out.wmax), _ptr(out.wsum), _stream()), "gsr_render_contrib")
    return out


def densify_stats(radii, grad, max_radii2D, accum, denom):
    """the per-iteration densification statistics in one launch (include/gsraster.h: gsr_densify_stats); in place.
    radii int32 [P]; grad float32 [P, >=2] with contiguous rows (any row stride: a column view of K10's record is fine);
    max_radii2D [P], accum [P,1], denom [P,1] float32 dense"""
    P = radii.shape[0]
    for t, n in ((radii, "radii"), (grad, "grad"), (max_radii2D, "max_radii2D"), (accum, "accum"), (denom, "denom")):
        if not t.is_cuda:
            raise RuntimeError(f"diff_gaussian_rasterization: `{n}` must live on the gfx950 device (no CPU fallback)")
    if radii.dtype != torch.int32 or grad.dtype != torch.float32 or grad.dim() != 2 or grad.stride(1) != 1 or \
            any(t.dtype != torch.float32 or not t.is_contiguous() for t in (max_radii2D, accum, denom)):
        raise ValueError("densify_stats: int32 radii, float32 grad rows and dense float32 accumulators expected")
    # gsr_densify_stats cannot check sizes: a buffer left over from before a densification event would be written
    # past its end
    if radii.dim() != 1 or grad.shape[0] != P or grad.shape[1] < 2 or max_radii2D.numel() != P or \
            accum.shape[0] != P or accum.numel() != P or denom.shape[0] != P or denom.numel() != P:
        raise ValueError(f"densify_stats: radii has {P} rows, but grad {tuple(grad.shape)}, max_radii2D "
                         f"{tuple(max_radii2D.shape)}, accum {tuple(accum.shape)}, denom {tuple(denom.shape)}")
    with _on(radii.device):
        check(lib.gsr_densify_stats(P, _ptr(radii.contiguous()), _ptr(grad), grad.stride(0) if P > 1 else 2,
                                    _ptr(max_radii2D), _ptr(accum), _ptr(denom), _stream()), "gsr_densify_stats")


def knn_mean_dist2(points):
    """mean squared distance of every point to its 3 nearest other points -- what the reference obtains from
    `simple_knn._C.distCUDA2` at scene creation (scene/gaussian_model.py:163-166).  points: fp32 [P,3] on the
    device; returns fp32 [P]."""
    pts = _f32c(points.detach(), "points")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [P,3]")
    P = pts.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    nbytes = lib.gsr_knn_workspace_bytes(P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    check(lib.gsr_knn_mean_dist2(P, _ptr(pts), _ptr(out), _ptr(ws), nbytes, _stream()), "gsr_knn_mean_dist2")
    return out


def group_rows(dest, num_groups):
    """stable grouping of row indices by destination: returns (order int32 [N], counts list of num_groups+1
    python ints; the last entry counts the rows whose destination is outside [0, num_groups) = dropped).
    One host read-back (the counts size what follows)."""
    if not dest.is_cuda:
        raise RuntimeError("diff_gaussian_rasterization: `dest` must live on the gfx950 device (no CPU fallback)")
    dest = dest.to(torch.int32).contiguous()
    N = dest.shape[0]
    order = torch.empty(N, dtype=torch.int32, device=dest.device)
    counts = torch.empty(num_groups + 1, dtype=torch.int64, device=dest.device)
    nbytes = lib.gsr_group_rows_bytes(N)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dest.device)
    check(lib.gsr_group_rows(N, num_groups, _ptr(dest), _ptr(order), _ptr(counts), _ptr(ws), nbytes, _stream()),
          "gsr_group_rows")
    return order, counts.cpu().tolist()


def scatter_rows(order, n_in, srcs, dsts, row0=0):
    """dst_k[order[row0 + r]] = src_k[r] for r < n_in, all tensors in ONE launch (the inverse of gather_rows)"""
    return gather_rows(order, n_in, srcs, dsts, row0, _scatter=True)


def gather_rows(order, n_out, srcs, dsts=None, row0=0, _scatter=False):
    """dst_k[r] = src_k[order[row0 + r]] (order None: identity) for r < n_out, all tensors in ONE launch.
    srcs / dsts: 4-byte-element tensors whose rows are contiguous (dim 0 may be strided, e.g. a column block of a
    record matrix); dsts=None allocates dense outputs shaped like the sources.  Returns the dsts."""
    if dsts is None:
        dsts = [torch.empty((n_out,) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device) for s in srcs]
    K = len(srcs)
    if K == 0 or n_out == 0:
        return dsts
    if K > 32:
        for i in range(0, K, 32):
            gather_rows(order, n_out, srcs[i:i + 32], dsts[i:i + 32], row0, _scatter)
        return dsts

    def row_layout(t, what):
        if not t.is_cuda:
            raise RuntimeError(f"diff_gaussian_rasterization: {what} must live on the gfx950 device (no CPU fallback)")
        if t.element_size() != 4:
            raise ValueError(f"{what}: 4-byte elements expected, got {t.dtype}")
        w = 1
        for d in t.shape[1:]:
            w *= d
        inner = t[0] if t.shape[0] > 0 else None
        if inner is not None and inner.numel() > 1 and not inner.is_contiguous():
            raise ValueError(f"{what}: rows must be contiguous")
        return w, (t.stride(0) if t.dim() > 0 and t.shape[0] > 1 else w)

    widths, ss, ds = [], [], []
    for s_, d_ in zip(srcs, dsts):
        w, st = row_layout(s_, "source")
        w2, dt = row_layout(d_, "destination")
        if w != w2 or (s_ if _scatter else d_).shape[0] < n_out:
            raise ValueError("source / destination row shapes differ")
        widths.append(w)
        ss.append(st)
        ds.append(dt)
    VP = ctypes.c_void_p * K
    order_ptr = ctypes.c_void_p(order.data_ptr() + 4 * row0) if order is not None else ctypes.c_void_p(0)
    if order is not None and (order.dtype != torch.int32 or not order.is_contiguous()):
        raise ValueError("order must be a contiguous int32 tensor")
    fn, what = (lib.gsr_scatter_rows, "gsr_scatter_rows") if _scatter else (lib.gsr_gather_rows, "gsr_gather_rows")
    check(fn(n_out, order_ptr, K, VP(*[s_.data_ptr() for s_ in srcs]), VP(*[d_.data_ptr() for d_ in dsts]),
             (ctypes.c_int32 * K)(*widths), (ctypes.c_int64 * K)(*ss), (ctypes.c_int64 * K)(*ds), _stream()), what)
    return dsts


DENSIFY_KEEP_ORIGINAL, DENSIFY_KEEP_CLONE, DENSIFY_SPLIT_PARENT, DENSIFY_KEEP_CHILDREN = 1, 2, 4, 8  # class bits
DENSIFY_ROLE_COPY, DENSIFY_ROLE_MOMENT, DENSIFY_ROLE_XYZ, DENSIFY_ROLE_SCALING = 0, 1, 2, 3


def densify_plan(cls, ranks=None, split_rows=None, workspace=None):
    """the plan of a one-pass densification event (include/gsraster.h: gsr_densify_plan): cls uint8 [P] class bytes ->
    (ranks int32 [4,P], split_rows int32 [P], counts int64 [4] ON THE DEVICE = n_orig, n_clone, n_child, n_split).
    No host read-back here: the caller reads the four counts once.  ranks / split_rows / workspace: buffers to reuse
    (at least P rows / gsr_densify_plan_bytes(P) bytes)."""
    if not cls.is_cuda:
        raise RuntimeError("diff_gaussian_rasterization: `cls` must live on the gfx950 device (no CPU fallback)")
    if cls.dtype != torch.uint8 or cls.dim() != 1 or not cls.is_contiguous():
        raise ValueError("cls must be a contiguous uint8 vector")
    P, dev = cls.shape[0], cls.device
    if ranks is None or ranks.numel() < 4 * P:
        ranks = torch.empty(4 * max(P, 1), dtype=torch.int32, device=dev)
    if split_rows is None or split_rows.numel() < P:
        split_rows = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    if ranks.dtype != torch.int32 or split_rows.dtype != torch.int32 or not ranks.is_contiguous() or \
            not split_rows.is_contiguous():
        raise ValueError("ranks / split_rows must be contiguous int32 tensors")
    nbytes = lib.gsr_densify_plan_bytes(P)
    if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
        workspace = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with _on(dev):
        check(lib.gsr_densify_plan(P, _ptr(cls), _ptr(ranks), _ptr(split_rows), _ptr(counts), _ptr(workspace),
                                   workspace.numel() * workspace.element_size(), _stream()), "gsr_densify_plan")
    return ranks.view(-1)[:4 * P].view(4, P), split_rows[:P], counts


def densify_move(cls, ranks, counts, srcs, dsts, roles, alts=None, rotation=None, samples=None, copies=2):
    """write the result of a densification event for all tensors in ONE launch (include/gsraster.h: gsr_densify_move).
    cls / ranks: the plan's; counts: its four counts as python ints; srcs[k] [P, ...] -> dsts[k] [>= n_new, ...]
    (rows contiguous, 4-byte elements, never aliasing), roles[k] one of DENSIFY_ROLE_*; alts[k]: the dense [P,3] child
    source of a SCALING tensor; rotation [P,4] / samples [copies * n_split, 3]: what the XYZ role computes children
    from.  Returns n_new = n_orig + n_clone + copies * n_child."""
    n_orig, n_clone, n_child, n_split = (int(c) for c in counts)
    n_new = n_orig + n_clone + copies * n_child
    K, P = len(srcs), cls.shape[0]
    if K > 32:
        raise ValueError("densify_move: at most 32 tensors per launch")
    if K == 0 or P == 0:
        return n_new
    alts = list(alts) if alts is not None else [None] * K
    if tuple(ranks.shape) != (4, P) or ranks.dtype != torch.int32 or not ranks.is_contiguous():
        raise ValueError("ranks must be the plan's contiguous int32 [4,P]")
    widths, ss, ds = [], [], []
    dst_rows = min(d.shape[0] for d in dsts)
    for s_, d_, a_, role in zip(srcs, dsts, alts, roles):
        for t, what in ((s_, "source"), (d_, "destination"), (a_, "alternate source")):
            if t is None:
                continue
            if not t.is_cuda:
                raise RuntimeError(f"diff_gaussian_rasterization: {what} must live on the gfx950 device (no CPU "
                                   "fallback)")
            if t.element_size() != 4 or not t.is_contiguous():
                raise ValueError(f"{what}: dense tensors of 4-byte elements expected")
        w = 1
        for d in s_.shape[1:]:
            w *= d
        if s_.shape[0] != P or tuple(d_.shape[1:]) != tuple(s_.shape[1:]) or d_.dtype != s_.dtype:
            raise ValueError("source / destination row shapes differ")
        if role == DENSIFY_ROLE_SCALING and (a_ is None or tuple(a_.shape) != (P, 3) or w != 3):
            raise ValueError("a SCALING tensor needs a dense [P,3] alternate source")
        if role == DENSIFY_ROLE_XYZ and n_child > 0 and (
                w != 3 or rotation is None or samples is None or tuple(rotation.shape) != (P, 4) or
                tuple(samples.shape) != (copies * n_split, 3) or not rotation.is_contiguous() or
                not samples.is_contiguous() or rotation.dtype != torch.float32 or samples.dtype != torch.float32):
            raise ValueError("an XYZ tensor needs rotation [P,4] and samples [copies * n_split, 3], dense fp32")
        s0, e0 = s_.data_ptr(), s_.data_ptr() + s_.numel() * 4
        d0, d1 = d_.data_ptr(), d_.data_ptr() + n_new * w * 4
        if s0 < d1 and d0 < e0:
            raise ValueError("densify_move: a source aliases its destination")
        widths.append(w)
        ss.append(w)
        ds.append(w)
    VP = ctypes.c_void_p * K
    with _on(cls.device):
        check(lib.gsr_densify_move(P, _ptr(cls), _ptr(ranks), n_orig, n_clone, n_child, n_split, int(copies), K,
                                   VP(*[s_.data_ptr() for s_ in srcs]), VP(*[d_.data_ptr() for d_ in dsts]),
                                   VP(*[a_.data_ptr() if a_ is not None else None for a_ in alts]),
                                   (ctypes.c_int32 * K)(*widths), (ctypes.c_int32 * K)(*[int(r) for r in roles]),
                                   (ctypes.c_int64 * K)(*ss), (ctypes.c_int64 * K)(*ds), dst_rows, _ptr(rotation),
                                   _ptr(samples), _stream()), "gsr_densify_move")
    return n_new


# ------------------------------------------------------------------------------------------ 3DGS-MCMC
MCMC_ROLE_COPY, MCMC_ROLE_MOMENT, MCMC_ROLE_OPACITY, MCMC_ROLE_SCALING = 0, 1, 2, 3
MCMC_N_MAX = 51


def _mcmc_dense(t, name, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(f"diff_gaussian_rasterization: `{name}` must live on the gfx950 device (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: a dense {dtype} tensor expected")
    return t


def mcmc_relocate_plan(opacity_act, n_add, min_opacity, seed, event, src=None, count=None, workspace=None):
    """the plan of a relocation event (include/gsraster.h: gsr_mcmc_relocate_plan): opacity_act fp32 [P] (activated) ->
    (src int32 [P+n_add], count int32 [P], totals int64 [2] = {n_dead, n_alive}), all on the device; nothing is read back.
    src / count / workspace: buffers to reuse (at least P+n_add / P elements / gsr_mcmc_relocate_bytes(P) bytes)."""
    op = _mcmc_dense(opacity_act, "opacity_act").reshape(-1)
    P, n_add, dev = op.shape[0], int(n_add), op.device
    if n_add < 0:
        raise ValueError("n_add must not be negative")
    if src is None or src.numel() < P + n_add:
        src = torch.empty(max(P + n_add, 1), dtype=torch.int32, device=dev)
    if count is None or count.numel() < P:
        count = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    _mcmc_dense(src, "src", torch.int32)
    _mcmc_dense(count, "count", torch.int32)
    nbytes = lib.gsr_mcmc_relocate_bytes(P)
    if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
        workspace = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    if P == 0:  # no row to draw from (the entry point writes nothing): no destination has a source
        src.view(-1)[:n_add].fill_(-1)
        return src.view(-1)[:n_add], count.view(-1)[:0], totals.zero_()
    with _on(dev):
        check(lib.gsr_mcmc_relocate_plan(P, n_add, _ptr(op), float(min_opacity), int(seed) & (2 ** 64 - 1),
                                         int(event) & 0xffffffff, _ptr(src), _ptr(count), _ptr(totals), _ptr(workspace),
                                         workspace.numel() * workspace.element_size(), _stream()),
              "gsr_mcmc_relocate_plan")
    return src.view(-1)[:P + n_add], count.view(-1)[:P], totals


def mcmc_relocate_apply(src, count, opacity_act, min_opacity, tensors, roles, n_max=MCMC_N_MAX):
    """apply a relocation plan IN PLACE to every tensor in two launches (include/gsraster.h: gsr_mcmc_relocate_apply).
    src [P+n_add] / count [P]: the plan's; tensors[k]: [>= P+n_add, ...] dense, 4-byte elements; roles[k] one of
    MCMC_ROLE_*."""
    op = _mcmc_dense(opacity_act, "opacity_act").reshape(-1)
    _mcmc_dense(src, "src", torch.int32)
    _mcmc_dense(count, "count", torch.int32)
    P, rows, K = op.shape[0], src.shape[0], len(tensors)
    if count.shape[0] != P or rows < P:
        raise ValueError("mcmc_relocate_apply: src [P+n_add] and count [P] of the plan expected")
    if K > 32:
        raise ValueError("mcmc_relocate_apply: at most 32 tensors per call")
    if not 1 <= int(n_max) <= MCMC_N_MAX:
        raise ValueError(f"n_max must lie in [1, {MCMC_N_MAX}]")
    widths = []
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("diff_gaussian_rasterization: every tensor must live on the gfx950 device (no CPU "
                               "fallback)")
        if t.element_size() != 4 or not t.is_contiguous() or t.shape[0] < rows:
            raise ValueError("mcmc_relocate_apply: dense tensors of 4-byte elements with at least P + n_add rows expected")
        w = 1
        for d in t.shape[1:]:
            w *= d
        widths.append(w)
    if K == 0 or P == 0:
        return
    VP = ctypes.c_void_p * K
    with _on(op.device):
        check(lib.gsr_mcmc_relocate_apply(P, rows - P, _ptr(src), _ptr(count), _ptr(op), float(min_opacity), int(n_max), K,
                                          VP(*[t.data_ptr() for t in tensors]), (ctypes.c_int32 * K)(*widths),
                                          (ctypes.c_int64 * K)(*widths), (ctypes.c_int32 * K)(*[int(r) for r in roles]),
                                          _stream()), "gsr_mcmc_relocate_apply")


def mcmc_normals(n, seed, step, device=None, out=None):
    """the xi [n,3] that mcmc_noise(xi=None) draws for rows 0..n-1 at (seed, step) (gsr_mcmc_normals)"""
    if out is None:
        out = torch.empty((int(n), 3), dtype=torch.float32, device=device if device is not None else "cuda")
    _mcmc_dense(out, "out")
    if out.numel() < 3 * int(n):
        raise ValueError("out: room for [n,3] expected")
    with _on(out.device):
        check(lib.gsr_mcmc_normals(int(n), int(seed) & (2 ** 64 - 1), int(step) & 0xffffffff, _ptr(out), _stream()),
              "gsr_mcmc_normals")
    return out


def mcmc_noise(xyz, scaling_raw, rotation_raw, opacity_raw, scaler, xi=None, seed=0, step=0):
    """xyz += scaler * g(1 - sigmoid(opacity_raw)) * Sigma * xi, in place, one launch (gsr_mcmc_noise).  xi None: drawn in
    the kernel from (seed, step) -- the values of mcmc_normals; otherwise a dense fp32 [P,3]."""
    P = xyz.shape[0]
    for t, name, shape in ((xyz, "xyz", (P, 3)), (scaling_raw, "scaling_raw", (P, 3)),
                           (rotation_raw, "rotation_raw", (P, 4)), (xi, "xi", (P, 3))):
        if t is not None and tuple(_mcmc_dense(t, name).shape) != shape:
            raise ValueError(f"{name}: shape {shape} expected")
    if _mcmc_dense(opacity_raw, "opacity_raw").numel() != P:
        raise ValueError("opacity_raw: P elements expected")
    with _on(xyz.device):
        check(lib.gsr_mcmc_noise(P, _ptr(xyz), _ptr(scaling_raw), _ptr(rotation_raw), _ptr(opacity_raw), float(scaler),
                                 _ptr(xi), int(seed) & (2 ** 64 - 1), int(step) & 0xffffffff, _stream()),
              "gsr_mcmc_noise")
    return xyz


def mcmc_reg_grad(opacity_raw, scaling_raw, c_opacity, c_scale, grad_opacity, grad_scaling):
    """grad_opacity += c_opacity * o (1 - o), grad_scaling += c_scale * exp(s), in place, one launch (gsr_mcmc_reg_grad)"""
    P = scaling_raw.shape[0]
    for t, name, numel in ((opacity_raw, "opacity_raw", P), (scaling_raw, "scaling_raw", 3 * P),
                           (grad_opacity, "grad_opacity", P), (grad_scaling, "grad_scaling", 3 * P)):
        if _mcmc_dense(t, name).numel() != numel:
            raise ValueError(f"{name}: {numel} elements expected")
    with _on(scaling_raw.device):
        check(lib.gsr_mcmc_reg_grad(P, _ptr(opacity_raw), _ptr(scaling_raw), float(c_opacity), float(c_scale),
                                    _ptr(grad_opacity), _ptr(grad_scaling), _stream()), "gsr_mcmc_reg_grad")


# ------------------------------------------------------------------------------------------ _C
class _CNamespace:
    """stand-in for the reference extension's pybind module `diff_gaussian_rasterization._C`."""

    @staticmethod
    def get_block_XY():
        bx, by, bz = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        check(lib.gsr_get_block_xy(ctypes.byref(bx), ctypes.byref(by), ctypes.byref(bz)), "gsr_get_block_xy")
        return bx.value, by.value, bz.value

    @staticmethod
    def get_local2j_ids_bool(image_height, image_width, mp_rank, mp_world_size, means2D, radii,
                             dist_global_strategy, cuda_args=None):
        """bool [P, mp_world_size]: Gaussian i touches a tile of band j
        (gaussian_renderer/workload_division.py:727-738)."""
        means2D = _f32c(means2D.detach(), "means2D")
        radii = radii.to(torch.int32).contiguous()
        div = dist_global_strategy.to(device=means2D.device, dtype=torch.int32).contiguous()
        if div.numel() != mp_world_size + 1:
            raise ValueError("dist_global_strategy must have world_size + 1 entries")
        P = means2D.shape[0]
        out = torch.empty((P, mp_world_size), dtype=torch.uint8, device=means2D.device)
        with _on(means2D.device):
            check(lib.gsr_get_local2j_ids_bool(P, int(image_width), int(image_height), int(mp_world_size),
                                               _ptr(means2D), _ptr(radii), _ptr(div), _ptr(out), _stream()),
                  "gsr_get_local2j_ids_bool")
        return out.view(torch.bool)

    @staticmethod
    def _dead(name):
        raise NotImplementedError(
            f"diff_gaussian_rasterization._C.{name}: only reachable from the reference's legacy (non-`final`) "
            "distribution modes, which train.py never selects (SURVEY.md F4)")

    @staticmethod
    def get_local2j_ids_bool_adjust_mode6(*a, **k):
        _CNamespace._dead("get_local2j_ids_bool_adjust_mode6")

    @staticmethod
    def get_touched_locally(*a, **k):
        _CNamespace._dead("get_touched_locally")

    @staticmethod
    def get_pixels_compute_locally_and_in_rect(*a, **k):
        _CNamespace._dead("get_pixels_compute_locally_and_in_rect")


_C = _CNamespace()


def load_image_tiles_by_pos(*a, **k):
    _CNamespace._dead("load_image_tiles_by_pos")


def merge_image_tiles_by_pos(*a, **k):
    _CNamespace._dead("merge_image_tiles_by_pos")
