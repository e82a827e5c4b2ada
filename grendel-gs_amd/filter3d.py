"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024) for a GaussianModel -- the companion of
diff_gaussian_rasterization.set_antialiasing (its 2D Mip filter).  Extension of this build: the reference has neither.

A Gaussian may not shrink below the sampling interval of the nearest training camera that sees it: per row one scalar
`pc.filter_3D` [N,1], recomputed from ALL training cameras after every densification event and every 100 iterations
afterwards (Mip-Splatting's schedule), and folded into the scales and the opacity in front of K1 / K11 while
gaussian_renderer.set_filter3d(True) is on:

    s'_k = sqrt(s_k^2 + f^2),      o' = sigmoid(_opacity) prod_k s_k / s'_k.

Densification and pruning keep reading the unfiltered getters, as Mip-Splatting's do.  include/gsraster.h
(gsr_filter3d_*) has the definitions; the kernels are csrc/filter3d.hip."""
import math

import torch

import diff_gaussian_rasterization as _dgr


def _record(camera, dev):
    """the camera's [40] packed record, from / into the cache the renderer keeps on the camera object (same key)"""
    tanfovx, tanfovy = math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5)
    mats = (camera.world_view_transform, camera.full_proj_transform, camera.camera_center)
    key = (float(tanfovx), float(tanfovy)) + tuple((t.data_ptr(), t._version) for t in mats)
    cached = getattr(camera, "_gsr_packed", None)
    if cached is not None and cached[0] == key and cached[1].device == dev and not cached[1].requires_grad:
        return cached[1]
    rs = _dgr.GaussianRasterizationSettings(int(camera.image_height), int(camera.image_width), tanfovx, tanfovy, None,
                                            1.0, *(t.detach().to(dev) for t in mats[:2]), 0, mats[2].detach().to(dev),
                                            False, False)
    rec = _dgr.pack_camera(rs)
    if all(t.device == dev and not t.requires_grad for t in mats):  # (the renderer's rule for caching a record)
        try:
            camera._gsr_packed = (key, rec)
        except AttributeError:
            pass
    return rec


@torch.no_grad()
def compute_3D_filter(pc, cameras, group=None):
    """sets (and returns) pc.filter_3D [N,1] from the training cameras (Mip-Splatting's GaussianModel.compute_3D_filter).
    `group`: the process group that shards the Gaussians (default: utils.DEFAULT_GROUP); at size > 1 every rank must
    call this -- one MAX all-reduce of one device float gives the rows no camera sees the same value on all ranks.
    Nothing is read back to the host."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("compute_3D_filter: no cameras")
    xyz = pc._xyz
    if not xyz.is_cuda:
        raise RuntimeError("compute_3D_filter: the model must live on the gfx950 device (there is no CPU path)")
    sizes = {(int(c.image_width), int(c.image_height)) for c in cameras}
    if len(sizes) != 1:
        raise ValueError("compute_3D_filter: all cameras must have one image size (as the renderer requires)")
    (W, H), = sizes
    block = torch.stack([_record(c, xyz.device) for c in cameras])
    focal_max = _dgr.filter3d_focal_max([math.tan(c.FoVx * 0.5) for c in cameras], W)
    if group is None:
        import utils.general_utils as utils

        group = utils.DEFAULT_GROUP
    hook = None
    if group is not None and group.size() > 1:
        import torch.distributed as dist

        def hook(t):
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group if isinstance(group, dist.ProcessGroup) else None)

    pc.filter_3D = _dgr.compute_filter3d(xyz, block, W, H, all_reduce_max=hook, focal_max=focal_max)
    return pc.filter_3D


def _filter_of(pc, what):
    f = getattr(pc, "filter_3D", None)
    if not torch.is_tensor(f) or f.numel() != pc._xyz.shape[0]:
        raise RuntimeError(f"{what}: pc.filter_3D is missing or does not have one entry per Gaussian "
                           f"({'none' if not torch.is_tensor(f) else f.numel()} for {pc._xyz.shape[0]} rows): call "
                           "filter3d.compute_3D_filter(pc, training_cameras) after every densification event")
    return f


@torch.no_grad()
def bake(pc):
    """-> (scaling, opacity): raw tensors with the filter folded in -- exp(scaling) = s', sigmoid(opacity) = o' -- what
    Mip-Splatting's save_fused_ply stores; a model with these parameters renders, with the filter off, the image the
    filtered model renders"""
    return _dgr.filter3d_apply(pc._scaling, pc._opacity, _filter_of(pc, "filter3d.bake"))


@torch.no_grad()
def reset_opacity_filter3d(pc):
    """Mip-Splatting's reset_opacity: the FILTERED opacity <- min(., 0.01), with c = prod_k s_k / s'_k divided out again
    before the logit; rows whose filtered opacity already is <= 0.01 keep their raw value.  Swaps the parameter through
    replace_tensor_to_optimizer (zeroed moments), like densification_ops.reset_opacity."""
    from densification_ops import replace_tensor_to_optimizer

    scaling_eff, opacity_eff = bake(pc)
    c = torch.exp((pc._scaling - scaling_eff).sum(dim=1, keepdim=True))
    sigma = (0.01 / c).clamp(max=1.0 - 2.0 ** -20)
    new = torch.where(torch.sigmoid(opacity_eff) <= 0.01, pc._opacity, torch.log(sigma / (1.0 - sigma)))
    pc._opacity = replace_tensor_to_optimizer(pc, new.contiguous(), "opacity")["opacity"]
