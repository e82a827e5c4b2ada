"""Mesh extraction from a trained model: the training views' depth maps fused into a truncated signed distance volume,
and the zero level set by marching tetrahedra -- the step 2DGS / PGSR / GOF run in Open3D on the host.  The reference has
no mesh extraction: nothing here mirrors a reference call site.

Both stages run on the HIP kernels of tsdf.hip (`tsdf_integrate`: one launch per 16 views with a voxel's state in
registers; `tsdf_extract`: count, scan, emit), without atomics: the same views in the same order give the same bits,
however they are batched.  World size 1 only; DESIGN.md 3.21.  `clean_mesh` / `extract(keep_largest=...)` then drop the
small disconnected shells on the device (meshclean.hip).
"""
import math

import numpy as np
import torch

from diff_gaussian_rasterization import TSDF_MAX_VIEWS, mesh_filter, tsdf_extract, tsdf_integrate


class TSDFVolume:
    """A regular grid of X x Y x Z voxels (rounded up to multiples of 8), voxel (i,j,k) centred at
    origin + voxel_size (i,j,k), truncation distance `trunc`.  Planes `tsdf` (1 = untouched), `weight` (0) and, with
    color=True, `rgb` ([3, ...]) are fp32 torch tensors in brick-major layout [Z/8, Y/8, X/8, 8, 8, 8]."""

    def __init__(self, origin, voxel_size, dims, trunc, color=True, device="cuda"):
        if not (voxel_size > 0 and trunc > 0) or len(dims) != 3 or min(dims) <= 0:
            raise ValueError("TSDFVolume: voxel_size, trunc and the three dims must be positive")
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size, self.trunc = float(voxel_size), float(trunc)
        self.dims = tuple(-(-int(d) // 8) * 8 for d in dims)
        X, Y, Z = self.dims
        shape = (Z // 8, Y // 8, X // 8, 8, 8, 8)
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=device)
        self.rgb = torch.zeros((3,) + shape, dtype=torch.float32, device=device) if color else None

    def integrate(self, depths, viewmatrices, tanfovx, tanfovy, colors=None, weights=None, depth_trunc=math.inf,
                  near=0.2):
        """depths [V,H,W], viewmatrices [V,4,4] (the cameras' world_view_transform), colors [V,3,H,W] (needed iff the
        volume has colour), weights: V positive numbers or None.  The views are applied in order, 16 per launch."""
        V = depths.shape[0]
        if weights is not None:
            weights = torch.as_tensor(weights, dtype=torch.float32).reshape(-1).cpu()
            if weights.shape[0] != V or not bool((weights > 0).all()):
                raise ValueError("TSDFVolume.integrate: `weights` must be V positive numbers")
            weights = weights.to(self.tsdf.device)
        for s in range(0, V, TSDF_MAX_VIEWS):
            e = min(V, s + TSDF_MAX_VIEWS)
            tsdf_integrate(self.tsdf, self.weight, self.rgb, self.origin, self.voxel_size, self.dims, self.trunc,
                           depths[s:e], viewmatrices[s:e], tanfovx, tanfovy,
                           colors=None if colors is None else colors[s:e],
                           view_weights=None if weights is None else weights[s:e], depth_trunc=depth_trunc, near=near)
        return self

    @staticmethod
    def _dense(plane):
        nz, ny, nx = plane.shape[-6:-3]
        return plane.permute(*range(plane.dim() - 6), -6, -3, -5, -2, -4, -1).reshape(*plane.shape[:-6], nz * 8, ny * 8,
                                                                                      nx * 8)

    def dense(self):
        """(tsdf [Z,Y,X], weight [Z,Y,X], rgb [3,Z,Y,X] or None): copies in the plain layout"""
        return self._dense(self.tsdf), self._dense(self.weight), None if self.rgb is None else self._dense(self.rgb)

    def from_dense(self, tsdf, weight, rgb=None):
        """the inverse of dense(): fill the planes from [Z,Y,X] (rgb: [3,Z,Y,X]) tensors"""
        X, Y, Z = self.dims
        for dst, src, lead in ((self.tsdf, tsdf, ()), (self.weight, weight, ()), (self.rgb, rgb, (3,))):
            if dst is None and src is not None:
                raise ValueError("TSDFVolume.from_dense: the volume has no colour planes")
            if dst is None or src is None:
                continue
            src = torch.as_tensor(src, dtype=torch.float32)
            if tuple(src.shape) != lead + (Z, Y, X):
                raise ValueError(f"TSDFVolume.from_dense: expected {lead + (Z, Y, X)}, got {tuple(src.shape)}")
            n = len(lead)
            v = src.to(dst.device).reshape(*lead, Z // 8, 8, Y // 8, 8, X // 8, 8)
            dst.copy_(v.permute(*range(n), n, n + 2, n + 4, n + 1, n + 3, n + 5))
        return self

    def extract(self, min_weight=0.0, keep_largest=0, min_triangles=0):
        """-> (vertices [Nv,3] fp32, faces [Nf,3] int32, colors [Nv,3] or None); a cell counts iff its 8 corners have a
        positive weight that is at least min_weight; normals face positive tsdf (the free side).  With keep_largest or
        min_triangles above 0 the mesh then goes through mesh_filter (see clean_mesh); with both 0 it does not."""
        mesh = tsdf_extract(self.tsdf, self.weight, self.rgb, self.origin, self.voxel_size, self.dims, min_weight)
        if keep_largest == 0 and min_triangles == 0:
            return mesh
        return mesh_filter(*mesh, keep_largest=keep_largest, min_triangles=min_triangles)


def clean_mesh(vertices, faces, colors=None, keep_largest=50, min_triangles=0):
    """Drop the floaters of a fused mesh on the device (meshclean.hip): keep the connected components that
    are among the `keep_largest` largest by triangle count (ties to the one with the lowest vertex index; 0: no limit;
    the default is 2DGS's post_process_mesh(cluster_to_keep=50)) and have at least max(min_triangles, 1) triangles.
    -> (vertices, faces re-indexed, colors or None), order kept, rows copied bit for bit.  Any indexed triangle mesh on
    the device will do: vertices fp32 [V,3], faces int32 [F,3], colors fp32 [V,3]."""
    return mesh_filter(vertices, faces, colors, keep_largest=keep_largest, min_triangles=min_triangles)


def save_ply(path, vertices, faces, colors=None):
    """binary little-endian PLY: float x y z (and uchar red green blue), faces as uchar-counted int lists"""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4")
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c = (torch.as_tensor(colors).detach().cpu().numpy().clip(0, 1) * 255 + 0.5).astype("u1")
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"], frec["i"] = 3, f
    props = "".join(f"property {'float' if t == '<f4' else 'uchar'} {n}\n" for n, t in fields)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\n{props}"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def fuse_views(cameras, gaussians, pipe_args, background, strategies, volume, depth="median"):
    """Render every camera (forward only, one at a time, as gaussian_renderer.score_contributions does) with the surfel
    pass on and integrate its depth map and image into `volume` (a TSDFVolume), in camera order.  depth: "median"
    (pkg["batched_median_depth"]) or "expected" (D / A of the surfel map, 0 where A is 0).  The normals / surfel
    switches are set for the loop and restored afterwards.  World size 1 only (NotImplementedError before any
    collective); not inside a graph capture.  -> volume"""
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    import utils.general_utils as utils

    if depth not in ("median", "expected"):
        raise ValueError(f"fuse_views: depth must be 'median' or 'expected', got {depth!r}")
    if utils.DEFAULT_GROUP.size() > 1:
        raise NotImplementedError("fuse_views: mesh extraction is not available at world size > 1 (every rank would fuse "
                                  "its own band of every view)")
    if dgr.capturing() is not None:
        raise RuntimeError("fuse_views: not supported inside a graph capture")
    before = (gr.get_normal_consistency(), gr.get_surfel_pass(), gr._SURFELS[1])
    try:
        gr.set_normal_consistency(True)
        gr.set_surfel_pass(True, distortion=None)
        with torch.no_grad():
            for camera, strategy in zip(cameras, strategies):
                pkg = gr.distributed_preprocess3dgs_and_all2all_final([camera], gaussians, pipe_args, background,
                                                                      batched_strategies=[strategy], mode="test",
                                                                      _legacy=True)
                images, _ = gr.render_final(pkg, [strategy])
                if pkg.get("batched_median_depth") is None or pkg["batched_median_depth"][0] is None:
                    continue  # (fewer than 10 Gaussians in view: render_final drew nothing)
                d = pkg["batched_median_depth"][0]
                if depth == "expected":
                    F = pkg["batched_features"][0]
                    d = torch.where(F[0] > 0, F[1] / F[0], torch.zeros_like(F[1]))
                rs = pkg["batched_rasterizers"][0].raster_settings
                volume.integrate(d[None], camera.world_view_transform.reshape(1, 4, 4).float(), rs.tanfovx, rs.tanfovy,
                                 colors=images[0][None].float() if volume.rgb is not None else None)
    finally:
        gr.set_surfel_pass(False)
        gr.set_normal_consistency(before[0])
        if before[1]:
            gr.set_surfel_pass(True, distortion=before[2])
    return volume
