"""mesh extraction A/B: the fusion of a batch of depth maps on the HIP kernel of tsdf.hip beside a plain chunked torch
implementation of the same per-voxel rule, in one process, the legs taking turns after a warm-up, device events around
windows of a few hundred ms (tools/invdepth_ab.py's windows and statistics); then the extraction (count + scan + the
read-back of the totals + emit) on the fused volume, timed alone: no torch marching tetrahedra was written to put beside it.
    python tools/mesh_ab.py [OUT.json] [--dim 512] [--views 16] [--width 1920] [--height 1080] [--rounds 7]
Scene: a sphere of radius 0.3 x the volume's side in the middle of a cubic volume of --dim^3 voxels, --views cameras on a
ring at 1.6 sides from the centre, depth maps and colours by analytic ray intersection (torch, on the device), trunc = 4
voxels.  Both legs start every pass from the same state (the planes are not reset: a pass adds the batch once more, which
costs the same).  The two results of ONE batch on a fresh volume are compared first: the share of voxels whose weights
differ (the legs round px, py and sdf differently in the last bit) and the largest tsdf difference where they agree.
No gate: the figures are written down.  The last line printed is the whole result as one JSON object (also written to
OUT.json when given; the project keeps profiles/mesh_ab.json).  Kernel names for a later trace: tsdf_tiles_kernel,
tsdf_integrate_kernel<true|false>, tsdf_count_kernel, tsdf_scan_kernel, tsdf_emit_kernel<true|false>.

    python tools/mesh_ab.py --clean [OUT.json] [--blobs 300] [the options above]
is the mesh-cleaning leg (csrc/meshclean.hip; the project keeps profiles/mesh_clean_ab.json): the same scene with --blobs
small spheres scattered between the big one and the volume's faces, fused and extracted once; then, taking turns under
the same windows, mesh_filter(keep_largest=1) on that mesh (components + select + the read-back of the totals + compact),
the same on a seeded shuffle of its vertex numbers and face order (everything on the global union path), the extraction
re-measured beside them, and a plain torch restatement: label propagation with scatter_reduce(amin) and a pointer jump
per round to a fixed point (one read-back per round), then unique / argsort / boolean indexing.  The torch leg's mesh
must equal the HIP leg's bit for bit or the script stops.  Kernel names: mc_init_kernel, mc_union_kernel,
mc_flatten_kernel, mc_count_kernel, mc_flag_count_kernel<0|1>, mc_scan_kernel, mc_flag_emit_kernel<0|1>,
mc_select_kernel, mc_compact_kernel<true|false>."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import meshing  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from invdepth_ab import WINDOW_MS, alternate, dev, stats  # noqa: E402

SLAB = 64  # z-slices per chunk of the torch leg: its temporaries stay near 1.5 GB at 512^2 x 64 voxels


def look_at(eye, target):
    """[4,4] fp32 view matrix, row-vector convention, +z towards the target, +y down"""
    fwd = torch.nn.functional.normalize(target - eye, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), fwd), dim=0)
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd])
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = R.t()
    M[3, :3] = -R @ eye
    return M.float()


def sphere_maps(view, W, H, tanx, tany, centre, radius, blobs=()):
    """z-depth [H,W] (0 where the ray misses) and colour [3,H,W] of the sphere, on the device; blobs: further
    (centre, radius) spheres, the nearest hit wins"""
    M = view.double()
    R, eye = M[:3, :3].t(), -M[:3, :3] @ M[3, :3]
    j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                          torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    d = torch.stack([((2 * i + 1) / W - 1) * tanx, ((2 * j + 1) / H - 1) * tany, torch.ones_like(i)], -1) @ R.to(dev)
    a, s = (d * d).sum(-1), None
    for c_k, r_k in ((centre, radius),) + tuple(blobs):
        oc = (eye - c_k).to(dev)
        b, c = 2 * (d @ oc), oc @ oc - r_k ** 2
        disc = b * b - 4 * a * c
        s_k = torch.where(disc > 0, (-b - disc.clamp_min(0).sqrt()) / (2 * a), torch.zeros_like(a)).clamp_min(0)
        s = s_k if s is None else torch.where((s_k > 0) & ((s == 0) | (s_k < s)), s_k, s)
    pt = eye.to(dev) + d * s[..., None]
    col = torch.stack([0.5 + 0.4 * torch.sin(9 * pt[..., 0]), 0.5 + 0.4 * torch.cos(7 * pt[..., 1]), 0.5 + 0.4 * torch.sin(5 * pt[..., 2])])
    return s.float(), (col * (s > 0)).float()


def torch_integrate(state, origin, vs, trunc, depths, views, tanx, tany, colors, near=0.2):
    """the rule of include/gsraster.h (gsr_tsdf_integrate) on dense [Z,Y,X] planes, SLAB z-slices at a time"""
    tsdf, weight, rgb = state
    Z, Y, X = tsdf.shape
    V, H, W = depths.shape
    ax = lambda n, o: o + vs * torch.arange(n, device=dev, dtype=torch.float32)
    px_, py_ = ax(X, origin[0])[None, None, :], ax(Y, origin[1])[None, :, None]
    for z0 in range(0, Z, SLAB):
        sl = slice(z0, z0 + SLAB)
        pz_ = ax(Z, origin[2])[sl, None, None]
        t, w, c = tsdf[sl], weight[sl], rgb[:, sl]
        for v in range(V):
            m = views[v]
            x = m[0, 0] * px_ + m[1, 0] * py_ + m[2, 0] * pz_ + m[3, 0]
            y = m[0, 1] * px_ + m[1, 1] * py_ + m[2, 1] * pz_ + m[3, 1]
            z = m[0, 2] * px_ + m[1, 2] * py_ + m[2, 2] * pz_ + m[3, 2]
            rx = torch.round(((x / (z * tanx) + 1) * W - 1) * 0.5)
            ry = torch.round(((y / (z * tany) + 1) * H - 1) * 0.5)
            ok = (z > near) & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
            pix = torch.where(ok, ry * W + rx, torch.zeros_like(rx)).long()
            d = depths[v].reshape(-1)[pix]
            sdf = d - z
            ok &= (d > 0) & (sdf >= -trunc) & (sdf <= trunc)
            wn = w + 1.0
            t.copy_(torch.where(ok, (t * w + sdf / trunc) / wn, t))
            c.copy_(torch.where(ok[None], (c * w[None] + colors[v].reshape(3, -1)[:, pix]) / wn[None], c))
            w.copy_(torch.where(ok, wn, w))


def torch_clean(vertices, faces, colors, keep_largest):
    """mesh_filter's definitions in plain torch: min-label propagation over the faces to a fixed point, then the order
    (count descending, label ascending) and boolean indexing"""
    V, f = vertices.shape[0], faces.long()
    labels = torch.arange(V, device=dev)
    while True:
        m = labels[f].amin(1, keepdim=True).expand(-1, 3)
        new = labels.scatter_reduce(0, f.reshape(-1), m.reshape(-1), "amin")
        new = new[new]  # (a label is a vertex of the same component: a pointer jump)
        if torch.equal(new, labels):
            break
        labels = new
    roots, counts = torch.unique(labels[f[:, 0]], return_counts=True)  # (increasing label; zero-triangle ones never kept)
    order = torch.argsort(counts, descending=True, stable=True)
    keep = torch.zeros(V, dtype=torch.bool, device=dev)
    keep[roots[order[:keep_largest] if keep_largest else order]] = True
    vkeep = keep[labels]
    remap = (torch.cumsum(vkeep, 0) - 1).int()
    return vertices[vkeep], remap[f[vkeep[f[:, 0]]]], colors[vkeep]


def clean_main(a, vol, res):
    import diff_gaussian_rasterization as dgr

    v, f, c = vol.extract()
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(v.shape[0], generator=g).to(dev)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(v.shape[0], device=dev)
    sv, sc, sf = v[inv], c[inv], perm.int()[f.long()][torch.randperm(f.shape[0], generator=g).to(dev)].contiguous()
    labels, tri_count = dgr.mesh_components(f, v.shape[0])
    sizes = tri_count[tri_count > 0].sort(descending=True).values
    hip, ref = dgr.mesh_filter(v, f, c, keep_largest=1), torch_clean(v, f, c, 1)
    if not all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(hip, ref)):
        raise SystemExit("mesh_ab --clean: the torch leg's mesh differs from the HIP leg's")
    shuf = dgr.mesh_filter(sv, sf, sc, keep_largest=1)
    res["clean"] = {"blobs": a.blobs, "vertices": int(v.shape[0]), "triangles": int(f.shape[0]),
                    "components_with_triangles": int(sizes.shape[0]), "largest": sizes[:3].tolist(),
                    "kept_vertices": int(hip[0].shape[0]), "kept_triangles": int(hip[1].shape[0]),
                    "shuffled_kept_triangles": int(shuf[1].shape[0]), "torch_equals_hip": True}
    del hip, ref, shuf, labels, tri_count
    legs = [[lambda: dgr.mesh_filter(v, f, c, keep_largest=1) and 0], [lambda: dgr.mesh_filter(sv, sf, sc, keep_largest=1) and 0],
            [lambda: vol.extract() and 0], [lambda: torch_clean(v, f, c, 1) and 0],
            [lambda: dgr.mesh_components(f, v.shape[0]) and 0]]
    names = ("clean_hip", "clean_hip_shuffled", "extract_hip", "clean_torch", "components_hip")
    for n, ts in zip(names, alternate(legs, a.rounds)):
        res[n] = stats(ts, 1)
    res["clean_torch_over_hip"] = round(res["clean_torch"]["median_ms"] / res["clean_hip"]["median_ms"], 2)
    res["clean_hip_over_extract"] = round(res["clean_hip"]["median_ms"] / res["extract_hip"]["median_ms"], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clean", action="store_true", help="the mesh-cleaning leg instead of the fusion A/B")
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.rounds < 7 or not (1 <= a.views <= 16) or a.dim % 8:
        ap.error("--rounds: at least 7; --views: 1..16; --dim: a multiple of 8")
    N, W, H, V = a.dim, a.width, a.height, a.views
    vs, tanx = 1.0 / N, 0.6
    tany = tanx * H / W
    origin, trunc = (-0.5, -0.5, -0.5), 4 * vs
    centre = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64)
    views = torch.stack([look_at(torch.tensor([1.6 * math.sin(2 * math.pi * k / V), -0.3, 1.6 * math.cos(2 * math.pi * k / V)],
                                              dtype=torch.float64), centre) for k in range(V)])
    blobs = ()
    if a.clean:  # small spheres of 3 .. 8 voxels radius between the big one and the volume's faces, seeded
        g = torch.Generator().manual_seed(1)
        dirs = torch.nn.functional.normalize(torch.randn(a.blobs, 3, generator=g, dtype=torch.float64), dim=1)
        dist, rad = 0.36 + 0.08 * torch.rand(a.blobs, generator=g, dtype=torch.float64), (3 + 5 * torch.rand(a.blobs, generator=g)) * vs
        blobs = tuple((dirs[k] * dist[k], float(rad[k])) for k in range(a.blobs))
    maps = [sphere_maps(v, W, H, tanx, tany, centre, 0.3, blobs) for v in views]
    depths, colors, views = torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps]), views.to(dev)
    vol = meshing.TSDFVolume(origin, vs, (N, N, N), trunc, device=dev)

    def dense_state():
        return [torch.ones((N, N, N), device=dev), torch.zeros((N, N, N), device=dev), torch.zeros((3, N, N, N), device=dev)]

    vol.integrate(depths, views, tanx, tany, colors=colors)
    if a.clean:
        res = {"dim": N, "views": V, "width": W, "height": H, "trunc_voxels": 4, "window_ms": WINDOW_MS, "rounds": a.rounds,
               "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH)}
        clean_main(a, vol, res)
        return finish(a, res)
    # one batch on fresh volumes: do the two legs compute the same thing at this size?
    state = dense_state()
    torch_integrate(state, origin, vs, trunc, depths, views, tanx, tany, colors)
    t, w, _ = vol.dense()
    same = w == state[1]
    res = {"dim": N, "views": V, "width": W, "height": H, "trunc_voxels": 4, "window_ms": WINDOW_MS, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "voxels_with_weight": int((w > 0).sum()), "weight_mismatch_share": float((~same).float().mean()),
           "tsdf_max_abs_diff_where_weights_agree": float(((t - state[0]).abs() * same).max())}
    del t, w, same
    mesh = vol.extract()
    res["mesh"] = {"vertices": int(mesh[0].shape[0]), "triangles": int(mesh[1].shape[0])}
    del mesh
    legs = [[lambda: vol.integrate(depths, views, tanx, tany, colors=colors) and 0],
            [lambda: torch_integrate(state, origin, vs, trunc, depths, views, tanx, tany, colors)],
            [lambda: vol.extract() and 0]]
    hip, ref, ext = alternate(legs, a.rounds)
    res["integrate_hip"], res["integrate_torch"], res["extract_hip"] = stats(hip, 1), stats(ref, 1), stats(ext, 1)
    res["integrate_torch_over_hip"] = round(res["integrate_torch"]["median_ms"] / res["integrate_hip"]["median_ms"], 2)
    finish(a, res)


def finish(a, res):
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
