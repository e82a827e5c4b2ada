"""Depth-normal consistency A/B: what the surfel-row kernels and the fused image-space loss of csrc/normals.hip cost, beside
the same math as plain torch float32 operations on the device and inside the training step, in one process, the legs
taking turns after a warm-up, device events around windows of a few hundred ms (tools/invdepth_ab.py's method, whose
windows, statistics and Trainer are reused).
    python tools/normals_ab.py [OUT.json] [--P 1000000] [--rounds 7] [--views 4]
The c1 shape: 10^6 Gaussians of the synthetic scene (seed 0), 1920 x 1080, SH degree 3, orbit cameras, one rank.
    rows_forward / rows_backward                gsr_normal_rows_forward / _backward on the model's raw rows and one view's radii
    consistency_forward / consistency_backward  gsr_normal_consistency_forward (+ finalize) / _backward on a rendered map
    torch_rows_forward, torch_rows_both         the same definitions as torch operations (forward; forward + autograd)
    torch_consistency_forward, torch_consistency_both
    step, step_with_term, step_again            the eager training step without the mode, with it (loss + 0.05 x the term),
                                                and without it again (ms per step, FusedAdam(fuse_backward=False) both ways)
The first HIP leg runs twice in the rotation: the noise floor of this very method.  No gate: the figures are written down.
The last line printed is the whole result as one JSON object (also written to OUT.json when given; the project keeps
profiles/normals_ab.json)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
from diff_gaussian_rasterization import _lib  # noqa: E402
from invdepth_ab import H, W, DEG, WINDOW_MS, Trainer, alternate, dev, ptr, stats  # noqa: E402

TERM_WEIGHT = 0.05  # 2DGS's lambda_normal


def torch_rows(xyz, scaling, rotation, radii, V):
    """include/gsraster.h's gsr_normal_rows_forward as torch operations"""
    P = xyz.shape[0]
    t = xyz @ V[:3, :3] + V[3, :3]
    k = scaling.argmin(dim=1)
    q = rotation / rotation.norm(dim=1, keepdim=True).clamp(min=1e-12)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(P, 3, 3)
    a_c = torch.gather(R, 2, k[:, None, None].expand(P, 3, 1))[:, :, 0] @ V[:3, :3]
    sigma = torch.where((a_c * t).sum(1) > 0, -1.0, 1.0).detach()
    rows = torch.cat([torch.ones_like(t[:, :1]), t[:, 2:3], sigma[:, None] * a_c], dim=1)
    return rows * (radii > 0)[:, None]


def torch_consistency(F, tanfovx, tanfovy, weight):
    """include/gsraster.h's gsr_normal_consistency_forward as torch operations"""
    Hh, Ww = F.shape[1:]
    A, D, N = F[0], F[1], F[2:5]
    ok = A > 1e-6
    z = torch.where(ok, D / torch.where(ok, A, 1.0), 0.0)
    rx = ((2 * torch.arange(Ww, dtype=F.dtype, device=F.device) + 1) / Ww - 1) * tanfovx
    ry = ((2 * torch.arange(Hh, dtype=F.dtype, device=F.device) + 1) / Hh - 1) * tanfovy
    X = torch.stack([z * rx[None, :], z * ry[:, None], z])
    dx = X[:, 1:-1, 2:] - X[:, 1:-1, :-2]
    dy = X[:, 2:, 1:-1] - X[:, :-2, 1:-1]
    c = torch.cross(dy, dx, dim=0)
    l2 = (c * c).sum(0)
    good = l2 > 1e-24
    n = torch.where(good, c / torch.sqrt(torch.where(good, l2, 1.0)), 0.0)
    e = 1 - A.detach()[1:-1, 1:-1] * (N[:, 1:-1, 1:-1] * n).sum(0)
    return weight / (Hh * Ww) * e.sum()


class NormalsTrainer(Trainer):
    def step(self, with_term, keep=None):
        from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
        from gaussian_renderer.loss_distribution import (batched_loss_computation, load_camera_from_cpu_to_all_gpu,
                                                         normal_consistency_loss)
        from gaussian_renderer.workload_division import start_strategy_final

        self.gr.set_normal_consistency(with_term)
        batch = [self.cams[self.turn % len(self.cams)]]
        self.turn += 1
        strategies, tasks = start_strategy_final(batch, self.hist)
        load_camera_from_cpu_to_all_gpu(batch, strategies, tasks)
        pkg = distributed_preprocess3dgs_and_all2all_final(batch, self.model, self.pipe, self.bg,
                                                           batched_strategies=strategies, mode="train")
        images, masks = render_final(pkg, strategies)
        loss, _ = batched_loss_computation(images, batch, masks, strategies,
                                           [ca["stats_collector"] for ca in pkg["batched_cuda_args"]])
        if with_term:
            loss = loss + normal_consistency_loss(pkg, batch, TERM_WEIGHT)
        loss.backward()
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        if keep is not None:
            keep.update(fmap=pkg["batched_features"][0].detach().clone(),
                        radii=pkg["batched_locally_preprocessed_radii"][0].detach().to(torch.int32).clone(), cam=batch[0])
        return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--views", type=int, default=4)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    tr = NormalsTrainer(a.P, a.views)
    kept = {}
    tr.step(True, keep=kept)  # one step with the mode on: a rendered surfel map and that view's radii
    F, radii, cam = kept["fmap"], kept["radii"], kept["cam"]
    tanx, tany = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    V = cam.world_view_transform.float().contiguous()
    m = tr.model
    xyz, sc, rot = m._xyz.detach(), m._scaling.detach(), m._rotation.detach()
    P = xyz.shape[0]
    rows, g_rows = torch.empty((P, 5), device=dev), torch.rand((P, 5), device=dev)
    d_xyz, d_rot = torch.empty_like(xyz), torch.empty_like(rot)
    n_part = _lib.lib.gsr_normal_consistency_num_partials(W, H)
    partials, loss = torch.empty(n_part, dtype=torch.float64, device=dev), torch.empty((), device=dev)
    dF = torch.empty_like(F)
    L = _lib.lib

    def rows_fwd():
        return L.gsr_normal_rows_forward(P, ptr(xyz), ptr(sc), ptr(rot), ptr(radii), ptr(V), ptr(rows), dgr._stream())

    def rows_bwd():
        return L.gsr_normal_rows_backward(P, ptr(xyz), ptr(sc), ptr(rot), ptr(radii), ptr(V), ptr(g_rows), ptr(d_xyz),
                                          ptr(d_rot), dgr._stream())

    def cons_fwd():
        return L.gsr_normal_consistency_forward(W, H, ptr(F), tanx, tany, 1.0, ptr(partials), loss.data_ptr(), None,
                                                dgr._stream())

    def cons_bwd():
        return L.gsr_normal_consistency_backward(W, H, ptr(F), tanx, tany, 1.0, None, ptr(dF), dgr._stream())

    leaves = [t.clone().requires_grad_(True) for t in (xyz, rot)]
    Fl = F.clone().requires_grad_(True)

    def t_rows_fwd():
        with torch.no_grad():
            torch_rows(xyz, sc, rot, radii, V)
        return 0

    def t_rows_both():
        torch.autograd.grad(torch_rows(leaves[0], sc, leaves[1], radii, V), leaves, g_rows)
        return 0

    def t_cons_fwd():
        with torch.no_grad():
            torch_consistency(F, tanx, tany, 1.0)
        return 0

    def t_cons_both():
        torch.autograd.grad(torch_consistency(Fl, tanx, tany, 1.0), Fl)
        return 0

    # the two formulations agree before anything is timed
    assert rows_fwd() == 0 and cons_fwd() == 0 and rows_bwd() == 0 and cons_bwd() == 0
    e_rows = float((rows - torch_rows(xyz, sc, rot, radii, V)).abs().max())
    e_loss = abs(float(loss) - float(torch_consistency(F, tanx, tany, 1.0)))
    names = ["rows_forward", "rows_backward", "consistency_forward", "consistency_backward", "torch_rows_forward",
             "torch_rows_both", "torch_consistency_forward", "torch_consistency_both", "rows_forward_again"]
    legs = [[rows_fwd], [rows_bwd], [cons_fwd], [cons_bwd], [t_rows_fwd], [t_rows_both], [t_cons_fwd], [t_cons_both],
            [rows_fwd]]
    res = {"P": a.P, "width": W, "height": H, "sh_degree": DEG, "views": a.views, "window_ms": WINDOW_MS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "term_weight": TERM_WEIGHT,
           "rows_visible": int((radii > 0).sum()), "max_abs_rows_hip_minus_torch": e_rows,
           "abs_loss_hip_minus_torch": e_loss, "loss": float(loss)}
    for name, ts in zip(names, alternate(legs, a.rounds)):
        res[name] = stats(ts, 1)
    med = {n: res[n]["median_ms"] for n in names}
    res["torch_rows_backward_ms"] = round(med["torch_rows_both"] - med["torch_rows_forward"], 5)
    res["torch_consistency_backward_ms"] = round(med["torch_consistency_both"] - med["torch_consistency_forward"], 5)
    res["ratio_torch_over_hip_rows_both"] = round(med["torch_rows_both"] / (med["rows_forward"] + med["rows_backward"]), 2)
    res["ratio_torch_over_hip_consistency_both"] = round(
        med["torch_consistency_both"] / (med["consistency_forward"] + med["consistency_backward"]), 2)
    res["kernel_noise_floor_ms"] = round(max(abs(med["rows_forward_again"] - med["rows_forward"]),
                                             res["rows_forward"]["spread_ms"], res["rows_forward_again"]["spread_ms"]), 5)
    del leaves, Fl
    torch.cuda.empty_cache()
    off, on = [lambda: tr.step(False)], [lambda: tr.step(True)]
    t_off, t_on, t_again = alternate([off, on, off], a.rounds)
    tr.gr.set_normal_consistency(False)
    res["step"], res["step_with_term"], res["step_again"] = stats(t_off, 1), stats(t_on, 1), stats(t_again, 1)
    res["ratio_step_with_term_over_step"] = round(res["step_with_term"]["median_ms"] / res["step"]["median_ms"], 4)
    res["step_noise_floor_ms"] = round(max(abs(res["step_again"]["median_ms"] - res["step"]["median_ms"]),
                                           res["step"]["spread_ms"], res["step_again"]["spread_ms"]), 5)
    res["library"] = os.path.basename(_lib.LIB_PATH)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
