"""3D smoothing filter A/B: what the four kernels of csrc/filter3d.hip cost alone, and what
gaussian_renderer.set_filter3d(True) adds to a training step, in one process, the legs taking turns after a warm-up,
device events around windows of a few hundred ms.
    python tools/filter3d_ab.py [OUT.txt] [--P 1000000] [--rounds 9] [--views 4] [--kernels-only]
The c1 shape: 10^6 Gaussians of the synthetic scene (seed 0), 1920 x 1080, SH degree 3, orbit cameras, one rank.

Kernels alone:
    distance C=1 / 100 / 1000   gsr_filter3d_distance + gsr_filter3d_finalize over C orbit cameras (12 B in, 9 B out per
                                row and launch pair; 18 lane-operations per (row, camera))
    finalize                    gsr_filter3d_finalize alone
    apply forward / backward    gsr_filter3d_apply_forward (36 B per row) / gsr_filter3d_apply_backward (52 B per row)
Training step (the product's calls: projection, render_final, fused L1 + SSIM loss, backward,
FusedAdam(fuse_backward=True) -- learning rates 0 so that every window sees the same scene), the views in rotation:
    step                 set_filter3d(False): the fused K11 + Adam launch
    step + filter        set_filter3d(True): apply forward, K1, ..., plain K11, apply backward, dense Adam
    step, again          the first leg twice in the rotation: the noise floor of this very method
Every line printed also goes to OUT.txt when given; the last line is the whole result as one JSON object."""
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
from diff_gaussian_rasterization import _lib  # noqa: E402

W, H, DEG = 1920, 1080, 3
WINDOW_MS = 200.0
dev = torch.device("cuda:0")  # (a name only: nothing touches the device before main())


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def window(fns, n):
    """-> ms per pass over `fns`, n passes between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    code = 0
    for _ in range(n):
        for fn in fns:
            code |= fn() or 0
    e1.record()
    e1.synchronize()
    assert code == 0, code
    return e0.elapsed_time(e1) / n


def alternate(legs, rounds):
    ns = []
    for fns in legs:
        window(fns, 3)
        ns.append(max(3, min(4000, int(math.ceil(WINDOW_MS / max(window(fns, 5), 1e-3))))))
    out = [[] for _ in legs]
    for _ in range(rounds):
        for k, fns in enumerate(legs):
            out[k].append(window(fns, ns[k]))
    return out


def stats(ts):
    s = sorted(ts)
    return {"median_ms": round(s[len(s) // 2], 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5),
            "spread_ms": round(s[-1] - s[0], 5)}


class Kernels:
    def __init__(self, P):
        import filter3d as F

        self.P = P
        self.model = S.SyntheticGaussianModel(P, W, H, seed=0, sh_degree=DEG, device=dev)
        self.xyz = self.model._xyz.detach()
        self.blocks = {C: torch.stack([F._record(c, dev) for c in S.orbit_cameras(C, W, H, device=dev)])
                       for C in (1, 100, 1000)}
        self.focal = dgr.filter3d_focal_max(self.blocks[1][:, 35].cpu().numpy(), W)
        self.dist = torch.empty(P, device=dev)
        self.seen = torch.empty(P, dtype=torch.uint8, device=dev)
        self.n_part = _lib.lib.gsr_filter3d_num_partials(P)
        self.partials = torch.empty(self.n_part, device=dev)
        self.f = torch.empty(P, 1, device=dev)
        self.s_eff, self.o_eff = torch.empty(P, 3, device=dev), torch.empty(P, 1, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        self.gs, self.go = torch.randn(P, 3, device=dev, generator=gen), torch.randn(P, 1, device=dev, generator=gen)
        self.ds, self.do = torch.empty(P, 3, device=dev), torch.empty(P, 1, device=dev)

    def distance(self, C):
        b = self.blocks[C]
        return _lib.lib.gsr_filter3d_distance(self.P, C, ptr(self.xyz), ptr(b), W, H, ptr(self.dist), ptr(self.seen),
                                              ptr(self.partials), dgr._stream())

    def finalize(self):
        return _lib.lib.gsr_filter3d_finalize(self.P, ptr(self.dist), ptr(self.seen), ptr(self.partials), self.n_part,
                                              None, self.focal, ptr(self.f), dgr._stream())

    def forward(self):
        m = self.model
        return _lib.lib.gsr_filter3d_apply_forward(self.P, ptr(m._scaling), ptr(m._opacity), ptr(self.f),
                                                   ptr(self.s_eff), ptr(self.o_eff), dgr._stream())

    def backward(self):
        m = self.model
        return _lib.lib.gsr_filter3d_apply_backward(self.P, ptr(m._scaling), ptr(m._opacity), ptr(self.f), ptr(self.gs),
                                                    ptr(self.go), ptr(self.ds), ptr(self.do), dgr._stream())


class Trainer:
    """the product's training step on one rank, one camera per step"""

    def __init__(self, P, n_views):
        import filter3d as F
        import gaussian_renderer as gr
        import utils.general_utils as utils
        from fused_optim import FusedAdam
        from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal

        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
        utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        self.gr = gr
        self.model = S.SyntheticGaussianModel(P, W, H, seed=0, sh_degree=DEG, device=dev)
        self.cams = S.orbit_cameras(n_views, W, H, device=dev)
        for k, c in enumerate(self.cams):
            c.original_image_backup = S.make_gt_image(W, H, seed=20 + k, device=dev)
        F.compute_3D_filter(self.model, self.cams)
        self.hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(self.cams), 1, 0)
        groups = self.model.param_groups()
        for g in groups:
            g["lr"] = 0.0
        self.opt = FusedAdam(groups, lr=0.0, eps=1e-15, fuse_backward=True)
        self.bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
        self.pipe = type("P", (), {"debug": False})()
        self.turn = 0

    def step(self, with_filter):
        from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
        from gaussian_renderer.loss_distribution import batched_loss_computation, load_camera_from_cpu_to_all_gpu
        from gaussian_renderer.workload_division import start_strategy_final

        self.gr.set_filter3d(with_filter)
        batch = [self.cams[self.turn % len(self.cams)]]
        self.turn += 1
        strategies, tasks = start_strategy_final(batch, self.hist)
        load_camera_from_cpu_to_all_gpu(batch, strategies, tasks)
        pkg = distributed_preprocess3dgs_and_all2all_final(batch, self.model, self.pipe, self.bg,
                                                           batched_strategies=strategies, mode="train")
        images, masks = render_final(pkg, strategies)
        loss, _ = batched_loss_computation(images, batch, masks, strategies,
                                           [ca["stats_collector"] for ca in pkg["batched_cuda_args"]])
        loss.backward()
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true", help="skip the training-step legs")
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if a.out:
            with open(a.out, "w") as fo:
                fo.write("\n".join(lines) + "\n")

    k = Kernels(a.P)
    for C in (1, 100, 1000):
        assert k.distance(C) == 0 and k.finalize() == 0
    assert k.forward() == 0 and k.backward() == 0
    torch.cuda.synchronize()
    res = {"P": a.P, "width": W, "height": H, "sh_degree": DEG, "views": a.views, "window_ms": WINDOW_MS,
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "rows_seen_C1000": int(k.seen.sum()), "filter_mean": round(float(k.f.mean()), 6)}
    legs = [[lambda: k.distance(1), k.finalize], [lambda: k.distance(100), k.finalize],
            [lambda: k.distance(1000), k.finalize], [k.finalize], [k.forward], [k.backward],
            [lambda: k.distance(1), k.finalize]]
    names = ("distance_C1", "distance_C100", "distance_C1000", "finalize", "apply_forward", "apply_backward",
             "distance_C1_again")
    for name, ts in zip(names, alternate(legs, a.rounds)):
        res[name] = stats(ts)
        say(f"{name:20s} {res[name]['median_ms']:.5f} ms (min {res[name]['min_ms']:.5f}, max {res[name]['max_ms']:.5f})")
    res["kernel_noise_floor_ms"] = round(max(abs(res["distance_C1_again"]["median_ms"] - res["distance_C1"]["median_ms"]),
                                             res["distance_C1"]["spread_ms"]), 5)
    per_pair = (res["distance_C1000"]["median_ms"] - res["distance_C100"]["median_ms"]) * 1e-3 / (900.0 * a.P)
    res["ns_per_row_and_camera"] = round(per_pair * 1e9, 6)
    res["apply_forward_GBps"] = round(36.0 * a.P / (res["apply_forward"]["median_ms"] * 1e-3) / 1e9, 1)
    res["apply_backward_GBps"] = round(52.0 * a.P / (res["apply_backward"]["median_ms"] * 1e-3) / 1e9, 1)
    say(f"per (row, camera) {res['ns_per_row_and_camera']} ns; apply forward {res['apply_forward_GBps']} GB/s, "
        f"backward {res['apply_backward_GBps']} GB/s; noise floor {res['kernel_noise_floor_ms']} ms")
    if not a.kernels_only:
        del k
        torch.cuda.empty_cache()
        tr = Trainer(a.P, a.views)
        off, on = [lambda: tr.step(False)], [lambda: tr.step(True)]
        t_off, t_on, t_again = alternate([off, on, off], a.rounds)
        tr.gr.set_filter3d(False)
        tr.opt.set_fuse_backward(False)
        res["step"], res["step_with_filter"], res["step_again"] = stats(t_off), stats(t_on), stats(t_again)
        res["ratio_step_with_filter_over_step"] = round(res["step_with_filter"]["median_ms"] / res["step"]["median_ms"], 4)
        res["step_noise_floor_ms"] = round(max(abs(res["step_again"]["median_ms"] - res["step"]["median_ms"]),
                                               res["step"]["spread_ms"], res["step_again"]["spread_ms"]), 5)
        res["fused_steps"] = tr.opt.fused_steps
        for name in ("step", "step_with_filter", "step_again"):
            say(f"{name:20s} {res[name]['median_ms']:.5f} ms (min {res[name]['min_ms']:.5f}, max {res[name]['max_ms']:.5f})")
        say(f"step with filter / step {res['ratio_step_with_filter_over_step']}; noise floor {res['step_noise_floor_ms']} ms")
    say(json.dumps(res))


if __name__ == "__main__":
    main()
