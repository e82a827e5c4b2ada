"""densification event A/B: step-by-step (switch off) vs one-pass (switch on), alternating, plus a streaming copy of the
same bytes.  python tools/densify_event_ab.py ROWS EVENTS OUT.json"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

import densification_ops as D  # noqa: E402
import diff_gaussian_rasterization as dgr  # noqa: E402
from fused_optim import FusedAdam  # noqa: E402

dev = torch.device("cuda:0")  # (a name only: nothing touches the device before main())


class Model(torch.nn.Module):
    def __init__(self, n, seed):
        super().__init__()
        g = torch.Generator(device=dev).manual_seed(seed)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        self._xyz = torch.nn.Parameter(r(n, 3))
        self._features_dc = torch.nn.Parameter(r(n, 1, 3))
        self._features_rest = torch.nn.Parameter(r(n, 15, 3) * 0.1)
        self._opacity = torch.nn.Parameter(r(n, 1) * 2.0)
        self._scaling = torch.nn.Parameter(r(n, 3) * 0.5 - 4.0)
        self._rotation = torch.nn.Parameter(r(n, 4))
        self.percent_dense = 0.01
        names = [("xyz", self._xyz), ("f_dc", self._features_dc), ("f_rest", self._features_rest),
                 ("opacity", self._opacity), ("scaling", self._scaling), ("rotation", self._rotation)]
        self.optimizer = FusedAdam([{"params": [p], "lr": 1e-3, "name": k} for k, p in names], lr=0.0, eps=1e-15)
        for _, p in names:
            self.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.randn_like(p) * 1e-3,
                                       "exp_avg_sq": torch.rand_like(p) * 1e-6}
        self.send_to_gpui_cnt = None
        self.fresh(seed)

    def fresh(self, seed):
        n = self._xyz.shape[0]
        g = torch.Generator(device=dev).manual_seed(seed + 77)
        self.xyz_gradient_accum = torch.rand(n, 1, device=dev, generator=g)
        self.denom = torch.ones(n, 1, device=dev)
        self.max_radii2D = torch.zeros(n, device=dev)
        self.sum_visible_count_in_one_batch = torch.zeros(n, device=dev)

    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)


def event(m, fused):
    D.set_fused_densify(fused)
    gr = (m.xyz_gradient_accum / m.denom.clamp(min=1)).squeeze(1)
    thr = torch.kthvalue(gr[:4_000_000], max(int(0.98 * min(gr.numel(), 4_000_000)), 1)).values.item()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        D.densify_and_prune(m, thr, 0.005, 4.0, None)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    n, events, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import utils.general_utils as utils
    utils.GLOBAL_RANK, utils.WORLD_SIZE = 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1))
    a, b = Model(n, 1), Model(n, 1)
    res = {"rows0": n, "steps_ms": [], "fused_ms": [], "rows_steps": [n], "rows_fused": [n]}
    for ev in range(events):
        for m in (a, b):
            m.fresh(ev)
        torch.manual_seed(ev)
        res["steps_ms"].append(round(event(a, False), 3))
        torch.manual_seed(ev)
        res["fused_ms"].append(round(event(b, True), 3))
        res["rows_steps"].append(int(a._xyz.shape[0]))
        res["rows_fused"].append(int(b._xyz.shape[0]))
        print(ev, res["steps_ms"][-1], res["fused_ms"][-1], res["rows_steps"][-1], res["rows_fused"][-1], flush=True)
    # one instrumented one-pass event: where its time goes (synchronised parts, slower than the event as a whole)
    parts = {}

    def timed(name, fn):
        def w(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*args, **kw)
            torch.cuda.synchronize()
            parts[name] = round(1e3 * (time.perf_counter() - t0), 3)
            return r
        return w

    b.fresh(99)
    P = int(b._xyz.shape[0])
    o_cls, o_plan, o_move = D.densify_classes, dgr.densify_plan, dgr.densify_move
    D.densify_classes, dgr.densify_plan, dgr.densify_move = timed("classes", o_cls), timed("plan", o_plan), \
        timed("move", o_move)
    parts["event"] = round(event(b, True), 3)
    D.densify_classes, dgr.densify_plan, dgr.densify_move = o_cls, o_plan, o_move
    n_new = int(b._xyz.shape[0])
    res["parts_ms"], res["parts_rows"] = parts, [P, n_new]
    row_bytes = 708
    moved = row_bytes * (P + n_new)
    res["move_GBps"] = round(moved / parts["move"] / 1e6, 1)
    # a streaming copy that reads P rows' worth and writes as much: what the memory system gives for the same traffic
    del a
    torch.cuda.empty_cache()
    words = row_bytes * P // 4
    src, dst = torch.empty(words, device=dev), torch.empty(words, device=dev)
    src.normal_()
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["copy_ms"] = [round(t, 3) for t in ts]
    res["copy_GBps"] = round(2 * 4 * words / sorted(ts)[2] / 1e6, 1)
    res["arena_bytes"] = b._row_arena.nbytes()
    print(json.dumps(res))
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
