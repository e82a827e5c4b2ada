"""One-pass densification on the device (densification_ops.densify_and_prune_fused: gsr_densify_plan + gsr_densify_move
on a RowArena) against the step-by-step restatement of the reference (oracle/densify_oracle.py) on a twin model.

Everything is bit-equal -- rows are moved, not recomputed, and torch.normal draws the same samples on the same device --
except the children's positions: the move kernel evaluates R . sample + xyz itself, torch.bmm accumulates in an order
of its own.  Bound per component, in fp64 from the oracle's values: 16 * 2^-24 * (|sample|_1 + |xyz_i|).  The entries of
R are at most 1 in magnitude and carry a few ulp each (four squares and sums, a square root, a division, two more
products and sums), the three-term dot and the final add carry four more roundings, each relative to a partial sum that
|sample|_1 + |xyz_i| bounds."""
import gc

import pytest
import torch

import densification_ops as D
import diff_gaussian_rasterization as dgr
import synthetic_scene as S
from fused_optim import FusedAdam
from oracle import densify_oracle as O

pytestmark = pytest.mark.gpu

EXTENT = 4.0


@pytest.fixture(autouse=True)
def _switch_off():
    D.set_fused_densify(None)
    yield
    D.set_fused_densify(None)


def _model(device, n=30000, seed=0, world=1):
    torch.manual_seed(seed)
    m = S.SyntheticGaussianModel(n, 320, 240, seed=seed, device=device, scale_coef=0.02)
    m.optimizer = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15)
    for _ in range(2):  # populate exp_avg / exp_avg_sq
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.percent_dense = 0.01
    _fresh_statistics(m, seed, world)
    return m


def _fresh_statistics(m, seed, world=None):
    n, device = m._xyz.shape[0], m._xyz.device
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    m.xyz_gradient_accum = torch.rand(n, 1, device=device, generator=g) * 0.001
    m.denom = torch.randint(0, 4, (n, 1), device=device, generator=g).float()  # zeros -> NaN grads -> 0
    m.max_radii2D = torch.rand(n, device=device, generator=g) * 40  # zeroed before the final prune reads it
    m.sum_visible_count_in_one_batch = torch.rand(n, device=device, generator=g)
    if world is not None:
        m.send_to_gpui_cnt = torch.randint(0, 9, (n, world), dtype=torch.int, device=device, generator=g)


def _state(m):
    out = {}
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        out[g["name"]] = p.detach()
        st = m.optimizer.state[p]
        out[g["name"] + ".exp_avg"] = st["exp_avg"]
        out[g["name"] + ".exp_avg_sq"] = st["exp_avg_sq"]
        assert p is getattr(m, D._ATTR[g["name"]])
        assert set(m.optimizer.state.keys()) == {gg["params"][0] for gg in m.optimizer.param_groups}  # re-keyed
    for s in D._STATS:
        out[s] = getattr(m, s)
    return out


def _event_pair(a, b, seed, max_grad, min_opacity, screen, fused=D.densify_and_prune_fused, exact=False):
    """one event on the product model `a` and on the oracle's twin `b` (bit-equal on entry); checks the result and returns
    the largest child-position error as a fraction of its bound.  exact: the step-by-step path is expected (the switch
    is off, or the event falls back): everything is bit-equal, the children's positions included"""
    if exact:
        torch.manual_seed(seed)
        fused(a, max_grad, min_opacity, EXTENT, screen)
        torch.manual_seed(seed)
        O.densify_and_prune(b, max_grad, min_opacity, EXTENT, screen)
        sa, sb = _state(a), _state(b)
        for k in sb:
            assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
        return 0.0, sb["xyz"].shape[0], (None, None)
    with torch.no_grad():  # what the bound needs, from the oracle's side, before the event changes it
        cls, _, _ = D.densify_classes(b, max_grad, min_opacity, EXTENT, screen)
        split, child = (cls & 4) != 0, (cls & 8) != 0
        n_split, n_child = int(split.sum()), int(child.sum())
        torch.manual_seed(seed)
        stds = b.get_scaling[split].repeat(2, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=stds.device), std=stds).double()
        rank_split = (torch.cumsum(split.long(), 0) - split.long())[child]
        parent_xyz = b._xyz.detach()[child].double()
    torch.manual_seed(seed)
    fused(a, max_grad, min_opacity, EXTENT, screen)
    torch.manual_seed(seed)
    O.densify_and_prune(b, max_grad, min_opacity, EXTENT, screen)
    sa, sb = _state(a), _state(b)
    n_new = sb["xyz"].shape[0]
    for k in sb:
        assert sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype, (k, sa[k].shape, sb[k].shape)
        if k != "xyz":
            assert torch.equal(sa[k], sb[k]), k
    first = n_new - 2 * n_child
    assert first >= 0 and torch.equal(sa["xyz"][:first], sb["xyz"][:first])
    worst = 0.0
    if n_child:
        for c in range(2):
            got = sa["xyz"][first + c * n_child: first + (c + 1) * n_child].double()
            want = sb["xyz"][first + c * n_child: first + (c + 1) * n_child].double()
            s = samples[c * n_split + rank_split]
            bound = 16 * 2.0 ** -24 * (s.abs().sum(dim=1, keepdim=True) + parent_xyz.abs())
            ratio = ((got - want).abs() / bound).max().item()
            assert ratio <= 1.0, (c, ratio)
            worst = max(worst, ratio)
    return worst, n_new, (n_split, n_child)


# ------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("P", [1, 5, 4097, 300_001, 2_000_003])
def test_plan_ranks_and_counts_are_exact(device, P):
    g = torch.Generator().manual_seed(P)
    cls = torch.randint(0, 16, (P,), generator=g, dtype=torch.uint8).to(device)
    ranks, split_rows, counts = dgr.densify_plan(cls)
    assert ranks.shape == (4, P) and ranks.dtype == torch.int32 and counts.dtype == torch.int64
    want_counts = []
    for c, bit in enumerate((1, 2, 8, 4)):  # kept original, kept clone, parent with kept children, split parent
        m = ((cls & bit) != 0).long()
        assert torch.equal(ranks[c].long(), torch.cumsum(m, 0) - m), (c, bit)
        want_counts.append(int(m.sum()))
    assert counts.cpu().tolist() == want_counts
    assert torch.equal(split_rows[:want_counts[3]].long(), ((cls & 4) != 0).nonzero().squeeze(1))


def test_plan_of_no_rows(device):
    ranks, split_rows, counts = dgr.densify_plan(torch.empty(0, dtype=torch.uint8, device=device))
    assert ranks.shape == (4, 0) and split_rows.shape == (0,) and counts.cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="no CPU"):
        dgr.densify_plan(torch.zeros(4, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("screen,world", [(20, 1), (None, 2)])
def test_three_events_match_the_reference_restatement(device, screen, world):
    a, b = _model(device, world=world), _model(device, world=world)
    rows, worst = [30000], 0.0
    for ev in range(3):
        ratio, n_new, (n_split, n_child) = _event_pair(a, b, 123 + ev, 0.0002, 0.05, screen)
        assert n_new != rows[-1] and n_split > 0 and n_child > 0
        rows.append(n_new)
        worst = max(worst, ratio)
        with torch.no_grad():
            a._xyz.copy_(b._xyz)  # the later events start bit-equal
        for m in (a, b):
            _fresh_statistics(m, 10 * ev + 1)
    arena = a._row_arena
    assert arena.events == 3
    for name, attr in D._ATTR.items():  # the parameters are views of the arena, alternating halves
        assert arena.half_of((name, None), getattr(a, attr)) == 0  # event 1 -> half 0, 2 -> half 1, 3 -> half 0
    print(f"rows {rows}, child xyz: largest |fused - torch.bmm| / bound = {worst:.4f} (screen {screen})")


# ------------------------------------------------------------------------------------------------------ degenerate
def test_nothing_selected_leaves_the_state_bit_identical(device):
    a, b = _model(device, n=5000), _model(device, n=5000)
    for m in (a, b):
        m.denom = torch.ones_like(m.denom)  # (a zero count under a positive sum is +inf: hot at any threshold)
    before = {k: v.clone() for k, v in _state(a).items()}
    _, n_new, _ = _event_pair(a, b, 1, 1e9, 0.0, None)
    assert n_new == 5000
    for k, v in _state(a).items():
        if k in ("xyz_gradient_accum", "denom", "max_radii2D", "sum_visible_count_in_one_batch"):
            assert not v.any(), k  # the reference zeroes them at every event
        else:
            assert torch.equal(v, before[k]), k


def test_everything_pruned_leaves_no_rows(device):
    a, b = _model(device, n=5000), _model(device, n=5000)
    _, n_new, _ = _event_pair(a, b, 2, 0.0002, 2.0, 20)
    assert n_new == 0 and all(v.shape[0] == 0 for v in _state(a).values())
    # ... and an event on the empty model is an empty event
    D.densify_and_prune_fused(a, 0.0002, 0.05, EXTENT, 20)
    assert all(v.shape[0] == 0 for v in _state(a).values())


@pytest.mark.parametrize("tight", [False, True])
def test_every_row_split_and_forced_growth(device, tight):
    """three events: nothing selected (5000 rows; `tight`: into an arena created at capacity == rows), every row split
    (10000 rows: the arena has to grow, and the half that was read is now too small and is released), a pruning one
    (which has to replace that half at the grown capacity) -- same results as the reference every time"""
    a, b = _model(device, n=5000), _model(device, n=5000)
    arena = D.row_arena(a, capacity=5000 if tight else None)
    assert arena.capacity == (5000 if tight else 5500)
    for m in (a, b):
        m.denom = torch.ones_like(m.denom)  # (a zero count under a positive sum is +inf: hot at any threshold)
    _, n_new, _ = _event_pair(a, b, 2, 1e9, 0.0, None)
    assert n_new == 5000 and arena.growths == 0 and arena._halves[("xyz", None)][0].shape[0] == arena.capacity
    for m in (a, b):
        _fresh_statistics(m, 3)
        m.percent_dense = 0.0  # every scale is "large": hot rows split
        m.denom = torch.ones_like(m.denom)
        m.xyz_gradient_accum = m.xyz_gradient_accum + 1.0
    _, n_new, (n_split, n_child) = _event_pair(a, b, 3, 1e-30, 0.0, None)
    assert (n_new, n_split, n_child) == (10000, 5000, 5000)
    assert arena.growths == 1 and arena.capacity == 11000
    assert arena.half_of(("xyz", None), a._xyz) == 1 and arena._halves[("xyz", None)][0] is None
    with torch.no_grad():
        a._xyz.copy_(b._xyz)
    for m in (a, b):
        _fresh_statistics(m, 5)
        m.percent_dense = 0.01
        m.denom = torch.ones_like(m.denom)
    _, n2, _ = _event_pair(a, b, 4, 1e9, 0.05, None)  # prunes only: fits, so the capacity stays
    assert 0 < n2 < n_new and arena.growths == 1 and arena.half_of(("xyz", None), a._xyz) == 0
    assert all(h.shape[0] == 11000 for hs in arena._halves.values() for h in hs)


# ------------------------------------------------------------------------------------------------------- optimizer
@pytest.mark.parametrize("fuse_backward", [False, True])
def test_optimizer_steps_on_the_arena_views_like_on_dense_tensors(device, fuse_backward):
    """FusedAdam caches pointer tables keyed by addresses; ping-pong brings an address back with another length and a new
    Parameter object.  After event 1 and after event 3 (the same half as event 1) one step on the views must equal the
    same step on dense clones, bit for bit"""
    a = _model(device, n=8000)
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
    for g in a.optimizer.param_groups:
        g["lr"] = lrs[g["name"]]
    a.optimizer.set_fuse_backward(fuse_backward)
    try:
        for ev in range(3):
            torch.manual_seed(ev)
            D.densify_and_prune_fused(a, 0.0002, 0.05, EXTENT, 20)
            _fresh_statistics(a, ev)
            if ev == 1:
                continue
            groups = a.optimizer.param_groups
            for g in groups:
                p = g["params"][0]
                assert p is getattr(a, D._ATTR[g["name"]]) and p.requires_grad and p.grad is None
                assert a._row_arena.half_of((g["name"], None), p) == 0
                st = a.optimizer.state[p]
                assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
            assert len(a.optimizer.state) == 6  # re-keyed: no entry of a replaced Parameter is left
            dense = [torch.nn.Parameter(g["params"][0].detach().clone()) for g in groups]
            ref = FusedAdam([{"params": [q], "lr": g["lr"], "name": g["name"]} for q, g in zip(dense, groups)], lr=0.0,
                            eps=1e-15)
            for q, g in zip(dense, groups):
                st = a.optimizer.state[g["params"][0]]
                ref.state[q] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"].clone(),
                                "exp_avg_sq": st["exp_avg_sq"].clone()}
                grad = torch.randn_like(q)
                q.grad, g["params"][0].grad = grad, grad.clone()
            a.optimizer.step()
            ref.step()
            for q, g in zip(dense, groups):
                p = g["params"][0]
                assert torch.equal(p.detach(), q.detach()), g["name"]
                for k in ("exp_avg", "exp_avg_sq", "step"):
                    assert torch.equal(a.optimizer.state[p][k], ref.state[q][k]), (g["name"], k)
            a.optimizer.zero_grad(set_to_none=True)
    finally:
        a.optimizer.set_fuse_backward(False)


# ---------------------------------------------------------------------------------------------------------- switch
def test_switch_dispatches_and_max_grad_zero_falls_back(device, monkeypatch):
    monkeypatch.delenv("GSR_FUSED_DENSIFY", raising=False)
    a, b = _model(device, n=5000), _model(device, n=5000)
    _event_pair(a, b, 11, 0.0002, 0.05, 20, fused=D.densify_and_prune, exact=True)  # unset: today's path and results
    assert getattr(a, "_row_arena", None) is None
    monkeypatch.setenv("GSR_FUSED_DENSIFY", "1")
    for m in (a, b):
        _fresh_statistics(m, 12)
    # max_grad <= 0: clones may be split, the closed form does not hold -> falls back
    _event_pair(a, b, 13, 0.0, 0.05, 20, fused=D.densify_and_prune, exact=True)
    assert getattr(a, "_row_arena", None) is None
    for m in (a, b):
        _fresh_statistics(m, 14)
    _event_pair(a, b, 15, 0.0002, 0.05, 20, fused=D.densify_and_prune)  # set: the one-pass path
    assert a._row_arena.events == 1 and a._xyz.shape[0] > 0
    # a model whose optimizer has no moments yet falls back as well
    c = S.SyntheticGaussianModel(2000, 320, 240, seed=3, device=device, scale_coef=0.02)
    c.optimizer = FusedAdam(c.param_groups(), lr=0.0, eps=1e-15)
    c.percent_dense = 0.01
    _fresh_statistics(c, 16, world=1)
    D.densify_and_prune(c, 0.0002, 0.05, EXTENT, 20)
    assert getattr(c, "_row_arena", None) is None and c._xyz.shape[0] != 2000


# -------------------------------------------------------------------------------------------------------- training
def test_training_with_one_pass_densification_end_to_end(device):
    """the 60-iteration loop of tests/test_gpu_densify.py::test_training_with_densification_end_to_end under the
    switch: the scene re-sizes, nothing goes non-finite, the loss keeps falling"""
    import utils.general_utils as utils
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.loss_distribution import batched_loss_computation, load_camera_from_cpu_to_all_gpu
    from gaussian_renderer.workload_division import (DivisionStrategyHistoryFinal, finish_strategy_final,
                                                     start_strategy_final)

    D.set_fused_densify(True)
    N, W, H = 15000, 320, 208
    utils.GLOBAL_RANK, utils.WORLD_SIZE = 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    cams = S.orbit_cameras(8, W, H, device=device)[:3]
    bg = torch.zeros(3, device=device)
    pipe = type("P", (), {"debug": False})()
    teacher = S.SyntheticGaussianModel(N, W, H, seed=11, device=device, scale_coef=0.01)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    with torch.no_grad():
        for cam in cams:
            st, _ = start_strategy_final([cam], hist)
            pkg = distributed_preprocess3dgs_and_all2all_final([cam], teacher, pipe, bg, batched_strategies=st,
                                                               mode="test")
            cam.original_image_backup = (render_final(pkg, st)[0][0].clamp(0, 1) * 255).round().to(torch.uint8)
    m = S.SyntheticGaussianModel(N, W, H, seed=11, device=device, scale_coef=0.01)  # the teacher, perturbed
    with torch.no_grad():
        g = torch.Generator().manual_seed(0)
        m._features_dc += 1.0 * torch.randn(m._features_dc.shape, generator=g).to(device)
        m._opacity += 0.5 * torch.randn(m._opacity.shape, generator=g).to(device)
        m._xyz += 0.01 * torch.randn(m._xyz.shape, generator=g).to(device)
    m.optimizer = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15)
    m.percent_dense = 0.01
    m.xyz_gradient_accum = torch.zeros(N, 1, device=device)
    m.denom = torch.zeros(N, 1, device=device)
    m.max_radii2D = torch.zeros(N, device=device)
    m.sum_visible_count_in_one_batch = torch.zeros(N, device=device)
    m.send_to_gpui_cnt = torch.zeros(N, 1, dtype=torch.int, device=device)
    sizes, losses = [N], []
    for it in range(60):
        cam = cams[it % 3]
        utils.set_cur_iter(it + 1)
        st, tasks = start_strategy_final([cam], hist)
        load_camera_from_cpu_to_all_gpu([cam], st, tasks)
        pkg = distributed_preprocess3dgs_and_all2all_final([cam], m, pipe, bg, batched_strategies=st)
        images, masks = render_final(pkg, st)
        stats = [c["stats_collector"] for c in pkg["batched_cuda_args"]]
        loss, _ = batched_loss_computation(images, [cam], masks, st, stats)
        loss.backward()
        finish_strategy_final([cam], hist, st, stats)
        losses.append(loss.item())
        with torch.no_grad():  # densification.py:13-25
            vis = pkg["batched_locally_preprocessed_visibility_filter"][0]
            radii = pkg["batched_locally_preprocessed_radii"][0]
            m.max_radii2D[vis] = torch.max(m.max_radii2D[vis], radii[vis].float())
            D.add_densification_stats(m, pkg["batched_locally_preprocessed_mean2D"][0], vis)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        cam.original_image = None
        if it in (19, 39):
            with torch.no_grad():  # threshold at the 95th percentile of the accumulated statistic: ~5 % densify
                gr = (m.xyz_gradient_accum / m.denom.clamp(min=1)).squeeze(1)
                thr = torch.quantile(gr[m.denom.squeeze(1) > 0], 0.95).item()
                D.densify_and_prune(m, thr, 0.005, 4.0, None)
            sizes.append(m._xyz.shape[0])
            for name in D._STATS:
                assert getattr(m, name).shape[0] == m._xyz.shape[0], name
    assert m._row_arena.events == 2                         # the events took the one-pass path
    assert len(set(sizes)) > 1, sizes                       # the scene was actually re-sized
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert all(l == l for l in losses)
    assert sum(losses[-6:]) < sum(losses[:6]), (losses[:6], losses[-6:])  # still improving after two re-sizings


# --------------------------------------------------------------------------------------------------------- replays
def test_replays_resume_after_one_pass_events(device):
    """the scenario of tests/test_gpu_graphed_step.py::test_replays_survive_densification_events under the switch: the
    statistics are one launch inside the replayed iteration, an event runs after GraphedIteration.reset() -- the graphs
    hold views of the half the event is about to overwrite one event later -- and the loop is back on replays"""
    import gaussian_renderer as gr
    import utils.general_utils as utils
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.loss_distribution import batched_loss_computation, load_camera_from_cpu_to_all_gpu
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final
    from graphed_step import GraphedIteration

    D.set_fused_densify(True)
    N, W, H = 60000, 640, 368
    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    gr._PLANNERS.clear()
    gr.set_exchange_forced(False)
    cams = S.orbit_cameras(4, W, H, device=device)
    for k, c in enumerate(cams):
        c.original_image_backup = S.make_gt_image(W, H, seed=30 + k, device=device)
    dgr.release_workspaces()
    model = S.SyntheticGaussianModel(N, W, H, seed=9, device=device, scale_coef=0.008)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    bg = torch.tensor([0.1, 0.2, 0.3], device=device)
    pipe = type("P", (), {"debug": False})()
    opt = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, grad_scale=1.0)
    for g in opt.param_groups:
        if g["name"] == "xyz":
            g["lr"] = 0.00016
    model.optimizer, model.percent_dense = opt, 0.01
    n = model._xyz.shape[0]
    model.xyz_gradient_accum = torch.zeros((n, 1), device=device)
    model.denom = torch.zeros((n, 1), device=device)
    model.max_radii2D = torch.zeros((n,), device=device)
    model.sum_visible_count_in_one_batch = torch.zeros((n,), device=device)
    model.send_to_gpui_cnt = None

    def body(batch, strategies, tasks):
        load_camera_from_cpu_to_all_gpu(batch, strategies, tasks)
        pkg = distributed_preprocess3dgs_and_all2all_final(batch, model, pipe, bg, batched_strategies=strategies,
                                                           mode="train")
        images, masks = render_final(pkg, strategies)
        stats = [ca["stats_collector"] for ca in pkg["batched_cuda_args"]]
        loss, _ = batched_loss_computation(images, batch, masks, strategies, stats)
        loss.backward()
        with torch.no_grad():
            D.update_densification_stats(model, pkg["batched_locally_preprocessed_mean2D"][0],
                                         pkg["batched_locally_preprocessed_radii"][0])
        opt.step()
        opt.zero_grad(set_to_none=True)
        return loss

    step = GraphedIteration(opt, body, warmup=2, enabled=True)
    rows, losses = [n], []
    try:
        for it in range(1, 41):
            batch = [cams[it % len(cams)]]
            utils.set_cur_iter(utils.get_cur_iter() + 1)
            strategies, tasks = start_strategy_final(batch, hist)
            loss = step(batch, strategies, tasks)
            if it % 10 == 0:
                redo = step.reset()  # validates the iteration in flight, then drops the graphs
                loss = redo if redo is not None else loss
                with torch.no_grad():
                    gr_ = (model.xyz_gradient_accum / model.denom.clamp(min=1)).squeeze(1)
                    thr = torch.kthvalue(gr_, max(int(0.97 * gr_.numel()), 1)).values.item()
                    D.densify_and_prune(model, max(thr, 1e-30), 0.005, 4.0, None)
                rows.append(int(model._xyz.shape[0]))
            if it % 10 in (0, 9):
                redo = step.validate()
                losses.append(float((redo if redo is not None else loss).detach()))
        step.validate()
        torch.cuda.synchronize()
    finally:
        opt.set_fuse_backward(False)
        # the graphs go now: left to the garbage collector they would be destroyed at an arbitrary later moment, possibly
        # in the middle of another test's stream capture (which aborts the process)
        step.reset()
        gc.collect()
        torch.cuda.synchronize()
    st = dict(step.stats)
    print("rows", rows, "stats", st)
    assert model._row_arena.events == 4
    assert st["disabled"] is None, st
    assert st["captured"] >= 4 and st["replayed"] >= 20, st  # one capture per shard size, replays in between
    assert len(rows) == 5 and all(r != rows[0] for r in rows[1:])  # the events really changed the shard
    assert all(l == l for l in losses) and all(torch.isfinite(p).all() for p in model.parameters())
    assert opt.fused_steps > 0
    del step, body, opt
    model.optimizer = None
    gc.collect()
