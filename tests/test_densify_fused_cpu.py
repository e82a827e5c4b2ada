"""One-pass densification, the parts that need no GPU: argument validation of gsr_densify_plan / gsr_densify_move, the
class codes and the closed-form layout (densification_ops.densify_classes + a torch restatement of what the plan and
the move compute) against the step-by-step restatement of the reference (oracle/densify_oracle.py) -- bit for bit,
child positions included, because here the same torch operations compute them -- and the RowArena on CPU tensors."""
import ctypes

import pytest
import torch

import densification_ops as D
import diff_gaussian_rasterization as dgr
import synthetic_scene as S
from oracle import densify_oracle as O
from row_arena import RowArena


def test_entry_points_validate_before_any_device_work():
    lib = dgr._lib.lib
    prev = 0
    for P in (0, 1, 2047, 2048, 2049, 300_001, 40_000_000, 2**31 - 1):
        n = lib.gsr_densify_plan_bytes(P)
        assert n > 0 and n >= prev, (P, n)
        prev = n
    assert lib.gsr_densify_plan_bytes(-1) == 0
    one = ctypes.c_void_p(64)  # never dereferenced: every call below returns before any device work
    assert lib.gsr_densify_plan(-1, one, one, one, one, one, 1 << 20, None) == -1
    assert lib.gsr_densify_plan(2**31, one, one, one, one, one, 1 << 40, None) == -1
    assert lib.gsr_densify_plan(10, None, one, one, one, one, 1 << 20, None) == -1
    assert lib.gsr_densify_plan(10, one, None, one, one, one, 1 << 20, None) == -1
    assert lib.gsr_densify_plan(10, one, one, one, None, one, 1 << 20, None) == -1
    assert lib.gsr_densify_plan(10, one, one, one, one, None, 1 << 20, None) == -1
    assert lib.gsr_densify_plan(0, None, None, None, None, None, 0, None) == 0
    assert lib.gsr_densify_plan(10, one, one, one, one, one, lib.gsr_densify_plan_bytes(10) - 1, None) == -2
    assert lib.gsr_densify_plan(10**6, one, one, None, one, one, lib.gsr_densify_plan_bytes(10**6) - 1, None) == -2

    VP, I32, I64 = ctypes.c_void_p * 2, ctypes.c_int32 * 2, ctypes.c_int64 * 2

    def move(P=10, n=(4, 1, 1, 2), copies=2, K=2, srcs=VP(64, 64), dsts=VP(64, 64), alts=VP(64, 64), widths=(3, 3),
             roles=(0, 1), ss=(3, 3), ds=(3, 3), dst_rows=100, cls=one, ranks=one, rot=one, samples=one):
        return lib.gsr_densify_move(P, cls, ranks, n[0], n[1], n[2], n[3], copies, K, srcs, dsts, alts, I32(*widths),
                                    I32(*roles), I64(*ss), I64(*ds), dst_rows, rot, samples, None)

    assert move(P=0, n=(0, 0, 0, 0), cls=None, ranks=None, srcs=None, dsts=None, alts=None) == 0
    assert move(K=0) == 0
    assert move(P=-1) == -1
    assert move(n=(-1, 0, 0, 0)) == -1
    assert move(n=(11, 0, 0, 0)) == -1          # more kept originals than rows
    assert move(n=(4, 1, 3, 2)) == -1           # more parents with children than split rows
    assert move(dst_rows=6) == -1               # 4 + 1 + 2 * 1 rows do not fit
    assert move(copies=0) == -1
    assert move(K=33) == -1
    assert move(cls=None) == -1
    assert move(ranks=None) == -1
    assert move(srcs=VP(64, None)) == -1
    assert move(dsts=VP(None, 64)) == -1
    assert move(widths=(3, 0)) == -1
    assert move(roles=(0, 4)) == -1
    assert move(ss=(2, 3)) == -1                # rows would overlap
    assert move(roles=(2, 1), widths=(4, 3), ss=(4, 3), ds=(4, 3)) == -1    # xyz rows are 3 wide
    assert move(roles=(2, 1), rot=None) == -1
    assert move(roles=(2, 1), samples=None) == -1
    assert move(roles=(3, 1), alts=VP(None, 64)) == -1
    assert move(roles=(3, 1), alts=None) == -1
    assert lib.gsr_abi_version() == 15          # new symbols only


def _cpu_model(n, seed, world):
    torch.manual_seed(seed)
    m = S.SyntheticGaussianModel(n, 320, 240, seed=seed, device="cpu", scale_coef=0.02)
    m.optimizer = torch.optim.Adam(m.param_groups(), lr=0.0, eps=1e-15)
    for _ in range(2):
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.percent_dense = 0.01
    m.xyz_gradient_accum = torch.rand(n, 1) * 0.001
    m.denom = torch.randint(0, 4, (n, 1)).float()
    m.max_radii2D = torch.rand(n) * 40  # the reference zeroes it before the final prune reads it: must not matter
    m.sum_visible_count_in_one_batch = torch.rand(n)
    m.send_to_gpui_cnt = torch.randint(0, 9, (n, world), dtype=torch.int)
    return m


def _layout(m, cls, child_scaling, N=2):
    """what gsr_densify_plan + gsr_densify_move compute, in torch: name -> tensor of the new length"""
    orig, clone, split, child = ((cls & b) != 0 for b in (1, 2, 4, 8))
    rank_split = torch.cumsum(split.long(), 0) - split.long()
    n_split = int(split.sum())
    stds = m.get_scaling[split].repeat(N, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3)), std=stds)
    parent = child.nonzero().squeeze(1)
    take = torch.cat([samples[c * n_split + rank_split[parent]] for c in range(N)])
    rots = O.build_rotation(m._rotation[parent]).repeat(N, 1, 1)
    child_xyz = torch.bmm(rots, take.unsqueeze(-1)).squeeze(-1) + m._xyz[parent].repeat(N, 1)
    out = {}
    for g in m.optimizer.param_groups:
        p, st = g["params"][0], m.optimizer.state[g["params"][0]]
        kids = {"xyz": child_xyz, "scaling": child_scaling[parent].repeat(N, 1)}.get(g["name"])
        kids = kids if kids is not None else p[parent].repeat(N, *([1] * (p.dim() - 1)))
        out[g["name"]] = torch.cat((p[orig], p[clone], kids)).detach()
        for k in ("exp_avg", "exp_avg_sq"):
            out[g["name"] + "." + k] = torch.cat((st[k][orig], torch.zeros_like(st[k][clone]), torch.zeros_like(kids)))
    out["send_to_gpui_cnt"] = torch.cat((m.send_to_gpui_cnt[orig], m.send_to_gpui_cnt[clone],
                                         m.send_to_gpui_cnt[parent].repeat(N, 1)))
    return out


@pytest.mark.parametrize("n,screen,world", [(1, 20, 1), (1, 20, 2), (7, None, 2), (7, 20, 1), (5000, 20, 1),
                                            (5000, None, 2), (20000, 20, 2), (20000, None, 1)])
def test_classes_and_layout_match_the_step_by_step_reference(n, screen, world):
    # (one row with max_screen_size None is left out: the restatement's `.squeeze()` then makes the prune mask 0-dim and
    # its boolean indexing returns [0, 1, 3] tensors -- a shape of that corner, not a result to reproduce)
    a, b = _cpu_model(n, n, world), _cpu_model(n, n, world)
    extent = 4.0
    with torch.no_grad():
        cls, child_scaling, _ = D.densify_classes(a, 0.0002, 0.05, extent, screen)
        assert cls.dtype == torch.uint8 and cls.shape == (n,) and child_scaling.shape == (n, 3)
        assert not ((cls & 2) != 0).logical_and((cls & 4) != 0).any()  # clone and split exclude each other
        assert not ((cls & 8) != 0).logical_and((cls & 4) == 0).any()  # only split rows have children
        torch.manual_seed(7)
        got = _layout(a, cls, child_scaling)
    torch.manual_seed(7)
    O.densify_and_prune(b, 0.0002, 0.05, extent, screen)
    n_new = b._xyz.shape[0]
    for g in b.optimizer.param_groups:
        p = g["params"][0]
        assert torch.equal(got[g["name"]], p.detach()), g["name"]
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got[g["name"] + "." + k], b.optimizer.state[p][k]), (g["name"], k)
    assert torch.equal(got["send_to_gpui_cnt"], b.send_to_gpui_cnt)
    for s in ("xyz_gradient_accum", "denom", "max_radii2D", "sum_visible_count_in_one_batch"):
        assert getattr(b, s).shape[0] == n_new and not getattr(b, s).any()  # all zero at the new length
    if n >= 5000:
        assert n_new != n and ((cls & 2) != 0).any() and ((cls & 8) != 0).any() and ((cls & 1) == 0).any()


def test_switch_is_off_by_default_and_read_at_call_time(monkeypatch):
    monkeypatch.delenv("GSR_FUSED_DENSIFY", raising=False)
    D.set_fused_densify(None)
    assert not D.fused_densify_enabled()
    monkeypatch.setenv("GSR_FUSED_DENSIFY", "1")
    assert D.fused_densify_enabled()
    monkeypatch.setenv("GSR_FUSED_DENSIFY", "0")
    assert not D.fused_densify_enabled()
    D.set_fused_densify(True)
    assert D.fused_densify_enabled()
    D.set_fused_densify(False)
    monkeypatch.setenv("GSR_FUSED_DENSIFY", "1")
    assert not D.fused_densify_enabled()
    D.set_fused_densify(None)


def test_row_arena_views_halves_growth_and_statistics():
    arena = RowArena(100, "cpu")
    assert arena.capacity == 110
    ext = torch.arange(300.0).reshape(100, 3)            # the tensor the model was built with: outside the arena
    assert arena.half_of("xyz", ext) is None
    d0 = arena.destination("xyz", ext, 105)
    assert d0.shape == (110, 3) and d0.dtype == ext.dtype
    v0 = d0[:105]
    assert arena.half_of("xyz", v0) == 0
    v0.fill_(1.0)
    assert float(d0[:105].sum()) == 315.0                # the view aliases the arena
    d1 = arena.destination("xyz", v0, 108)               # an event alternates halves
    assert arena.half_of("xyz", d1[:108]) == 1 and d1.data_ptr() != d0.data_ptr()
    d2 = arena.destination("xyz", d1[:108], 90)
    assert d2.data_ptr() == d0.data_ptr()                # ... and comes back: nothing new was allocated
    assert arena.growths == 0 and arena.capacity == 110
    # int tensors and other row shapes get halves of their own
    c = arena.destination("cnt", torch.zeros(100, 2, dtype=torch.int32), 105)
    assert c.shape == (110, 2) and c.dtype == torch.int32
    # growth: an arena created at capacity == rows must grow at the first event that adds a row
    tight = RowArena(100, "cpu", capacity=100)
    src = torch.zeros(100, 3)
    assert tight.destination("xyz", src, 100).shape[0] == 100 and tight.growths == 0
    g = tight.destination("xyz", tight.destination("xyz", src, 100)[:100], 101)
    assert tight.growths == 1 and tight.capacity == 150 and g.shape[0] == 150
    live = g[:101]
    tight.release_other("xyz", live)                     # the half that was read is too small for the next event
    assert tight._halves["xyz"][tight.half_of("xyz", live)] is g
    assert tight._halves["xyz"][1 - tight.half_of("xyz", live)] is None
    back = tight.destination("xyz", live, 120)           # ... which allocates it at the grown capacity
    assert back.shape[0] == 150 and back.data_ptr() != g.data_ptr()
    big = tight.destination("xyz", back[:120], 1000)     # far beyond: 1.1 x rows wins over 1.5 x capacity
    assert tight.capacity == 1100 and big.shape[0] == 1100
    # the statistics are zero-filled views of reserved buffers
    z = arena.zeros("denom", 105, (1,))
    assert z.shape == (105, 1) and not z.any()
    z += 3.0
    z2 = arena.zeros("denom", 108, (1,))
    assert z2.data_ptr() == z.data_ptr() and z2.shape == (108, 1) and not z2.any()
    assert arena.zeros("max_radii2D", 108).shape == (108,)
    s = arena.scratch("ranks", 400, torch.int32)
    assert arena.scratch("ranks", 300, torch.int32) is s and arena.scratch("ranks", 500, torch.int32) is not s
    assert arena.nbytes() > 0


def _plan_stand_in(cls, ranks=None, split_rows=None, workspace=None):
    P = cls.shape[0]
    masks = [((cls & bit) != 0).long() for bit in (1, 2, 8, 4)]
    rk = torch.stack([torch.cumsum(m, 0) - m for m in masks]).to(torch.int32)
    rows = torch.zeros(max(P, 1), dtype=torch.int32)
    sel = masks[3].nonzero().squeeze(1)
    rows[:sel.numel()] = sel.to(torch.int32)
    return rk, rows[:P], torch.stack([m.sum() for m in masks])


def _move_stand_in(cls, ranks, counts, srcs, dsts, roles, alts=None, rotation=None, samples=None, copies=2):
    n_orig, n_clone, n_child, n_split = counts
    orig, clone, child = ((cls & b) != 0 for b in (1, 2, 8))
    parent = child.nonzero().squeeze(1)
    for s, d, role, alt in zip(srcs, dsts, roles, alts):
        assert s.untyped_storage().data_ptr() != d.untyped_storage().data_ptr()  # never in place
        d[:n_orig] = s[orig]
        d[n_orig:n_orig + n_clone] = 0 if role == 1 else s[clone]
        for c in range(copies):
            if role == 1:
                kids = torch.zeros_like(s[parent])
            elif role == 2:
                smp = samples[c * n_split + ranks[3][parent].long()]
                kids = torch.bmm(O.build_rotation(rotation[parent]), smp.unsqueeze(-1)).squeeze(-1) + s[parent]
            else:
                kids = alt[parent] if role == 3 else s[parent]
            lo = n_orig + n_clone + c * n_child
            d[lo:lo + n_child] = kids
    return n_orig + n_clone + copies * n_child


@pytest.mark.parametrize("screen,world", [(20, 2), (None, 1)])
def test_host_side_of_the_event_with_torch_stand_ins_for_the_two_launches(monkeypatch, screen, world):
    """densify_and_prune_fused on CPU models, gsr_densify_plan / gsr_densify_move replaced by torch restatements: the
    class codes, the one read-back, the sample draw, the arena and the optimizer surgery over three events, against the
    step-by-step reference -- bit for bit"""
    monkeypatch.setattr(dgr, "densify_plan", _plan_stand_in)
    monkeypatch.setattr(dgr, "densify_move", _move_stand_in)
    a, b = _cpu_model(4000, 5, world), _cpu_model(4000, 5, world)
    rows = [4000]
    for ev in range(3):
        torch.manual_seed(40 + ev)
        D.densify_and_prune_fused(a, 0.0002, 0.05, 4.0, screen)
        torch.manual_seed(40 + ev)
        O.densify_and_prune(b, 0.0002, 0.05, 4.0, screen)
        n = b._xyz.shape[0]
        assert n != rows[-1]
        rows.append(n)
        arena = a._row_arena
        for ga, gb in zip(a.optimizer.param_groups, b.optimizer.param_groups):
            pa, pb = ga["params"][0], gb["params"][0]
            assert pa is getattr(a, D._ATTR[ga["name"]]) and pa.requires_grad
            assert arena.half_of((ga["name"], None), pa) == ev % 2  # a view of the arena, alternating halves
            assert torch.equal(pa.detach(), pb.detach()), ga["name"]
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(a.optimizer.state[pa][k], b.optimizer.state[pb][k]), (ga["name"], k)
            assert a.optimizer.state[pa]["step"] == b.optimizer.state[pb]["step"]
        assert len(a.optimizer.state) == 6
        for s in D._STATS:
            assert torch.equal(getattr(a, s), getattr(b, s)), s
        for m in (a, b):  # fresh statistics for the next event
            g = torch.Generator().manual_seed(ev)
            m.xyz_gradient_accum = torch.rand(n, 1, generator=g) * 0.001
            m.denom = torch.randint(0, 4, (n, 1), generator=g).float()
    assert a._row_arena.events == 3
    # and the model keeps training: one Adam step on the views
    for p in a.parameters():
        p.grad = torch.ones_like(p)
    a.optimizer.step()


def test_classes_use_the_models_own_activation_pair():
    """a model whose scaling activation is not exp: the children's raw scale goes through ITS inverse, and the child drop
    test through ITS activation, so the getter sees get_scaling / (0.8 N) again"""
    m = _cpu_model(500, 3, 1)
    with torch.no_grad():
        m._scaling.copy_(torch.exp(m._scaling) ** 0.5)  # raw parameter of a square activation with the same get_scaling
    m.scaling_activation = lambda x: x * x
    m.scaling_inverse_activation = torch.sqrt
    type(m).get_scaling = property(lambda self: self.scaling_activation(self._scaling))
    try:
        with torch.no_grad():
            cls, child_scaling, scaling = D.densify_classes(m, 0.0002, 0.05, 4.0, 20)
        assert torch.equal(scaling, m._scaling.detach() ** 2)
        assert torch.equal(child_scaling, torch.sqrt(scaling / 1.6))
        big = (child_scaling * child_scaling).max(dim=1).values > 0.4
        low = (m.get_opacity < 0.05).reshape(-1)
        split = (cls & 4) != 0
        assert torch.equal((cls & 8) != 0, split & ~(big | low))
    finally:
        type(m).get_scaling = property(lambda self: torch.exp(self._scaling))
