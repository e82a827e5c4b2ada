"""-m gpu: the 3D smoothing filter (csrc/filter3d.hip) kernel by kernel against tests/filter3d_refs.py, and through the
Python layers: diff_gaussian_rasterization.compute_filter3d / filter3d_apply, filter3d.compute_3D_filter / bake,
gaussian_renderer.set_filter3d, FusedAdam, GraphedIteration.

Distance kernel.  N in {1, 63, 64, 65, 257, 4099} x C in {1, 2, 37}, and C = 64, 65 and 129 around the kernel's camera
chunk (F3D_CAM_CHUNK = 64 cameras staged in LDS per pass: 64 fills one pass exactly, 65 starts a second pass with one
camera, 129 a third).  `seen` is exact (the builder keeps every inequality 1e-4 away from equality); the filter is within
2 ulp of float32(sqrt(0.2)) dist / focal_max formed in float32 from the kernel's own dist, and within
8 x 2^-24 x sum|terms of t.z| x sqrt(0.2) / focal_max of the float64 rule.

Apply kernels.  Every element against float64, in units of 2^-24 M, M = the sum of the magnitudes of the addends the
float64 formula forms the element from.  The tolerance is twice the error of a float32 numpy evaluation of the kernels'
formulas on the same inputs (tests/filter3d_refs.py: apply_*_f32; computed on the host, no code under test) -- device
and numpy logf / expf may differ by an ulp each.  Measured, worst over N in {1, 63, 65, 1000}, in those units:
                   numpy float32    MI355X kernel
    scaling_eff        1.03             1.14
    opacity_eff        2.43             2.92
    d_scaling          3.68             3.68
    d_opacity          3.74             3.47
Rows with f == 0 keep their bits, forward and backward."""
import math

import numpy as np
import pytest
import torch

import filter3d_refs as R
import synthetic_scene as S

pytestmark = pytest.mark.gpu

SHAPES = [(N, C) for N in (1, 63, 64, 65, 257, 4099) for C in (1, 2, 37)] + \
         [(257, R.CAM_CHUNK), (257, R.CAM_CHUNK + 1), (65, 2 * R.CAM_CHUNK + 1)]
ALL = ["_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ulps(a, b):
    """distance in float32 ulps between two float32 arrays of one sign"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _run_distance(case, device, hook=None, rows=slice(None)):
    import diff_gaussian_rasterization as dgr

    xyz = torch.from_numpy(case["xyz"][rows]).to(device)
    cams = torch.from_numpy(case["cams"]).to(device)
    fm = dgr.filter3d_focal_max(case["cams"][:, 35], case["W"])
    f, dist, seen = dgr.compute_filter3d(xyz, cams, case["W"], case["H"], all_reduce_max=hook, focal_max=fm,
                                         return_parts=True)
    torch.cuda.synchronize()
    return f.cpu().numpy(), dist.cpu().numpy(), seen.cpu().numpy(), fm


def _check_distance(case, got, ref):
    f, dist, seen, fm = got
    N = case["xyz"].shape[0]
    assert f.shape == (N, 1) and f.dtype == np.float32 and dist.shape == (N,) and seen.dtype == np.uint8
    f = f[:, 0]
    assert np.array_equal(seen.astype(bool), ref["seen"]), "seen differs from the float64 rule"
    assert not np.any(dist[~ref["seen"]]) and np.all(dist[ref["seen"]] > np.float32(0.2))
    # the filter from the kernel's own distances, formed in float32
    gmax = dist.max() if ref["seen"].any() else np.float32(0)
    d = np.where(ref["seen"], dist, gmax).astype(np.float32)
    want = ((np.float32(R.K_FILTER) * d) / np.float32(fm)).astype(np.float32) if gmax > 0 else np.zeros(N, np.float32)
    assert int(_ulps(f, want).max()) <= 2
    # unseen rows: one value, that of the farthest seen row
    if (~ref["seen"]).any():
        u = f[~ref["seen"]]
        assert np.all(u.view(np.int32) == u.view(np.int32)[0])
        assert u[0] == (f[ref["seen"]].max() if ref["seen"].any() else 0.0)
    err = np.abs(f.astype(np.float64) - ref["filter"])
    assert np.all(err <= ref["tol"]), f"worst error / bound {float((err / np.maximum(ref['tol'], 1e-300)).max()):.3g}"
    return float((err / np.maximum(ref["tol"], 1e-300)).max()) if N else 0.0


@pytest.mark.parametrize("N,C", SHAPES)
def test_distance_kernel_against_the_float64_rule(device, N, C):
    case = R.build_distance_case(N, C, seed=N + C)
    ref = R.filter_ref(case["xyz"], case["cams"], case["W"], case["H"])
    worst = _check_distance(case, _run_distance(case, device), ref)
    print(f"FILTER3D distance N={N} C={C}: seen {int(ref['seen'].sum())}, seen by one {int((ref['n_valid'] == 1).sum())}, "
          f"worst error / bound {worst:.3g}")
    if N >= 257:
        assert 0 < ref["seen"].sum() < N


def test_distance_kernel_intended_rows(device):
    """camera 0 alone: the row inside the 15 % margin is seen, the one just outside is not, and so on"""
    case = R.build_distance_case(257, 1, seed=3)
    ref = R.filter_ref(case["xyz"], case["cams"], case["W"], case["H"])
    _, dist, seen, _ = got = _run_distance(case, device)
    _check_distance(case, got, ref)
    sp = case["special"]
    assert [int(seen[sp[k]]) for k in R.SPECIAL] == [1, 0, 1, 1, 0, 0]
    assert abs(float(dist[sp["inside_margin"]]) - 5.0) < 1e-4 and abs(float(dist[sp["near_in"]]) - 0.25) < 1e-5


def test_nothing_seen_is_the_identity_filter(device):
    for N, C in ((257, 2), (4099, 37), (63, 0)):
        case = R.build_distance_case(N, C, seed=1, unseen=True)
        ref = R.filter_ref(case["xyz"], case["cams"], case["W"], case["H"])
        assert not ref["seen"].any()
        import diff_gaussian_rasterization as dgr

        f, dist, seen = dgr.compute_filter3d(torch.from_numpy(case["xyz"]).to(device),
                                             torch.from_numpy(case["cams"]).to(device), case["W"], case["H"],
                                             focal_max=100.0, return_parts=True)
        assert not bool(_bits(f).any()) and not bool(seen.any()) and not bool(_bits(dist).any())


def test_distance_equals_k1_depths_bit_for_bit(device):
    """a row seen by exactly one camera: dist is what K1 writes to `depths` for that camera"""
    import diff_gaussian_rasterization as dgr

    case = R.build_distance_case(4099, 2, seed=7)  # (two cameras: most seen rows are seen by exactly one)
    ref = R.filter_ref(case["xyz"], case["cams"], case["W"], case["H"])
    _, dist, seen, _ = _run_distance(case, device)
    N = case["xyz"].shape[0]
    g = torch.Generator().manual_seed(9)
    scaling = torch.log(0.02 + 0.05 * torch.rand(N, 3, generator=g)).to(device)
    rotation = torch.nn.functional.normalize(torch.randn(N, 4, generator=g)).to(device)
    dc, rest = torch.rand(N, 1, 3, generator=g).to(device), 0.1 * torch.randn(N, 15, 3, generator=g).to(device)
    opacity = torch.randn(N, 1, generator=g).to(device)
    with torch.no_grad():
        _, _, _, radii, depths = dgr.preprocess_gaussians_raw_batched(
            torch.from_numpy(case["xyz"]).to(device), scaling, rotation, dc, rest, opacity,
            torch.from_numpy(case["cams"]).to(device), 3, 1.0, case["W"], case["H"])
    radii, depths = torch.stack(radii).cpu().numpy(), torch.stack(depths).cpu().numpy()  # [C,N]
    one = np.nonzero(ref["n_valid"] == 1)[0]
    cam = ref["valid"][one].argmax(1)
    drawn = radii[cam, one] > 0  # (K1 leaves depth 0 for a row it culls for another reason)
    assert drawn.sum() > 50
    assert np.array_equal(dist[one][drawn].view(np.int32), depths[cam, one][drawn].view(np.int32))
    # and for every seen row: the smallest K1 depth among its valid cameras
    k1 = np.where(ref["valid"].T & (radii > 0), depths, np.inf).min(0)
    all_drawn = ref["seen"] & (np.where(ref["valid"].T, radii > 0, True).all(0))
    assert all_drawn.sum() > 100 and np.array_equal(dist[all_drawn].view(np.int32),
                                                    k1[all_drawn].astype(np.float32).view(np.int32))


def test_two_shards_with_the_max_hook_concatenate_to_one_rank(device):
    """world size 2 on tests/fake_world.py, through filter3d.compute_3D_filter: shard 1 holds only rows that no camera
    sees, so its filter is the other shard's largest distance, which only the MAX all-reduce can tell it"""
    import torch.distributed as dist

    import filter3d as F
    from fake_world import FakeWorld

    W, H = 64, 48
    cams = R.make_cameras(5, W, H, seed=2)
    block = R.pack_cameras(cams)
    a = R.build_distance_case(300, 5, seed=2)
    b = R.build_distance_case(200, 5, seed=2, unseen=True)
    assert np.array_equal(a["cams"], block) and np.array_equal(b["cams"], block)
    shards = [a["xyz"], b["xyz"]]
    full = dict(xyz=np.concatenate(shards), cams=block, W=W, H=H)
    ref = R.filter_ref(full["xyz"], block, W, H)
    assert ref["seen"][:300].any() and not ref["seen"][300:].any()
    one = _run_distance(full, device)
    _check_distance(full, one, ref)
    fw = FakeWorld(2, device)
    dev_cams = [c.to(device) for c in R.make_cameras(5, W, H, seed=2)]

    def rank_main(rank):
        pc = type("PC", (), {})()
        pc._xyz = torch.from_numpy(shards[rank]).to(device)
        before = len(fw.log)
        f = F.compute_3D_filter(pc, dev_cams, group=fw.groups[rank])
        assert f is pc.filter_3D and f.shape == (shards[rank].shape[0], 1)
        return f.clone(), len(fw.log) - before

    res = fw.run(rank_main, timeout=120)
    got = torch.cat([r[0] for r in res]).cpu().numpy()
    assert np.array_equal(got.view(np.int32), one[0].view(np.int32))
    assert bool(got[300:].any()) and res[0][1] == res[1][1] >= 1, "no collective ran"
    # without the hook the second shard would have seen nothing at all
    alone = _run_distance(full, device, rows=slice(300, None))
    assert not alone[0].any()
    assert dist.ReduceOp.MAX is not None


# ------------------------------------------------------------------------------------------------ apply kernels
@pytest.fixture(scope="module")
def f32_error():
    """the float32 numpy evaluation's worst error per output, in units of 2^-24 M, over the four sizes: computed once on
    the host from tests/filter3d_refs.py alone"""
    worst = {"scaling_eff": 0.0, "opacity_eff": 0.0, "d_scaling": 0.0, "d_opacity": 0.0}
    for N in (1, 63, 65, 1000):
        c = R.build_apply_case(N)
        s, q, Ms, Mo = R.apply_forward_ref(c["x"], c["o"], c["f"])
        s32, q32 = R.apply_forward_f32(c["x"], c["o"], c["f"])
        ds, do, Mds, Mdo = R.apply_backward_ref(c["x"], c["o"], c["f"], c["gs"], c["go"])
        ds32, do32 = R.apply_backward_f32(c["x"], c["o"], c["f"], c["gs"], c["go"])
        for name, e in (("scaling_eff", R.worst_units(s32, s, Ms)), ("opacity_eff", R.worst_units(q32, q, Mo)),
                        ("d_scaling", R.worst_units(ds32, ds, Mds)), ("d_opacity", R.worst_units(do32, do, Mdo))):
            worst[name] = max(worst[name], e)
    assert all(0 < v < 32 for v in worst.values()), worst
    return worst


@pytest.mark.parametrize("N", [1, 63, 65, 1000])
def test_apply_kernels_every_element_against_float64(device, f32_error, N):
    import diff_gaussian_rasterization as dgr

    c = R.build_apply_case(N)
    x = torch.from_numpy(c["x"]).to(device).requires_grad_(True)
    o = torch.from_numpy(c["o"]).to(device).requires_grad_(True)
    f = torch.from_numpy(c["f"]).to(device)
    s, q = dgr.filter3d_apply(x, o, f)
    torch.autograd.backward([s, q], [torch.from_numpy(c["gs"]).to(device), torch.from_numpy(c["go"]).to(device)])
    torch.cuda.synchronize()
    assert s.shape == (N, 3) and q.shape == (N, 1) and x.grad.shape == (N, 3) and o.grad.shape == (N, 1)
    got = dict(scaling_eff=s.detach().cpu().numpy(), opacity_eff=q.detach().cpu().numpy(),
               d_scaling=x.grad.cpu().numpy(), d_opacity=o.grad.cpu().numpy())
    ident = c["f"][:, 0] == 0
    for name, src in (("scaling_eff", "x"), ("opacity_eff", "o"), ("d_scaling", "gs"), ("d_opacity", "go")):
        assert np.array_equal(got[name][ident].view(np.int32), c[src][ident].view(np.int32)), \
            f"{name}: a row with f == 0 changed its bits"
    rs, rq, Ms, Mo = R.apply_forward_ref(c["x"], c["o"], c["f"])
    rds, rdo, Mds, Mdo = R.apply_backward_ref(c["x"], c["o"], c["f"], c["gs"], c["go"])
    seen = {}
    for name, ref, M in (("scaling_eff", rs, Ms), ("opacity_eff", rq, Mo), ("d_scaling", rds, Mds),
                         ("d_opacity", rdo, Mdo)):
        assert np.isfinite(got[name]).all(), name
        seen[name] = R.worst_units(got[name], ref, M)
    print(f"FILTER3D apply N={N}: kernel error in units of 2^-24 M {seen}; float32 numpy (worst of all N) {f32_error}")
    for name, e in seen.items():
        assert e <= 2.0 * f32_error[name], f"{name}: {e:.3g} units > 2 x {f32_error[name]:.3g}"


def test_apply_refuses_wrong_shapes_and_gives_f_no_gradient(device):
    import diff_gaussian_rasterization as dgr

    x = torch.zeros(5, 3, device=device, requires_grad=True)
    o = torch.zeros(5, 1, device=device, requires_grad=True)
    f = torch.full((5, 1), 0.1, device=device, requires_grad=True)
    s, q = dgr.filter3d_apply(x, o, f)
    (s.sum() + q.sum()).backward()
    assert f.grad is None and x.grad is not None and o.grad is not None
    with pytest.raises(ValueError, match="filter_3D"):
        dgr.filter3d_apply(x, o, f[:4])
    e = torch.zeros(0, 3, device=device), torch.zeros(0, 1, device=device), torch.zeros(0, 1, device=device)
    s, q = dgr.filter3d_apply(*e)
    assert s.shape == (0, 3) and q.shape == (0, 1)


# ------------------------------------------------------------------------------------------------ end to end
N_E2E, W_E2E, H_E2E, VIEWS = 300, 64, 48, (1, 2)


def _single_rank():
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=len(VIEWS), no_heuristics_update=True))
    utils.set_img_size(H_E2E, W_E2E)
    utils.set_cur_iter(1)
    wd._BALANCE["mode"] = "exact"
    gr._PLANNERS.clear()
    gr.set_exchange_forced(False)


def _model(device):
    return S.SyntheticGaussianModel(N_E2E, W_E2E, H_E2E, seed=5, sh_degree=3, device=device, scale_coef=0.02)


def _cameras(device):
    return S.orbit_cameras(4, W_E2E, H_E2E, device=device)


def _step(device, model, on):
    """forward + backward of the two views through the product's two calls -> dict(images, grads)"""
    import gaussian_renderer as gr
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    _single_rank()
    cams = _cameras(device)
    batch = [cams[v] for v in VIEWS]
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    strategies, _ = start_strategy_final(batch, hist)
    bg = torch.tensor([0.1, 0.2, 0.3], device=device)
    pipe = type("P", (), {"debug": False})()
    was = gr.get_filter3d()
    gr.set_filter3d(on)
    try:
        pkg = distributed_preprocess3dgs_and_all2all_final(batch, model, pipe, bg, batched_strategies=strategies,
                                                           mode="train")
        images, _ = render_final(pkg, strategies)
        wgt = torch.rand(3, H_E2E, W_E2E, generator=torch.Generator().manual_seed(4)).to(device)
        sum((im * wgt).sum() for im in images).backward()
    finally:
        gr.set_filter3d(was)
    torch.cuda.synchronize()
    return dict(images=[im.detach().clone() for im in images], pkg=pkg,
                grads={n: (getattr(model, n).grad.clone() if getattr(model, n).grad is not None else None) for n in ALL})


@pytest.fixture(scope="module")
def e2e(device):
    """filter off / filter on / the baked model with the filter off / a filter of zeros: computed once, not modified"""
    import filter3d as F

    _single_rank()
    cams = _cameras(device)
    on_model = _model(device)
    F.compute_3D_filter(on_model, cams)
    baked = _model(device)
    with torch.no_grad():
        s, o = F.bake(on_model)
        baked._scaling.copy_(s)
        baked._opacity.copy_(o)
    zero_model = _model(device)
    zero_model.filter_3D = torch.zeros(N_E2E, 1, device=device)
    return dict(off=_step(device, _model(device), False), on=_step(device, on_model, True),
                baked=_step(device, baked, False), zero=_step(device, zero_model, True), model=on_model, cams=cams)


def test_filtered_render_is_the_baked_model_s(e2e, f32_error):
    on, baked, off, model = e2e["on"], e2e["baked"], e2e["off"], e2e["model"]
    f = model.filter_3D
    assert f.shape == (N_E2E, 1) and bool((f > 0).all())
    for a, b, c in zip(on["images"], baked["images"], off["images"]):
        assert torch.equal(_bits(a), _bits(b)), "the filtered image is not the baked model's"
        assert not torch.equal(_bits(a), _bits(c)), "the filter changed nothing"
    for n in ("_xyz", "_rotation", "_features_dc", "_features_rest"):
        assert on["grads"][n] is not None and torch.equal(_bits(on["grads"][n]), _bits(baked["grads"][n])), n
    # _scaling / _opacity: the baked model's gradients through the float64 Jacobian of the apply step
    x, o = model._scaling.detach().cpu().numpy(), model._opacity.detach().cpu().numpy()
    gs, go = baked["grads"]["_scaling"].cpu().numpy(), baked["grads"]["_opacity"].cpu().numpy()
    ds, do, Mds, Mdo = R.apply_backward_ref(x, o, f.cpu().numpy(), gs, go)
    e_s = R.worst_units(on["grads"]["_scaling"].cpu().numpy(), ds, Mds)
    e_o = R.worst_units(on["grads"]["_opacity"].cpu().numpy(), do, Mdo)
    print(f"FILTER3D end to end: d_scaling {e_s:.3g}, d_opacity {e_o:.3g} units of 2^-24 M")
    assert bool(baked["grads"]["_scaling"].any()) and bool(baked["grads"]["_opacity"].any())
    assert e_s <= 2.0 * f32_error["d_scaling"] and e_o <= 2.0 * f32_error["d_opacity"]


def test_a_filter_of_zeros_is_the_unfiltered_model(e2e):
    off, zero = e2e["off"], e2e["zero"]
    for a, b in zip(off["images"], zero["images"]):
        assert torch.equal(_bits(a), _bits(b))
    for n in ALL:
        assert zero["grads"][n] is not None and torch.equal(_bits(off["grads"][n]), _bits(zero["grads"][n])), n


def test_bake_and_reset_opacity(device, e2e):
    import filter3d as F

    model = _model(device)
    model.filter_3D = e2e["model"].filter_3D.clone()
    with torch.no_grad():
        model._opacity[:10] = -6.0  # (rows whose filtered opacity is below 0.01 already)
        model._opacity[10:20] = 3.0
    s, o = F.bake(model)
    assert not s.requires_grad and not o.requires_grad
    x, q, f = model._scaling.detach().double(), model._opacity.detach().double(), model.filter_3D.double()
    s_prime = torch.sqrt(torch.exp(2 * x) + f * f)
    o_prime = torch.sigmoid(q) * torch.prod(torch.exp(x) / s_prime, dim=1, keepdim=True)
    assert torch.allclose(torch.exp(s.double()), s_prime, rtol=1e-5, atol=0)
    assert torch.allclose(torch.sigmoid(o.double()), o_prime, rtol=1e-5, atol=0)
    from fused_optim import FusedAdam

    model.optimizer = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15)
    before = model._opacity.detach().clone()
    keep = (o_prime <= 0.01).squeeze(1)
    F.reset_opacity_filter3d(model)
    assert model.optimizer.param_groups[3]["params"][0] is model._opacity and model._opacity.requires_grad
    _, o2 = F.bake(model)
    got = torch.sigmoid(o2.double()).squeeze(1)
    assert bool(keep.any()) and bool((~keep).any())
    assert torch.equal(_bits(model._opacity.detach()[keep]), _bits(before[keep]))
    assert torch.allclose(got[~keep], torch.full_like(got[~keep], 0.01), rtol=1e-4, atol=0)


@pytest.mark.parametrize("sparse", [False, True])
def test_fused_optimizer_declines_and_matches_the_unfused_step(device, e2e, sparse):
    from fused_optim import FusedAdam

    out = {}
    for fuse in (False, True):
        model = _model(device)
        model.filter_3D = e2e["model"].filter_3D.clone()
        opt = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=fuse, sparse=sparse and fuse)
        try:
            got = _step(device, model, True)
            assert all(got["grads"][n] is not None for n in ALL), "a parameter has no .grad after backward"
            for a, b in zip(got["images"], e2e["on"]["images"]):
                assert torch.equal(_bits(a), _bits(b))
            assert all("_gsr_defer_record" not in ca for ca in got["pkg"]["batched_cuda_args"])
            opt.step()
            torch.cuda.synchronize()
            assert opt.fused_steps == 0 and opt.materialized_steps == 0
        finally:
            opt.set_fuse_backward(False)
        out[fuse] = {n: getattr(model, n).detach().clone() for n in ALL}
        assert not torch.equal(out[fuse]["_scaling"], _model(device)._scaling.detach())
    for n in ALL:
        assert torch.equal(_bits(out[False][n]), _bits(out[True][n])), n


def test_missing_or_wrong_length_filter_raises(device):
    model = _model(device)
    with pytest.raises(RuntimeError, match="compute_3D_filter"):
        _step(device, model, True)
    model.filter_3D = torch.zeros(N_E2E - 1, 1, device=device)
    with pytest.raises(RuntimeError, match="compute_3D_filter"):
        _step(device, model, True)


def test_graph_capture_refuses(device, monkeypatch, e2e):
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    from graphed_step import GraphedIteration

    gr.set_filter3d(True)
    try:
        it = GraphedIteration(None, lambda *a: pytest.fail("the body ran"))
        with pytest.raises(RuntimeError, match="set_filter3d"):
            it([], [], [])
    finally:
        gr.set_filter3d(False)
    model = _model(device)
    model.filter_3D = e2e["model"].filter_3D.clone()
    monkeypatch.setattr(dgr, "_CAPTURE", [object()])  # what capturing() returns inside a graph capture
    with pytest.raises(RuntimeError, match="capture"):
        _step(device, model, True)
    monkeypatch.undo()
    assert dgr.capturing() is None and gr.get_filter3d() is False
