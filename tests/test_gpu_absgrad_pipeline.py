"""-m gpu: the absolute screen-space gradient through the Python layers -- gaussian_renderer.set_absgrad, the operator's
cuda_args["_gsr_absgrad"], collect_absgrad, densification_ops.update_densification_stats(..., absgrad=...).

Scene: the synthetic model of tests/test_gpu_invdepth_pipeline.py (2 000 Gaussians at 96 x 64, SH degree 1).
* switch off and on: the image, the loss and every parameter gradient keep their bits; no key and no tensor without it;
* switch on: every row has absgrad >= |means2D.grad[:, :2]| minus K units of the row (below), radius-0 rows are +0;
* the densification statistics with `absgrad` equal the torch formula on it; without it they are today's launch, bitwise;
* FusedAdam(fuse_backward=True), dense and sparse: the same bits as the plain path; graph capture raises;
* two bands on tests/fake_world.py: collect_absgrad of the two ranks, in the global rows, agrees with the one-rank tensor
  to 4 x 2^-24 per element, rows blended in one band only bitwise; a rank with the < 10-Gaussian stand-in takes part.

The slack of the inequality.  Both sides are sums over the same (pixel, entry) terms t; in exact arithmetic
sum |t| >= |sum t|.  The kernel's sum of magnitudes is within K units of the row of the exact one (tests/
test_gpu_absgrad_rows.py: K = composite_refs.K_GROUP["d_means2D"], a unit = helpers.ROW_UNIT_FLOOR = four half-ulps of the
row's largest value -- the floor of rows_unit, the smallest unit any case is checked with), and K10's fp32 sum of the
signed terms carries a rounding error that is a multiple of 2^-24 of sum |t| as well.  So the inequality is asserted with
K x ROW_UNIT_FLOOR x (the row's largest absgrad value) of room; the worst shortfall is printed in those units first."""
import pytest
import torch

import composite_refs as R
import synthetic_scene as S
from helpers import ROW_UNIT_FLOOR

pytestmark = pytest.mark.gpu

N, W, H, DEG, SCALE, SEED, VIEW = 2000, 96, 64, 1, 0.01, 5, 1
K = R.K_GROUP["d_means2D"]
ALL = ["_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest"]


def _single_rank(dev):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    wd._BALANCE["mode"] = "exact"
    gr._PLANNERS.clear()
    gr.set_exchange_forced(False)


def _model(dev):
    return S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, device=dev, scale_coef=SCALE)


def _weights(dev):
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).to(dev)


def _render(model, dev, world=1, rank=0, mode="train", view=VIEW):
    """-> (image, pkg, strategies) of one view through the product's two calls (the switch is the module's)"""
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    cams = S.orbit_cameras(4, W, H, device=dev)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), world, rank)
    views = list(view) if isinstance(view, (tuple, list)) else [view]
    batch = [cams[v] for v in views]
    strategies, _ = start_strategy_final(batch, hist)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    pkg = distributed_preprocess3dgs_and_all2all_final(batch, model, pipe, bg, batched_strategies=strategies, mode=mode)
    images, _ = render_final(pkg, strategies)
    return (images if isinstance(view, (tuple, list)) else images[0]), pkg, strategies


def _step(dev, on, model=None, view=VIEW):
    """one forward + backward on one rank -> dict(image, loss, grads, m2grad, radii, absgrad or None, pkg)"""
    import gaussian_renderer as gr

    _single_rank(dev)
    model = _model(dev) if model is None else model
    was = gr.get_absgrad()
    gr.set_absgrad(on)
    try:
        image, pkg, strategies = _render(model, dev, view=view)
        loss = (image * _weights(dev)).sum()
        loss.backward()
        a = gr.collect_absgrad(pkg, strategies)[0] if on else None
    finally:
        gr.set_absgrad(was)
    torch.cuda.synchronize()
    m2 = pkg["batched_locally_preprocessed_mean2D"][0]
    return dict(image=image.detach().clone(), loss=loss.detach().clone(), model=model, pkg=pkg, absgrad=a,
                grads={n: getattr(model, n).grad.clone() for n in ALL if getattr(model, n).grad is not None},
                m2grad=m2.grad[:, :2].clone(), m2=m2, radii=pkg["batched_locally_preprocessed_radii"][0])


@pytest.fixture(scope="module")
def plain(device):
    """the one-rank step with the switch off and on: computed once, never modified"""
    return _step(device, False), _step(device, True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_switch_off_and_on_keep_every_bit(plain):
    import diff_gaussian_rasterization as dgr

    off, on = plain
    assert all("absgrad" not in ca and dgr._ABSGRAD_KEY not in ca for ca in off["pkg"]["batched_cuda_args"])
    assert all(ca["absgrad"] is True and dgr._ABSGRAD_KEY in ca for ca in on["pkg"]["batched_cuda_args"])
    assert torch.equal(_bits(off["image"]), _bits(on["image"])) and torch.equal(_bits(off["loss"]), _bits(on["loss"]))
    assert set(off["grads"]) == set(on["grads"]) == set(ALL)
    for n in ALL:
        assert torch.equal(_bits(off["grads"][n]), _bits(on["grads"][n])), f"the gradient of {n} changed with the switch"
    assert torch.equal(_bits(off["m2grad"]), _bits(on["m2grad"])) and bool(on["grads"]["_xyz"].any())
    # world size 1: the operator's tensor itself
    assert on["absgrad"] is on["pkg"]["batched_cuda_args"][0][dgr._ABSGRAD_KEY]
    assert on["absgrad"].shape == (N, 2) and on["absgrad"].dtype == torch.float32


def test_absgrad_dominates_the_signed_gradient_on_every_row(plain):
    _, on = plain
    a, g, radii = on["absgrad"].double().cpu(), on["m2grad"].double().cpu().abs(), on["radii"].cpu()
    assert not bool(torch.isnan(a).any()) and bool((a >= 0).all())
    culled = radii <= 0
    assert bool(culled.any()) and not bool(_bits(on["absgrad"].cpu()[culled]).any()), "a radius-0 row is not +0.0f"
    unit = ROW_UNIT_FLOOR * a.amax(dim=1, keepdim=True)
    short = ((g - a) / unit.clamp(min=1e-300)).clamp(min=0)
    short = torch.where(unit > 0, short, torch.where(g > 0, torch.full_like(g, float("inf")), torch.zeros_like(g)))
    gain = float(a.sum() / g.sum())
    print(f"ABSGRAD-PIPE worst shortfall {float(short.max()):.3g} units of the row (K = {K}); sum absgrad / sum |grad| "
          f"= {gain:.3g}; rows with absgrad > 0: {int((a.amax(dim=1) > 0).sum())} of {N}")
    assert float(short.max()) <= K
    assert int((a.amax(dim=1) > 0).sum()) > N // 4 and gain > 1.0


def test_densification_statistics_with_and_without_absgrad(device, plain):
    import densification_ops as D
    import diff_gaussian_rasterization as dgr

    _, on = plain
    a, radii = on["absgrad"], on["radii"]

    class M:
        def __init__(self):
            g = torch.Generator().manual_seed(8)
            self.xyz_gradient_accum = torch.rand((N, 1), generator=g).to(device) * 1e-3
            self.denom = torch.randint(0, 5, (N, 1), generator=g).float().to(device)
            self.max_radii2D = torch.randint(0, 9, (N,), generator=g).float().to(device)

    vp = type("V", (), {})()
    vp.grad = on["m2grad"]
    today, now, absd, filt, ref = M(), M(), M(), M(), M()
    with torch.no_grad():
        dgr.densify_stats(radii, vp.grad, today.max_radii2D, today.xyz_gradient_accum, today.denom)  # today's launch
        D.update_densification_stats(now, vp, radii)
        D.update_densification_stats(absd, vp, radii, absgrad=a)
        D.add_densification_stats(filt, vp, radii > 0, absgrad=a)
        n = torch.linalg.vector_norm(a, dim=-1, keepdim=True)
        want = ref.xyz_gradient_accum + n
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(_bits(getattr(now, k)), _bits(getattr(today, k))), f"{k} without the argument moved"
    assert torch.equal(absd.denom, today.denom) and torch.equal(absd.max_radii2D, today.max_radii2D)
    assert torch.equal(filt.xyz_gradient_accum, want)  # (torch's own norm on both sides; culled rows add + 0)
    assert torch.equal(filt.denom, today.denom)
    # the one-launch kernel forms sqrt(fma(y, y, x x)): against torch's norm one rounding of the sum of squares (halved by
    # the root) and the root's own, 2^-23 of the norm; the addition into the accumulator is one fp32 add on both sides
    err = (absd.xyz_gradient_accum.double() - (ref.xyz_gradient_accum.double() + n.double())).abs()
    tol = 2.0 ** -23 * n.double() + 2.0 ** -24 * want.double().abs()
    print(f"ABSGRAD-PIPE statistics: worst error / tolerance {float((err / tol.clamp(min=1e-300)).max()):.3g}")
    assert bool((err <= tol).all())
    assert not torch.equal(absd.xyz_gradient_accum, today.xyz_gradient_accum)
    with pytest.raises(ValueError, match="absgrad"):
        D.update_densification_stats(M(), vp, radii, absgrad=a[:-1])


@pytest.mark.parametrize("sparse", [False, True])
def test_fused_backward_gives_the_same_bits(device, plain, sparse):
    from fused_optim import FusedAdam

    _, on = plain
    _single_rank(device)
    model = _model(device)
    opt = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=sparse)
    try:
        got = _step(device, True, model=model)
        assert torch.equal(_bits(got["absgrad"]), _bits(on["absgrad"])), "the fused path changed the absolute gradient"
        assert torch.equal(_bits(got["image"]), _bits(on["image"]))
        opt.step()
        torch.cuda.synchronize()
        assert opt.fused_steps == 1
        # (the kernel does not read the record, whose rounding this path leaves out until somebody looks: _step did)
        assert torch.equal(_bits(got["m2grad"]), _bits(on["m2grad"]))
    finally:
        opt.set_fuse_backward(False)


def test_graph_capture_refuses(device, monkeypatch):
    import diff_gaussian_rasterization as dgr
    from helpers import settings_from

    g = S.make_gaussians(300, W, H, seed=3, scale_coef=0.02)
    cam = S.orbit_cameras(4, W, H)[0]
    rast = dgr.GaussianRasterizer(settings_from(cam, torch.zeros(3), sh_degree=DEG, device=device))
    with torch.no_grad():
        m2, rgb, co, radii, depths = rast.preprocess_gaussians(*[g[k].to(device) for k in
                                                                 ("means3D", "scales", "rotations", "shs", "opacities")], {})
    m2 = m2.detach().requires_grad_(True)
    ca = {"absgrad": True}
    image = rast.render_gaussians(m2, co, rgb, depths, radii, None, None, ca)[0]
    assert dgr._ABSGRAD_KEY not in ca  # (the backward leaves it)
    image.sum().backward()
    a = ca[dgr._ABSGRAD_KEY]
    assert a.shape == (300, 2) and bool(a.any()) and bool((a >= m2.grad.abs() * (1 - 1e-3)).all())
    plain_ca = {}
    rast.render_gaussians(m2, co, rgb, depths, radii, None, None, plain_ca)[0].sum().backward()
    assert not any("absgrad" in k for k in plain_ca)
    monkeypatch.setattr(dgr, "_CAPTURE", [object()])  # what capturing() returns inside a graph capture
    with pytest.raises(RuntimeError, match="capture"):
        rast.render_gaussians(m2, co, rgb, depths, radii, None, None, {"absgrad": True})
    monkeypatch.undo()
    assert dgr.capturing() is None


# ------------------------------------------------------------------------------------------------ two bands
def _fake_world(device, make_model, world=2):
    """-> per rank dict(absgrad [P_local,2], own = this band's rows in GLOBAL numbering [n_total,2], scalar = the
    stand-in was taken, collectives)"""
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils
    import diff_gaussian_rasterization as dgr
    from fake_world import FakeWorld

    fw = FakeWorld(world, device)

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, world
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        wd._BALANCE["mode"] = "exact"
        gr._PLANNERS.clear()
        model = make_model(rank, world)
        image, pkg, strategies = _render(model, device, world, rank)
        scalar = image.dim() == 0
        loss = image if scalar else (image * _weights(device)).sum()
        loss.backward()
        before = len(fw.log)
        a = gr.collect_absgrad(pkg, strategies)[0]
        route = pkg["_absgrad_routes"][0]
        return dict(absgrad=a.clone(), scalar=scalar, P=model._xyz.shape[0], collectives=len(fw.log) - before,
                    rendered=pkg["batched_cuda_args"][0].get(dgr._ABSGRAD_KEY), send_idx=route[0].clone(),
                    send_splits=list(route[1]), recv_splits=list(route[2]))

    gr.set_absgrad(True)
    try:
        res = fw.run(rank_main, timeout=120)
    finally:
        gr.set_absgrad(False)
    print(f"ABSGRAD-PIPE fake world: rendezvous of the return trip per rank {[r['collectives'] for r in res]}, "
          f"{[t for _, t in fw.log][-2:]}")
    # the global row of every row a band rendered: source-major, the sources' send_idx segments
    first = [sum(r["P"] for r in res[:s]) for s in range(world)]
    total = sum(r["P"] for r in res)
    for d, r in enumerate(res):
        gids = []
        for s, src in enumerate(res):
            o = sum(src["send_splits"][:d])
            seg = src["send_idx"][o:o + src["send_splits"][d]].long()
            assert bool((seg >= 0).all()), "the exact layout of a first iteration has no padding rows"
            gids.append(seg + first[s])
        gids = torch.cat(gids)
        assert gids.numel() == sum(r["recv_splits"])
        r["own"] = torch.zeros(total, 2, device=device)
        if r["rendered"] is not None:
            assert r["rendered"].shape[0] == gids.numel()
            r["own"].index_add_(0, gids, r["rendered"])
    return res


def test_two_bands_agree_with_one_rank(device, plain):
    _, on = plain
    res = _fake_world(device, lambda rank, world: S.SyntheticGaussianModel(
        N, W, H, seed=SEED, sh_degree=DEG, rank=rank, world_size=world, device=device, scale_coef=SCALE))
    # (one all-to-all-v per camera on every rank: the stand-in collectives log the same rendezvous for both)
    assert not any(r["scalar"] for r in res) and res[0]["collectives"] == res[1]["collectives"] >= 1
    got = torch.cat([r["absgrad"] for r in res]).cpu()
    one = on["absgrad"].cpu()
    assert got.shape == one.shape == (N, 2)
    b0, b1 = res[0]["own"].cpu(), res[1]["own"].cpu()
    in0, in1 = b0.amax(dim=1) > 0, b1.amax(dim=1) > 0
    both, single = in0 & in1, in0 ^ in1
    print(f"ABSGRAD-PIPE two bands: {int(single.sum())} rows blended in one band, {int(both.sum())} in both")
    assert int(both.sum()) > 10 and int(in0.sum()) > 100 and int(in1.sum()) > 100
    assert torch.equal(_bits(got[single]), _bits(one[single])), "a row blended in one band only changed its bits"
    assert torch.equal(_bits(got[~(in0 | in1)]), _bits(one[~(in0 | in1)])) and not bool(got[~(in0 | in1)].any())
    # non-negative terms: two per-band roundings, one fp32 add, and the one-rank rounding -- 4 x 2^-24 per element
    err = (got.double() - one.double()).abs()
    rel = float((err / one.double().clamp(min=1e-300))[one > 0].max())
    print(f"ABSGRAD-PIPE two bands: worst relative difference {rel / 2.0 ** -24:.3g} x 2^-24")
    assert bool((err <= 4.0 * 2.0 ** -24 * one.double()).all())


def test_a_rank_with_the_stand_in_takes_part_and_sends_zeros(device):
    """a model whose Gaussians all end in the top tile row: rank 1's band receives nothing and takes the < 10-Gaussian
    stand-in; both ranks run the one return trip, and every row is blended in band 0 only: the one-rank bits"""
    import gaussian_renderer as gr

    _single_rank(device)
    full = _model(device)
    with torch.no_grad():
        _, pkg, _ = _render(full, device, mode="test")
        m2, radii = pkg["batched_locally_preprocessed_mean2D"][0], pkg["batched_locally_preprocessed_radii"][0]
        keep = ((radii > 0) & (m2[:, 1] + radii.float() + 1.0 < 16.0) & (m2[:, 1] - radii.float() > -8.0)
                & (m2[:, 0] > 0) & (m2[:, 0] < W)).nonzero().reshape(-1)
    n_keep = int(keep.numel())
    assert n_keep >= 24, f"only {n_keep} Gaussians end in the top tile row"

    def subset(rank, world):
        chunk = (n_keep + world - 1) // world
        rows = keep[rank * chunk:min((rank + 1) * chunk, n_keep)]
        m = _model(device)
        for n in ALL:
            setattr(m, n, torch.nn.Parameter(getattr(full, n).detach()[rows].clone().contiguous()))
        return m

    res = _fake_world(device, subset)
    assert [r["scalar"] for r in res] == [False, True], "rank 1 did not take the stand-in"
    assert res[1]["rendered"] is None and res[0]["collectives"] == res[1]["collectives"] >= 1
    assert not bool(res[1]["own"].any())
    _single_rank(device)
    one = _step(device, True, model=subset(0, 1))["absgrad"].cpu()
    got = torch.cat([r["absgrad"] for r in res]).cpu()
    assert got.shape == one.shape == (n_keep, 2) and bool(one.any())
    assert torch.equal(_bits(got), _bits(one))
    assert gr.get_absgrad() is False


def test_a_batch_of_two_cameras_on_two_ranks_keeps_a_route_per_camera(device):
    """bsz 2 at world size 2: with the switch on the exchange runs camera by camera, the package holds one route per
    camera, and each camera's collected rows agree with that camera's one-rank tensor (the bound of the two-band test)"""
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils
    from fake_world import FakeWorld

    world, views = 2, (VIEW, 2)
    fw = FakeWorld(world, device)

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, world
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        utils.set_args(utils.default_args(bsz=2, no_heuristics_update=True))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        wd._BALANCE["mode"] = "exact"
        gr._PLANNERS.clear()
        model = S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, rank=rank, world_size=world, device=device,
                                         scale_coef=SCALE)
        images, pkg, strategies = _render(model, device, world, rank, view=views)
        # (the division may give each rank one whole camera: a rank that renders no part of a camera sends zeros)
        mine = [im for im in images if im is not None]
        assert mine and all(im.dim() == 3 for im in mine)
        sum((im * _weights(device)).sum() for im in mine).backward()
        assert sorted(pkg["_absgrad_routes"]) == [0, 1]
        return [a.clone() for a in gr.collect_absgrad(pkg, strategies)]

    gr.set_absgrad(True)
    try:
        res = fw.run(rank_main, timeout=120)
    finally:
        gr.set_absgrad(False)
    for k, view in enumerate(views):
        one = _step(device, True, view=view)["absgrad"].double().cpu()
        got = torch.cat([r[k] for r in res]).double().cpu()
        assert got.shape == one.shape == (N, 2) and int((one.amax(dim=1) > 0).sum()) > N // 4
        err = (got - one).abs()
        print(f"ABSGRAD-PIPE batch of two, camera {k}: worst relative difference "
              f"{float((err / one.clamp(min=1e-300))[one > 0].max()) / 2.0 ** -24:.3g} x 2^-24")
        assert bool((err <= 4.0 * 2.0 ** -24 * one).all())
