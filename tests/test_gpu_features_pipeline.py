"""-m gpu: the N-channel feature map through the Python layers -- gaussian_renderer.set_features, pc.render_features,
render_final's pkg["batched_features"] -- against the float64 oracle chain (O.preprocess, O.bin_and_sort, O.render three
channels at a time with bg = 0).

Scene: 2 000 Gaussians at 96 x 64, SH degree 1, one rank, C = 5 channels (two oracle renders, the second zero-padded),
pc.render_features requiring grad.  Map, a seeded L2 loss on it and the gradients in xyz, opacity, scaling, rotation and
the features meet the norm-wise 1e-4 bar of tests/test_gpu_parity.py.  With the switch off and on the colour image and
the colour-only gradients keep their bits.  Features and inverse depth together give each one's own bits.
FusedAdam(fuse_backward=True), dense and sparse: the geometry gradients of the map reach the fused K11 + Adam launch
through autograd's sum with K10's record, and one fused step gives the unfused step's parameters bit for bit (the
dense launch its moments too; the sparse launch runs the batched row body: its moments meet the norm-wise bar).  The refusals raise: graph capture, world size 2 on tests/fake_world.py (before any collective), a missing or
mis-sized pc.render_features."""
import pytest
import torch

import synthetic_scene as S
from helpers import cam_kwargs, rel_err

pytestmark = pytest.mark.gpu

N, W, H, DEG, SCALE, SEED, VIEW, C = 2000, 96, 64, 1, 0.01, 5, 1, 5
RTOL = 1e-4
NAMES = ["_xyz", "_opacity", "_scaling", "_rotation"]
ALL = NAMES + ["_features_dc", "_features_rest"]


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


def _feature_rows():
    """float32 [N, C] in [0, 1], seeded"""
    return torch.rand(N, C, generator=torch.Generator().manual_seed(31))


def _render(model, dev, features, invdepth=False, mode="train", world=1, rank=0):
    """-> (image [3,H,W], the map [C,H,W] or None, the inverse-depth map or None, pkg) of view VIEW through the
    product's two calls; features None: the switches are the caller's (a fake world's ranks share the module)"""
    import gaussian_renderer as gr
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    cams = S.orbit_cameras(4, W, H, device=dev)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), world, rank)
    strategies, _ = start_strategy_final([cams[VIEW]], hist)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    was = gr.get_features(), gr.get_invdepth()
    if features is not None:
        gr.set_features(features)
        gr.set_invdepth(invdepth)
    try:
        pkg = distributed_preprocess3dgs_and_all2all_final([cams[VIEW]], model, pipe, bg, batched_strategies=strategies,
                                                           mode=mode)
        images, _ = render_final(pkg, strategies)
    finally:
        gr.set_features(was[0])
        gr.set_invdepth(was[1])
    return (images[0], pkg["batched_features"][0] if "batched_features" in pkg else None,
            pkg["batched_invdepth"][0] if "batched_invdepth" in pkg else None, pkg)


def _model(dev, grad=True):
    m = S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, device=dev, scale_coef=SCALE)
    m.render_features = _feature_rows().to(dev).requires_grad_(grad)
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def oracle():
    """the float64 chain on the host, once: map, target, loss, gradients"""
    from oracle import torch_oracle as O

    m = S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, device="cpu", scale_coef=SCALE)
    cam = S.orbit_cameras(4, W, H)[VIEW]
    kw = cam_kwargs(cam, DEG)
    mask = torch.ones((H + 15) // 16 * ((W + 15) // 16), dtype=torch.bool)
    raw = {n: getattr(m, n).detach().double().clone().requires_grad_(True) for n in ALL}
    f = _feature_rows().double().requires_grad_(True)
    shs = torch.cat([raw["_features_dc"], raw["_features_rest"]], dim=1)
    m2, rgb, co, radii, depths = O.preprocess(raw["_xyz"], torch.exp(raw["_scaling"]),
                                              torch.nn.functional.normalize(raw["_rotation"]), shs,
                                              torch.sigmoid(raw["_opacity"]), **kw)
    binning = O.bin_and_sort(m2, radii, depths, mask, W, H)
    maps = []
    for c0 in range(0, C, 3):
        n = min(3, C - c0)
        cols = torch.cat([f[:, c0:c0 + n], torch.zeros(N, 3 - n, dtype=torch.float64)], dim=1)
        img, _, _ = O.render(m2, co, cols, depths, radii, mask, bg=torch.zeros(3, dtype=torch.float64), W=W, H=H,
                             binning=binning)
        maps.append(img[:n])
    fmap = torch.cat(maps, dim=0)
    target = torch.rand(C, H, W, generator=torch.Generator().manual_seed(9))
    loss = ((fmap - target.double()) ** 2).mean()
    grads = torch.autograd.grad(loss, [raw[n] for n in NAMES] + [f])
    return dict(map=fmap.detach(), target=target, loss=float(loss), grads=dict(zip(NAMES + ["features"], grads)))


def test_map_loss_and_gradients_against_the_float64_oracle(device, oracle):
    _single_rank(device)
    model = _model(device)
    image, fmap, inv, pkg = _render(model, device, True)
    assert fmap is not None and fmap.shape == (C, H, W) and image.shape == (3, H, W) and inv is None
    loss = ((fmap - oracle["target"].to(device)) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    e_map, e_loss = rel_err(fmap, oracle["map"]), abs(float(loss) - oracle["loss"]) / oracle["loss"]
    print(f"FEATURES-PIPE map rel err {e_map:.3g}, loss {float(loss):.9g} vs {oracle['loss']:.9g} ({e_loss:.3g})")
    assert float(oracle["map"].max()) > 0.05 and e_map < RTOL and e_loss < RTOL
    for n in NAMES:
        e = rel_err(getattr(model, n).grad, oracle["grads"][n])
        print(f"FEATURES-PIPE d{n}: rel err {e:.3g}")
        assert e < RTOL, n
    e = rel_err(model.render_features.grad, oracle["grads"]["features"])
    print(f"FEATURES-PIPE d_features: rel err {e:.3g}")
    assert e < RTOL and bool(model.render_features.grad.any())
    # constant features: the map is the same bits, the geometry gradients are the same bits, no feature gradient
    const = _model(device, grad=False)
    _, fmap2, _, _ = _render(const, device, True)
    ((fmap2 - oracle["target"].to(device)) ** 2).mean().backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(fmap2), _bits(fmap)) and const.render_features.grad is None
    for n in NAMES:
        assert torch.equal(_bits(getattr(const, n).grad), _bits(getattr(model, n).grad)), n


def test_switch_off_and_on_keep_the_colour_bits(device):
    _single_rank(device)
    wgt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).to(device)
    out = {}
    for on in (False, True):
        model = _model(device)
        image, fmap, _, pkg = _render(model, device, on)
        assert (fmap is not None) == on and ("batched_features" in pkg) == on
        assert all(("features" in ca) == on for ca in pkg["batched_cuda_args"])
        assert not any("invdepth" in k for ca in pkg["batched_cuda_args"] for k in ca)
        (image * wgt).sum().backward()
        torch.cuda.synchronize()
        out[on] = (image.detach().clone(), {n: getattr(model, n).grad.clone() for n in ALL})
    assert torch.equal(out[False][0], out[True][0]), "the colour image changed with the switch"
    for n in ALL:
        assert torch.equal(out[False][1][n], out[True][1][n]), f"the colour-only gradient of {n} changed with the switch"
    assert bool(out[True][1]["_xyz"].any())


def test_features_and_inverse_depth_together_give_each_ones_own_bits(device):
    _single_rank(device)
    gen = torch.Generator().manual_seed(12)
    wf, wi = torch.rand(C, H, W, generator=gen).to(device), torch.rand(1, H, W, generator=gen).to(device)
    res = {}
    # (switches, the map the loss is on)
    for key, (feat, invd, on) in dict(f=(True, False, "f"), i=(False, True, "i"), both_f=(True, True, "f"),
                                      both_i=(True, True, "i")).items():
        model = _model(device)
        _, fmap, inv, _ = _render(model, device, feat, invdepth=invd)
        assert (fmap is not None) == feat and (inv is not None) == invd
        ((fmap * wf).sum() if on == "f" else (inv * wi).sum()).backward()
        torch.cuda.synchronize()
        res[key] = (None if fmap is None else fmap.detach().clone(), None if inv is None else inv.detach().clone(),
                    {n: getattr(model, n).grad.clone() for n in NAMES},
                    None if model.render_features.grad is None else model.render_features.grad.clone())
    assert torch.equal(_bits(res["both_f"][0]), _bits(res["f"][0])), "the feature map changed beside the inverse depth"
    assert torch.equal(_bits(res["both_i"][1]), _bits(res["i"][1])), "the inverse-depth map changed beside the features"
    for n in NAMES:
        assert torch.equal(_bits(res["both_f"][2][n]), _bits(res["f"][2][n])), f"features: d{n}"
        assert torch.equal(_bits(res["both_i"][2][n]), _bits(res["i"][2][n])), f"inverse depth: d{n}"
        assert bool(res["f"][2][n].any()) and not torch.equal(res["f"][2][n], res["i"][2][n])
    assert torch.equal(_bits(res["both_f"][3]), _bits(res["f"][3])) and res["both_i"][3] is None


@pytest.mark.parametrize("sparse", [False, True])
def test_one_fused_step_equals_the_unfused_step(device, sparse):
    """the map's geometry gradients and K10's are summed by autograd in front of the projection backward, which
    FusedAdam(fuse_backward=True) runs inside its step: the parameters after one step, bit for bit.
    Dense: the moments too, bit for bit -- the fused launch and the unfused K11 of a one-camera step are the same
    one-camera row body with the host's tan(fov / 2).  Sparse: its launch is the BATCHED row body, which reads the
    tangents from the packed camera block (fused_step passes it no host tangents), so against the one-camera unfused K11
    its gradients -- the first moments are 0.1 x them -- may differ in the last bit, with the map or without it;
    tests/test_gpu_sparse_adam.py holds that launch to the batched pair bit for bit.  Here its moments meet the
    norm-wise gradient bar of this file, and they contain the map's gradient."""
    from fused_optim import FusedAdam

    wgt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).to(device)
    target = torch.rand(C, H, W, generator=torch.Generator().manual_seed(9)).to(device)

    def run(fuse):
        _single_rank(device)
        model = _model(device)
        opt = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=fuse, sparse=sparse and fuse)
        try:
            image, fmap, _, _ = _render(model, device, True)
            ((image * wgt).sum() + ((fmap - target) ** 2).sum()).backward()
            assert all((getattr(model, n).grad is None) == fuse for n in ALL)
            opt.step()
            torch.cuda.synchronize()
            assert opt.fused_steps == (1 if fuse else 0)
            return [getattr(model, n).detach().clone() for n in ALL] + \
                [opt.state[getattr(model, n)][k].clone() for n in ALL for k in ("exp_avg", "exp_avg_sq")] + \
                [model.render_features.grad.clone()]
        finally:
            opt.set_fuse_backward(False)

    unfused, fused = run(False), run(True)
    for j, (x, y) in enumerate(zip(unfused, fused)):
        if sparse and len(ALL) <= j < 3 * len(ALL):
            e = rel_err(y, x)
            print(f"FEATURES-PIPE sparse step, moment {j - len(ALL)}: rel err {e:.3g}, "
                  f"{int((_bits(x) != _bits(y)).sum())} words differ")
            assert e < RTOL, f"tensor {j}: the sparse step's moment is off"
        else:
            assert torch.equal(_bits(x), _bits(y)), f"tensor {j}: the fused and the unfused step differ"
    # the map's gradients are in that step: the colour-only moments are others
    _single_rank(device)
    model = _model(device)
    opt = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=False)
    image, _, _, _ = _render(model, device, False)
    (image * wgt).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    colour_only = opt.state[model._xyz]["exp_avg"]
    assert not torch.equal(colour_only, unfused[len(ALL)]), "the feature loss moved nothing"
    assert rel_err(fused[len(ALL)], colour_only) > 100 * RTOL, "the fused step did not see the map's gradient"


def test_graph_capture_refuses_the_map(device, monkeypatch):
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    from helpers import settings_from

    g = S.make_gaussians(300, W, H, seed=3, scale_coef=0.02)
    cam = S.orbit_cameras(4, W, H)[0]
    rast = dgr.GaussianRasterizer(settings_from(cam, torch.zeros(3), sh_degree=DEG, device=device))
    feat = torch.rand(300, 3, generator=torch.Generator().manual_seed(2)).to(device)
    with torch.no_grad():
        m2, rgb, co, radii, depths = rast.preprocess_gaussians(*[g[k].to(device) for k in
                                                                 ("means3D", "scales", "rotations", "shs", "opacities")], {})
        ca = {"features": True}
        rast.render_gaussians(m2, co, rgb, depths, radii, None, None, ca)
        fmap = rast.render_features(m2, co, feat, ca)
        assert fmap.shape == (3, H, W) and bool(fmap.any()) and dgr._INVDEPTH_KEY not in ca
        with pytest.raises(RuntimeError, match="cuda_args\\['features'\\]"):
            rast.render_features(m2, co, feat, {})
        with pytest.raises(ValueError, match="rows of the view"):
            rast.render_features(m2, co, feat[:-1], ca)
        with pytest.raises(ValueError, match="channels"):
            rast.render_features(m2, co, torch.zeros(300, dgr.FEATURES_MAX + 1, device=device), ca)
        monkeypatch.setattr(dgr, "_CAPTURE", [object()])  # what capturing() returns inside a graph capture
        with pytest.raises(RuntimeError, match="capture"):
            rast.render_gaussians(m2, co, rgb, depths, radii, None, None, {"features": True})
        with pytest.raises(RuntimeError, match="capture"):
            rast.render_features(m2, co, feat, ca)
        _single_rank(device)
        with pytest.raises(RuntimeError, match="capture"):
            _render(_model(device), device, True, mode="test")
        monkeypatch.undo()
    assert dgr.capturing() is None and not gr.get_features()


def test_a_missing_or_mis_sized_feature_tensor_raises(device):
    _single_rank(device)
    model = _model(device)
    for bad in (None, model.render_features.detach()[:-1], model.render_features.detach()[:, 0],
                model.render_features.detach().double(), model.render_features.detach().cpu()):
        if bad is None:
            del model.render_features
        else:
            model.render_features = bad
        with pytest.raises(ValueError, match="render_features"):
            _render(model, device, True)
    # with the switch off nobody looks
    image, fmap, _, _ = _render(model, device, False)
    assert fmap is None and image.shape == (3, H, W)


def test_world_size_two_is_refused_before_any_collective(device):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils
    from fake_world import FakeWorld

    world = 2
    fw = FakeWorld(world, device)

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, world
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        wd._BALANCE["mode"] = "exact"
        gr._PLANNERS.clear()
        model = S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, rank=rank, world_size=world, device=device,
                                         scale_coef=SCALE)
        model.render_features = torch.zeros(model._xyz.shape[0], C, device=device)
        before = len(fw.log)
        try:
            _render(model, device, None, world=world, rank=rank)
        except NotImplementedError as e:
            return dict(refused="world size" in str(e), collectives=len(fw.log) - before)
        return dict(refused=False, collectives=len(fw.log) - before)

    gr.set_features(True)
    try:
        res = fw.run(rank_main, timeout=120)
    finally:
        gr.set_features(False)
        _single_rank(device)
    assert all(r["refused"] for r in res), "world size 2 was not refused"
    assert all(r["collectives"] == 0 for r in res) and len(fw.log) == 0, f"a collective ran: {fw.log}"
